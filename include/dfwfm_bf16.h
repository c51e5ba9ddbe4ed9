/*
 * dfwfm_bf16.h -- C ABI of the inference forward with a bf16 deep tower (libdfwfm.so, beside include/dfwfm.h and
 * include/dfwfm_serve.h).
 *
 * The logits of dfwfm_forward -- `DeepFMs.forward(Xi, Xv)` (reference model/DeepFMs.py:285-469) -- with the hidden
 * layers of the deep tower on gfx950's bf16 matrix pipe (v_mfma_f32_16x16x32_bf16, f32 accumulation) instead of the
 * f32 one: the engine's answer to the reference's static_quantization axis (a cheaper forward at nearly the same
 * AUC).  The gather, the first order and the FwFM / FM second order stay in exact f32.  The call is the gather launch,
 * one launch per hidden layer and a small combine launch: H + 2 stream-ordered launches, no workgroup waiting on
 * another, no atomics.
 *
 * Opt-in: nothing in include/dfwfm.h changes or routes here.  A model with a deep tower only.
 *
 * The numeric contract.  For hidden layers l = 1..H with weights W_l [N_l, K_l], biases b_l, and the output weights fc:
 *   1. E[b, f, :] is the f32 row the f32 forward uses: the table row of a categorical field (or the QR product / sum,
 *      in f32), the single f32 multiply v_f[0] * Xv[b, f] of a numerical field.  The first + second order of the row is
 *      the f32 value dfwfm_forward_gather writes to first_second, the same bits.
 *   2. x_0 = bf16(deep_emb), the row's E values in field order; bf16() is round-to-nearest-even of the f32 value
 *      (v_cvt_pk_bf16_f32), NaN stays NaN.
 *   3. Wb_l = bf16(W_l), converted once by dfwfm_model_pack_bf16, not per call.
 *   4. z_l[n] = sum_k x_{l-1}[k] Wb_l[n, k], accumulated in f32 on MFMA (a product of two bf16 values is exact in f32),
 *      in an order fixed by the layer's shape alone: K steps of 32 in ascending k into one accumulator.
 *   5. h_l = relu(z_l + b_l) in f32, b_l in f32; relu keeps NaN.
 *   6. x_l = bf16(h_l) for l < H; h_H is not rounded.
 *   7. deep = sum_n h_H[n] fc[n] in f32, fc in f32, in a fixed order (per 16 neurons, then the groups in ascending n).
 *   8. logit = (first_second + deep) + bias.
 * A row's logit is a function of that row's inputs and the parameters alone: the same bits for any batch size, row
 * position, workspace contents and run.  NaN and Inf propagate as in the f32 path; subnormal handling is unspecified.
 *
 * Nothing model-owned is written per call except the sticky error flag (as in dfwfm_forward): every intermediate
 * lives in the caller's workspace, so calls on two streams with two workspaces may overlap, and a call makes no
 * allocation or synchronisation and is capturable into a HIP graph (after one eager call of the same model, as for
 * dfwfm_forward).
 *
 * Status codes, dfwfm_last_error and the sticky index flag (dfwfm_read_error_flag) as in dfwfm.h.
 */
#ifndef DFWFM_BF16_H
#define DFWFM_BF16_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_BF16_ABI_VERSION 1

int dfwfm_bf16_abi_version(void);

/* enable != 0: (re)build the model-owned bf16 copy of the hidden layers' weights in MFMA operand order from the dense
 * parameters currently set (the caller's weight tensors of the last dfwfm_model_set_dense, read on `stream`).
 * Stream-ordered with no host synchronisation; the first enable of a model allocates the copy (2 bytes per padded
 * weight).  enable == 0: drop it (the memory is released with the model).  dfwfm_model_set_dense invalidates the copy.
 * DFWFM_ERR_UNSUPPORTED: no deep tower; DFWFM_ERR_STATE: dense parameters not yet set. */
int dfwfm_model_pack_bf16(dfwfm_model* m, int enable, void* stream);

/* bytes of 16-byte-aligned device scratch a call of `batch` rows needs (f32 deep_emb, first + second, the last
 * layer's per-tile partial sums, two bf16 activation buffers), sized for ceil(batch / 16) * 16 rows; host-only, no
 * launch.  DFWFM_ERR_UNSUPPORTED for a model without a deep tower. */
int dfwfm_bf16_workspace_bytes(dfwfm_model* m, int64_t batch, size_t* bytes);

/* logits[b], b < batch: the arguments of dfwfm_serve_forward (out-of-range indices read row 0 and set the sticky
 * flag), the workspace's contents on entry arbitrary and on return unspecified.  batch == 0: OK, no launch.
 * DFWFM_ERR_INVALID_ARG: a null pointer, a workspace smaller than dfwfm_bf16_workspace_bytes(batch) (the message
 * names the size) or not 16-byte aligned; DFWFM_ERR_UNSUPPORTED: no deep tower, or a batch too large for one launch;
 * DFWFM_ERR_STATE: tables or dense parameters not yet set, or the bf16 copy absent or stale. */
int dfwfm_bf16_forward(dfwfm_model* m, const int64_t* xi, int64_t xi_stride, const float* xv, int64_t xv_stride,
                       int64_t batch, float* out, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_BF16_H */
