/*
 * dfwfm_int8.h -- C ABI of the one-launch inference forward with an int8 deep tower (libdfwfm.so, beside
 * include/dfwfm_bf16_fused.h, whose calls these mirror).
 *
 * The logits of dfwfm_forward with the hidden layers of the deep tower on gfx950's int8 matrix pipe
 * (v_mfma_i32_16x16x64_i8, int32 accumulation): weights quantized per output neuron once per weight update,
 * activations quantized per row and per layer, dynamically and symmetrically.  One launch from Xi / Xv to the logits,
 * the E tile and the activations in LDS, 16 or 32 rows of one batch per workgroup; batch sets as dfwfm_forward_batches.
 * There is no per-layer int8 path and no numerical fold.
 *
 * Opt-in: nothing in the other headers changes or routes here.  A model with a deep tower only.
 *
 * The numeric contract.  All arithmetic is IEEE f32 unless it says integer; a division is the correctly rounded f32
 * division; rint rounds to nearest, ties to even (v_rndne_f32).  Hidden layers l = 1..H with weights W_l [N_l, K_l],
 * biases b_l, the output weights fc.
 *   0. Everything outside the hidden layers is the f32 forward's arithmetic: E[b, f, :], the first order and the
 *      FwFM / FM second order are the expressions of the one-launch bf16 forward's stage 1, so first + second are the
 *      bits dfwfm_forward_gather writes, and x_0 is the f32 deep_emb row (E in field order).
 *   1. Weights, formed once by dfwfm_model_pack_int8.  For layer l and neuron n:
 *        aw       = max_k |W_l[n, k]|; the max propagates NaN, as the activations' max of step 2 does
 *        sw[l][n] = aw / 127, or 1 when aw == 0
 *        qW[n, k] = clamp(rint(W_l[n, k] / sw[l][n]), -127, 127); 0 where W_l[n, k] / sw[l][n] is NaN
 *      padded neurons and padded k are 0.
 *   2. Activations, per row and per layer:
 *        a    = max_k |x_{l-1}[k]| over the layer's real K inputs; the max propagates NaN
 *        inv  = 127 / a and sx = a / 127, both 0 when a == 0
 *        q[k] = clamp(rint(x[k] * inv), -127, 127); 0 where x[k] * inv is NaN
 *   3. acc[n] = sum_k q[k] qW[n, k] in int32: exact, |acc| <= 512 * 127^2 < 2^24, so (float)acc is exact too.
 *   4. t = sx * sw[l][n];  h_l[n] = relu(fmaf((float)acc[n], t, b_l[n])), relu keeps NaN.
 *   5. For l < H, h_l in f32 is x_l: no intermediate rounding besides the quantization.  h_H is not quantized.
 *   6. deep = sum_n h_H[n] fc[n] in f32, fc in f32, per 16 neurons then the groups in ascending n; logit =
 *      (first_second + deep) + bias: the last two steps of the contract of dfwfm_bf16.h.
 *
 * Consequences.
 *   - Integer accumulation is exact and independent of order: every hidden sum is the same integer whatever the tile,
 *     the wave split or the K order.  A row's logit depends on the row and the parameters only: not on the batch
 *     size, the row's position, the row tile chosen or the batch set.
 *   - A row whose tower input holds a NaN or an infinity gets a NaN logit (a = inf: every q is 0, acc = 0 times
 *     sx = inf is NaN; a = NaN: sx is NaN).  Other rows are untouched.
 *   - A neuron whose weight row holds a NaN or an infinity is NaN for every row (aw = NaN: sw is NaN; aw = inf: every
 *     qW is 0 and acc = 0 times sw = inf is NaN), and so is every logit, as in the f32 and bf16 forwards of the same
 *     model.  A NaN or infinite bias, fc weight or model bias reaches the logits through the f32 steps 4 and 6.  A
 *     diverged model is never served as a finite one.
 *   - This is not fbgemm's dynamic quantization (one activation scale per tensor over the whole batch, 7-bit
 *     activations, per-tensor weights), which would make a row's logit depend on its batch neighbours.
 *
 * Guarantees, as dfwfm_bf16_fused.h: the forward calls take no workspace and write nothing model-owned except the
 * sticky index flag (out-of-range indices read row 0 and set it, dfwfm_read_error_flag); they make no allocation and
 * no synchronisation, are capturable into a HIP graph after one eager call of the same model, and calls on two
 * streams may overlap.  batch == 0 or nb == 0: DFWFM_OK, no launch.
 *
 * Supported shapes, the set of the fused bf16 forward: embedding_size 10, field_size <= 48, deep_nodes <= 512, any
 * h_depth >= 1; plain, EmbeddingBag and QR tables, the tables' serving copy, every first order, FwFM and FM.  Not
 * while a pruned FwFM pair list is on (dfwfm_model_build_fwfm_pairs).  Everything else is DFWFM_ERR_UNSUPPORTED.
 *
 * Errors: DFWFM_ERR_INVALID_ARG for a null pointer (or a stride below the row width); DFWFM_ERR_UNSUPPORTED for a
 * model without a deep tower, an unsupported shape or a grid too large for one launch; DFWFM_ERR_STATE for tables or
 * dense parameters not yet set, or the int8 pack absent or stale after dfwfm_model_set_dense.  No call aborts.  Status
 * codes and dfwfm_last_error as in dfwfm.h.
 */
#ifndef DFWFM_INT8_H
#define DFWFM_INT8_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_INT8_ABI_VERSION 1

int dfwfm_int8_abi_version(void);

/* (re)build the model-owned int8 pack of the hidden layers from the dense parameters currently set (the caller's
 * weight tensors of the last dfwfm_model_set_dense, read on `stream`): the int8 weights in MFMA operand order, the
 * per-neuron scales sw and the biases.  One launch, the sources as kernel arguments: no staging buffer, no host
 * synchronisation; the first call of a model allocates the pack.  dfwfm_model_set_dense marks it stale.
 * DFWFM_ERR_UNSUPPORTED: no deep tower, or a shape the forward calls do not run; DFWFM_ERR_STATE: dense parameters
 * not yet set. */
int dfwfm_model_pack_int8(dfwfm_model* m, void* stream);

/* *supported = 1 when the calls below run this model (its shape, and no FwFM pair list on), else 0; host-only, no
 * launch.  DFWFM_ERR_INVALID_ARG: a null pointer. */
int dfwfm_int8_supported(dfwfm_model* m, int* supported);

/* logits[b], b < batch: the arguments of dfwfm_bf16_fused_forward. */
int dfwfm_int8_forward(dfwfm_model* m, const int64_t* xi, int64_t xi_stride, const float* xv, int64_t xv_stride,
                       int64_t batch, float* out, void* stream);

/* the forward of nb batches of `batch` rows each (the same strides), batch i from xi[i] / xv[i] into out[i]: the
 * arguments of dfwfm_bf16_fused_forward_batches (up to 32 batches per launch, further launches beyond); every
 * batch's logits are those of its own dfwfm_int8_forward, bit for bit. */
int dfwfm_int8_forward_batches(dfwfm_model* m, int32_t nb, const int64_t* const* xi, int64_t xi_stride,
                               const float* const* xv, int64_t xv_stride, int64_t batch, float* const* out,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_INT8_H */
