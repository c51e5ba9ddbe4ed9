/*
 * dfwfm_serve.h -- C ABI of the small-batch serving forward (libdfwfm.so, beside include/dfwfm.h).
 *
 * The same logits as dfwfm_forward -- `DeepFMs.forward(Xi, Xv)` (reference model/DeepFMs.py:285-469) -- for the
 * call pattern of online serving and of the reference's own latency benchmark (1000 single-sample forwards,
 * model/DeepFMs.py:999-1009): one request or a handful of candidates per call.  dfwfm_forward gives every 16-row
 * tile to one workgroup, which carries it through the gather, the FwFM and every hidden layer; a batch below about
 * a thousand rows then leaves most of the chip idle while a few CUs run the layers one after the other.  This
 * forward runs the gather / shallow half as one launch and every hidden layer as a launch of its own, one workgroup
 * per 16 x 16 output tile, then a small combine launch: H + 2 stream-ordered launches, no workgroup waiting on
 * another, no atomics.
 *
 * Opt-in: nothing in include/dfwfm.h changes or routes here.  A model with a deep tower only (an MLP-free model's
 * whole forward is already one short launch).  Nothing model-owned is written per call except the sticky error flag
 * (as in dfwfm_forward): every intermediate lives in the caller's workspace, so calls on two streams with two
 * workspaces may overlap, and a call makes no allocation or synchronisation and is capturable into a HIP graph
 * (after one eager call of the same model, as for dfwfm_forward).
 *
 * A row's logit is a function of that row's inputs and the parameters alone: independent of the batch size, of the
 * row's position and of the workspace's previous contents, the same bits on every run.  It agrees with
 * dfwfm_forward's to rounding (a different, also fixed, summation order), not bit for bit.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.
 */
#ifndef DFWFM_SERVE_H
#define DFWFM_SERVE_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_SERVE_ABI_VERSION 1

int dfwfm_serve_abi_version(void);

/* bytes of 16-byte-aligned device scratch a call of `batch` rows needs (deep_emb, first + second, two activation
 * buffers, the last layer's per-tile partial sums), sized for ceil(batch / 16) * 16 rows; host-only, no launch.
 * DFWFM_ERR_UNSUPPORTED for a model without a deep tower. */
int dfwfm_serve_workspace_bytes(dfwfm_model* m, int64_t batch, size_t* bytes);

/* logits[b], b < batch: the same arguments and logits contract as dfwfm_forward (out-of-range indices read row 0
 * and set the sticky flag of dfwfm_read_error_flag), plus the workspace, whose contents on entry are arbitrary and
 * on return unspecified.  batch == 0: OK, no launch.  DFWFM_ERR_INVALID_ARG: a null pointer, a workspace smaller than
 * dfwfm_serve_workspace_bytes(batch) (the message names the size) or not 16-byte aligned; DFWFM_ERR_UNSUPPORTED:
 * no deep tower, or more than 2^31 - 1 workgroups in a layer's launch (ceil(batch / 16) * ceil(deep_nodes / 16));
 * DFWFM_ERR_STATE: tables or dense parameters not yet set. */
int dfwfm_serve_forward(dfwfm_model* m, const int64_t* xi, int64_t xi_stride, const float* xv, int64_t xv_stride,
                        int64_t batch, float* out, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_SERVE_H */
