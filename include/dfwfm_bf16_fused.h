/*
 * dfwfm_bf16_fused.h -- C ABI of the one-launch form of the forward with a bf16 deep tower (libdfwfm.so, beside
 * include/dfwfm_bf16.h, whose numeric contract it implements).
 *
 * dfwfm_bf16_forward is H + 2 stream-ordered launches with the f32 E rows, every bf16 activation and the last
 * layer's shares in a caller's workspace.  The calls here are ONE launch: a workgroup carries a tile of 16, 32 or 64
 * rows of one batch from Xi / Xv to the logits, the E tile and the activations in LDS, the hidden layers on
 * v_mfma_f32_16x16x32_bf16 from the same weight pack (dfwfm_model_pack_bf16) -- and, as dfwfm_forward_batches, a set
 * of batches per launch (up to 32; larger sets take further launches).
 *
 * Contract.
 *   - The logits are those of dfwfm_bf16_forward, bit for bit, for every row: the contract of dfwfm_bf16.h fixes
 *     every sum's order by the layer's shape alone, and the shallow half is the arithmetic of dfwfm_forward_gather.
 *     So a row's logit does not depend on the batch size, the row's position, the tile size chosen or the set.
 *   - The calls take no workspace and write nothing model-owned except the sticky index flag (out-of-range indices
 *     read row 0 and set it, dfwfm_read_error_flag); they make no allocation and no synchronisation, are capturable
 *     into a HIP graph after one eager call of the same model, and calls on two streams may overlap.
 *   - batch == 0 or nb == 0: DFWFM_OK, no launch.
 *   - Supported shapes: embedding_size 10, field_size <= 48, deep_nodes <= 512, any h_depth >= 1; plain,
 *     EmbeddingBag and QR tables, the tables' serving copy, every first order, FwFM and FM.  Not while a pruned
 *     FwFM pair list is on (dfwfm_model_build_fwfm_pairs: the gather launch then sums in another order).
 *     Everything else is DFWFM_ERR_UNSUPPORTED: the caller keeps dfwfm_bf16_forward.
 *
 * Errors, as dfwfm_bf16_forward: DFWFM_ERR_INVALID_ARG for a null pointer (or a stride below the row width);
 * DFWFM_ERR_UNSUPPORTED for a model without a deep tower, an unsupported shape or a grid too large for one launch;
 * DFWFM_ERR_STATE for tables or dense parameters not yet set, or the bf16 copy absent or stale after
 * dfwfm_model_set_dense.  No call aborts.  Status codes and dfwfm_last_error as in dfwfm.h.
 */
#ifndef DFWFM_BF16_FUSED_H
#define DFWFM_BF16_FUSED_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_BF16_FUSED_ABI_VERSION 1

int dfwfm_bf16_fused_abi_version(void);

/* *supported = 1 when the calls below run this model (its shape, and no FwFM pair list on), else 0; host-only, no
 * launch.  DFWFM_ERR_INVALID_ARG: a null pointer. */
int dfwfm_bf16_fused_supported(dfwfm_model* m, int* supported);

/* logits[b], b < batch: the arguments of dfwfm_forward. */
int dfwfm_bf16_fused_forward(dfwfm_model* m, const int64_t* xi, int64_t xi_stride, const float* xv,
                             int64_t xv_stride, int64_t batch, float* out, void* stream);

/* the forward of nb batches of `batch` rows each (the same strides), batch i from xi[i] / xv[i] into out[i]: the
 * arguments of dfwfm_forward_batches; every batch's logits are those of its own dfwfm_bf16_fused_forward. */
int dfwfm_bf16_fused_forward_batches(dfwfm_model* m, int32_t nb, const int64_t* const* xi, int64_t xi_stride,
                                     const float* const* xv, int64_t xv_stride, int64_t batch, float* const* out,
                                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_BF16_FUSED_H */
