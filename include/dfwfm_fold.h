/*
 * dfwfm_fold.h -- C ABI of the folded layer 1 of the fused inference forward (libdfwfm.so, beside include/dfwfm.h,
 * include/dfwfm_serve.h and include/dfwfm_bf16.h).
 *
 * The embedding of a numerical field is not data: E[b, f, :] = Xv[b, f] * v_f[0], one constant row per field times a
 * per-sample scalar (reference model/DeepFMs.py:297-299).  Layer 1 of the deep tower therefore receives from
 * numerical field f, at neuron n, Xv[b, f] * P[f][n] with
 *     P[f][n] = sum_d W1[n, f D + d] * v_f[0][d],
 * which depends on the weights alone.  With P built once per weight update, layer 1 contracts over
 * (F - num) D + num columns instead of F D: 18 K chunks of 16 instead of 25 at Criteo-39 (39 fields, 13 numerical,
 * D = 10), 7 of the 75 chunks of the 3 x 400 tower.
 *
 * Opt-in: nothing in include/dfwfm.h changes.  Only dfwfm_forward and dfwfm_forward_batches (the fused inference
 * kernels) read the folded pack; the training forward, dfwfm_serve_forward, dfwfm_bf16_forward, dfwfm_forward_ws and
 * dfwfm_forward_gather keep reading the unfolded layer 1, which stays in place.
 *
 * The numeric contract.  With the fold on, layer 1 is
 *     z_1[b, n] = b_1[n] + sum_{k ascending} x[b, k] * Wf[n, k]
 * accumulated in f32 on MFMA from the bias, over the folded K rows in this order:
 *   1. k < (F - num) D: x = the categorical columns of deep_emb in field order (E[b, f, d], f >= num), Wf = the same
 *      columns of W1, bit for bit;
 *   2. the next num rows: x = Xv[b, f], Wf = P[f][n], f = 0..num-1.  P[f][n] is accumulated in f64 over d = 0..D-1 in
 *      that order (each product of two f32 values is exact in f64) and rounded to f32 once;
 *   3. zeros up to the pack's chunk count (x and Wf both exactly 0).
 * The split output tile's partial sums are added in wave order, as in the unfolded forward.  Layers 2..H, the first
 * order and the FwFM / FM second order are unchanged.  The order is the same in every kernel form, and whether a
 * model folds is decided per model, never per launch: a row's logit is the same bits for any batch size, batch set,
 * row position and kernel form (16- or 32-sample workgroups, four or eight waves).
 * This is a re-association of f32 sums, not a change of precision: the folded logits are within
 * 1e-5 * max(1, |ref|) of the unfolded forward's and of the float64 oracle.  NaN and Inf in Xv[b, f] reach row b's
 * logit through Xv * P (and through the second order, as before) and no other row's.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.
 */
#ifndef DFWFM_FOLD_H
#define DFWFM_FOLD_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_FOLD_ABI_VERSION 1

int dfwfm_fold_abi_version(void);

/* enable != 0: build the folded layer-1 pack from the dense parameters currently set (the caller's
 * net_1_linear_1.weight of the last dfwfm_model_set_dense) and row 0 of the numerical fields' second-order tables of
 * the last dfwfm_model_set_tables, both read on `stream`; from then on dfwfm_forward / dfwfm_forward_batches run
 * layer 1 folded.  One launch, stream-ordered, no allocation and no host synchronisation (the pack's memory is the
 * model's from dfwfm_model_create), so the build can be captured into a HIP graph.  enable == 0: the forward is
 * unfolded again.  dfwfm_model_set_dense and dfwfm_model_set_tables turn the fold off until the next call.
 * *enabled = 1 when the fold is on after the call.  *enabled = 0, DFWFM_OK and an unfolded forward when enable == 0,
 * when the model has no deep tower or no numerical field, when the folded activation tile of some fused inference form
 * of this model does not fit (LDS, or a second workgroup per CU lost), or under DFWFM_DIAG fold=0 (A/B and tests).
 * The static 25-chunk forms run a folded layer 1 of 18 chunks; a model of that form whose folded layer 1 is longer
 * keeps 25 chunks over a zero-padded pack.  A failed call leaves the model unchanged.
 * DFWFM_ERR_INVALID_ARG: a null pointer; DFWFM_ERR_STATE: tables or dense parameters not yet set. */
int dfwfm_model_fold_numerical(dfwfm_model* m, int32_t enable, int32_t* enabled, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_FOLD_H */
