/*
 * dfwfm_bf16_fold.h -- C ABI of the folded layer 1 of the one-launch bf16 forward (libdfwfm.so, beside
 * include/dfwfm_bf16_fused.h, whose calls it changes, and include/dfwfm_fold.h, the same fold of the f32 forward).
 *
 * The embedding of a numerical field is E[b, f, :] = Xv[b, f] * v_f[0], a per-sample scalar times a constant row, so
 * layer 1 of the deep tower receives from it, at neuron n, Xv[b, f] * P[f][n] with P = W1 v_f[0] fixed by the weights.
 * With the fold on, layer 1 of dfwfm_bf16_fused_forward and dfwfm_bf16_fused_forward_batches contracts over
 * (F - num) D + num columns instead of F D: 9 K steps of 32 instead of 13 at Criteo-39 (39 fields, 13 numerical,
 * D = 10), 4 of the 39 steps of the 3 x 400 tower.
 *
 * Opt-in: nothing in the other headers changes.  Only the two calls of include/dfwfm_bf16_fused.h read the folded
 * pack; dfwfm_bf16_forward (the per-layer path) keeps reading the unfolded layer 1, which stays in place, so with the
 * fold on the fused calls no longer give the per-layer path's bits.
 *
 * The numeric contract.  With the fold on, layer 1 is
 *     z_1[b, n] = sum_k x[b, k] * Wf[n, k]
 * accumulated in f32 on v_mfma_f32_16x16x32_bf16, K steps of 32 ascending into one accumulator, over the folded K
 * rows in this order:
 *   1. k < (F - num) D: x = bf16(E[b, f, d]) for the categorical fields in field order (f >= num), Wf = the same
 *      columns of bf16(W1): the very bits of the pack of dfwfm_model_pack_bf16;
 *   2. the next num rows: x = bf16(Xv[b, f]), Wf = bf16(P[f][n]), f = 0..num-1, with
 *          P[f][n] = sum_d W1[n, f D + d] * v_f[0][d]
 *      from the f32 parameters, accumulated in f64 over d ascending (each product of two f32 values is exact in f64),
 *      rounded to f32, then to bf16 (both round to nearest even);
 *   3. zeros up to the step count ceil(((F - num) D + num) / 32), x and Wf both exactly 0.
 * Everything else is the contract of include/dfwfm_bf16.h: the epilogue (bias, ReLU, the rounding of the activation),
 * layers 2..H, the shares of deep, the combine, and first + second from the f32 gather expressions over all F fields.
 * Rows stay independent, and whether a model folds is decided per model, never per launch: a row's logit is the same
 * bits for any batch size, row position, batch set, row tile (16 / 32 / 64) and table form (plain, EmbeddingBag, QR,
 * the serving copy).  NaN and Inf in Xv[b, f] reach row b's logit and no other row's.
 * Against the unfolded contract this rounds Xv and P to bf16 in place of Xv * v_f[0] and W1: the same format, an
 * error of the same size (the tests bound both against the float64 oracle by the emulation's own error).
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.
 */
#ifndef DFWFM_BF16_FOLD_H
#define DFWFM_BF16_FOLD_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_BF16_FOLD_ABI_VERSION 1

int dfwfm_bf16_fold_abi_version(void);

/* enable != 0: build layer 1's folded bf16 fragments from net_1_linear_1.weight of the last dfwfm_model_set_dense and
 * row 0 of the numerical fields' second-order tables of the last dfwfm_model_set_tables, both read on `stream`; from
 * then on dfwfm_bf16_fused_forward / dfwfm_bf16_fused_forward_batches run layer 1 folded.  One launch, stream-ordered,
 * no host synchronisation; the first enabling call of a model allocates the pack, so the build is capturable into a
 * HIP graph after one eager call of the same model.  enable == 0: the forward is unfolded again.
 * dfwfm_model_set_dense, dfwfm_model_set_tables and dfwfm_model_pack_bf16 turn the fold off until the next call.
 * *enabled = 1 when the fold is on after the call.  *enabled = 0, DFWFM_OK and an unfolded forward when enable == 0,
 * when the model has no deep tower or no numerical field, when dfwfm_bf16_fused_supported refuses the model, when the
 * folded tile of a row-tile form does not fit the LDS or costs the 16- or 32-row form its second workgroup per CU,
 * or under DFWFM_DIAG bf16fold=0 (A/B and tests).  A failed call leaves the fold off.
 * DFWFM_ERR_INVALID_ARG: a null pointer; DFWFM_ERR_STATE (a model that could fold): tables or dense parameters not
 * yet set, or the bf16 copy absent or stale (dfwfm_model_pack_bf16). */
int dfwfm_model_fold_bf16(dfwfm_model* m, int32_t enable, int32_t* enabled, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_BF16_FOLD_H */
