/*
 * dfwfm_half_tables.h -- C ABI of the fp16 serving copy of the categorical tables (libdfwfm.so, beside
 * include/dfwfm.h, whose dfwfm_model_pack_tables this mirrors).
 *
 * The inference forwards gather the categorical rows from a model-owned serving copy of the tables when one is in
 * use.  dfwfm_model_pack_tables builds it in f32 (one aligned 64-byte row per table row at embedding_size 10);
 * dfwfm_model_pack_tables_half builds it with the second-order row in IEEE fp16: half the bytes, and two 16-byte
 * loads per row instead of three.
 *
 * Opt-in: nothing in the other headers changes or routes here.
 *
 * The numeric contract.  Every categorical second-order value is rounded to fp16 once, when the copy is built:
 * round to nearest, ties to even, subnormals kept.  The row's first-order weight stays f32.  A forward converts the
 * halves back to f32, which is exact, and runs the arithmetic of the same call on the f32 copy: the same combine,
 * first order, FwFM / FM and deep tower.  So with the fp16 copy in use a model's logits are, bit for bit, the logits
 * of the same call on a model whose categorical second-order tables were replaced by float(half(w)), everything else
 * untouched.  The numerical fields are not in the copy: their tables, and the folded layer 1 formed from them
 * (dfwfm_fold.h, dfwfm_bf16_fold.h), stay f32.
 *
 * A value that would round to +-inf (|x| >= 65520) is not served: the pack counts such values, and when there are
 * any it fails and leaves the model on the plain tables.
 *
 * Row layout: [embedding_size x fp16][pad to 4 bytes][f32 first-order weight][zero pad].  The stride is 32 bytes
 * while 2 * embedding_size + 4 <= 32 (embedding_size 10, 8 and 4: two rows per 64-byte line), else the next multiple
 * of 16 bytes (embedding_size 16: 48, 32: 80).  The copy lives in the allocation of the f32 copy: a model holds one
 * of the two at a time.
 *
 * Which calls read it: the ones that read the f32 copy -- dfwfm_forward and dfwfm_forward_batches (with and without
 * a deep tower, folded or not), dfwfm_forward_gather, dfwfm_bf16_fused_forward[_batches] and
 * dfwfm_int8_forward[_batches].  dfwfm_train_forward never reads a serving copy, and the gather launch of the sparse
 * deep tower (dfwfm_forward_ws) reads the plain tables.
 *
 * Synchronisation.  Both pack calls synchronise `stream` once (dfwfm.h's description of dfwfm_model_pack_tables says
 * "no sync", which holds for the forward calls only: the pack stages the per-field row bases from the host and waits
 * for that copy).  dfwfm_model_pack_tables_half waits once as well, after its launch, and reads the overflow count in
 * that same wait: once per weight update, nothing added to a forward.
 *
 * Errors: DFWFM_ERR_INVALID_ARG for a null pointer; DFWFM_ERR_STATE before dfwfm_model_set_tables;
 * DFWFM_ERR_UNSUPPORTED when a value overflows fp16.  No call aborts.  Status codes and dfwfm_last_error as in
 * dfwfm.h.
 */
#ifndef DFWFM_HALF_TABLES_H
#define DFWFM_HALF_TABLES_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_HALF_TABLES_ABI_VERSION 1

int dfwfm_half_tables_abi_version(void);

/* (re)build the serving copy with fp16 second-order rows from the tables of the last dfwfm_model_set_tables (read on
 * `stream`), or drop any serving copy (enable = 0).  Eligibility is that of dfwfm_model_pack_tables: a second order,
 * first-order tables, no QR field, at least one categorical field; an ineligible model gets *enabled = 0 and
 * DFWFM_OK and stays on the plain tables.  *overflow_count (may be null) receives the number of values that round to
 * +-inf; when it is not 0 the call returns DFWFM_ERR_UNSUPPORTED with a message naming the count, *enabled = 0, and
 * the model is left on the plain tables, usable.  One launch and one synchronisation of `stream`; the first call (or
 * larger tables) allocates.  dfwfm_model_set_tables and dfwfm_model_pack_tables drop this copy as they drop the f32
 * one. */
int dfwfm_model_pack_tables_half(dfwfm_model* m, int32_t enable, int32_t* enabled, int64_t* overflow_count,
                                 void* stream);

/* *bytes = the size of the serving copy in use (rows x row stride: f32, fp16, or the int8 one of
 * dfwfm_int8_tables.h), or 0 when the model reads the plain tables; host-only, no launch. */
int dfwfm_model_serving_copy_bytes(dfwfm_model* m, int64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_HALF_TABLES_H */
