/*
 * dfwfm_int8_tables.h -- C ABI of the int8 serving copy of the categorical tables (libdfwfm.so, beside
 * include/dfwfm.h and include/dfwfm_half_tables.h, whose pack calls this mirrors).
 *
 * The inference forwards gather the categorical rows from a model-owned serving copy of the tables when one is in
 * use.  dfwfm_model_pack_tables builds it in f32 (64 bytes per row at embedding_size 10),
 * dfwfm_model_pack_tables_half with the second-order row in fp16 (32 bytes), and dfwfm_model_pack_tables_int8 with
 * the second-order row as row-wise symmetric int8 under one bf16 scale: 16 bytes per row at embedding_size 10, a
 * quarter of the f32 copy, and one 16-byte load per row instead of three.
 *
 * Opt-in: nothing in the other headers changes or routes here.
 *
 * The numeric contract.  Every categorical second-order row w[0..D) is quantized once, when the copy is built, in
 * IEEE f32 throughout:
 *   amax = max_d |w[d]|,  t = amax / 127;
 *   the scale s is t rounded up to bf16: bits(s) = (bits(t) + 0xFFFF) & 0xFFFF0000;
 *   when t < 2^-126 (zero, or not a normal f32) s = 0 and the row serves zeros -- so the result does not depend on how
 *   a device treats f32 subnormals;
 *   q[d] = clamp(rint(w[d] / s), -127, 127): a correctly rounded division, rint to nearest even, q = 0 when s = 0;
 *   -128 is never produced.
 * The served value is float(q[d]) * s.  That product is exact in f32 (7 bits x 8 bits), so any decode order gives the
 * same bits.  The row's first-order weight stays f32.  A forward then runs the arithmetic of the same call on the f32
 * copy: the same combine, first order, FwFM / FM and deep tower.  So with the int8 copy in use a model's logits are,
 * bit for bit, the logits of the same call on a model whose categorical second-order tables were replaced by the
 * dequantized values, everything else untouched.  The numerical fields are not in the copy: their tables, and the
 * folded layer 1 formed from them (dfwfm_fold.h, dfwfm_bf16_fold.h), stay f32.
 *
 * A value that is NaN, +-inf or of magnitude >= 2^127 is not served (the bound keeps 127 s finite after the scale's
 * round-up): the pack counts such values, and when there are any it fails and leaves the model on the plain tables.
 *
 * Row layout: [embedding_size bytes][pad to 2 bytes][bf16 scale][pad to 4 bytes][f32 first-order weight][zero pad].
 * A byte holds q in two's complement (-127 .. 127; not q + 128): a gather decodes an element with one
 * sign-extending byte-to-float conversion and a multiply by s, the contract's product itself, one instruction per row
 * fewer than the offset form's conversion and fma.  The bf16 scale is the upper half of the f32 s, little endian like
 * the rest.  The stride is 16 bytes while the row fits (embedding_size 4, 8 and 10: four rows per 64-byte line), else
 * the next multiple of 16 bytes (embedding_size 16: 32, 32: 48).  The copy lives in the allocation of the f32 and fp16
 * copies: a model holds one of the three at a time.
 *
 * Which calls read it: the ones that read the f32 copy -- dfwfm_forward and dfwfm_forward_batches (with and without
 * a deep tower, folded or not), dfwfm_forward_gather, dfwfm_bf16_fused_forward[_batches] and
 * dfwfm_int8_forward[_batches].  dfwfm_train_forward never reads a serving copy.  The gather launch of the sparse
 * deep tower (dfwfm_forward_ws) reads the plain tables, so it returns DFWFM_ERR_UNSUPPORTED while this copy is in use.
 *
 * Synchronisation.  dfwfm_model_pack_tables_int8 issues one launch and synchronises `stream` once, after it: the
 * per-field row bases are staged from the host, and the unservable count is read in that same wait.  Once per weight
 * update, nothing added to a forward.
 *
 * Errors: DFWFM_ERR_INVALID_ARG for a null pointer; DFWFM_ERR_STATE before dfwfm_model_set_tables;
 * DFWFM_ERR_UNSUPPORTED when a value cannot be served.  No call aborts.  Status codes and dfwfm_last_error as in
 * dfwfm.h.
 */
#ifndef DFWFM_INT8_TABLES_H
#define DFWFM_INT8_TABLES_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_INT8_TABLES_ABI_VERSION 1

int dfwfm_int8_tables_abi_version(void);

/* (re)build the serving copy with int8 second-order rows from the tables of the last dfwfm_model_set_tables (read on
 * `stream`), or drop any serving copy (enable = 0).  Eligibility is that of dfwfm_model_pack_tables: a second order,
 * first-order tables, no QR field, at least one categorical field; an ineligible model gets *enabled = 0 and
 * DFWFM_OK and stays on the plain tables.  *unservable_count (may be null) receives the number of values that are
 * NaN, +-inf or of magnitude >= 2^127; when it is not 0 the call returns DFWFM_ERR_UNSUPPORTED with a message naming
 * the count, *enabled = 0, and the model is left on the plain tables, usable.  One launch and one synchronisation of
 * `stream`; the first call (or larger tables) allocates.  dfwfm_model_set_tables, dfwfm_model_pack_tables and
 * dfwfm_model_pack_tables_half drop this copy, and this call drops theirs.  dfwfm_model_serving_copy_bytes
 * (dfwfm_half_tables.h) reports this copy's size while it is in use. */
int dfwfm_model_pack_tables_int8(dfwfm_model* m, int32_t enable, int32_t* enabled, int64_t* unservable_count,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_INT8_TABLES_H */
