/*
 * dfwfm_lazy_adam.h -- C ABI of the row-lazy Adam step for embedding tables (libdfwfm.so, beside include/dfwfm.h).
 *
 * dfwfm_adam_step_dev (include/dfwfm.h) is torch.optim.Adam over nn.Embedding(sparse=False): every row of every table
 * is read and written every step, although a batch touches a few thousand of them.  This header adds the update people
 * who train large embedding tables expect instead -- torch.optim.SparseAdam over nn.Embedding(sparse=True),
 * TensorFlow's LazyAdam: only the rows a batch touched are updated.  That is ANOTHER optimizer, not a faster form of
 * the dense one: an untouched row gets no moment decay and no L2 that step.  Opt-in: nothing in include/dfwfm.h
 * changes, and nothing calls this unless asked to.
 *
 * The contract.
 *
 * Touched rows.  For each listed table, a row is *touched* by a call when at least one sample i < batch of the call
 * maps to it:
 *   - key = xi[i * xi_stride + column];
 *   - a key outside [0, key_range) counts as key 0 -- the clamp the forwards and the backward's scatter apply (they
 *     also raise the sticky index flag; this call does not);
 *   - the row is `key` for a plain (nn.Embedding / nn.EmbeddingBag) table, `key / c` for a QR quotient table and
 *     `key % c` for a QR remainder table.
 *
 * The update.  For every element of a touched row the call does exactly what dfwfm_adam_step_dev does for that
 * element given the same (p, g, m, v), the same hyper-parameters and the same step number -- the same bits:
 *   - the arithmetic is the dense kernels' per-element function (adam_elem, csrc/dfwfm_adam.h), shared by all of
 *     them: every rounding written out, the second moment as v = fma(v, beta2, ((1 - beta2) g) g).  That is
 *     dfwfm_adam_step on every element, and dfwfm_adam_step_dev on every element it updates through 16-byte accesses
 *     (all of a 16-byte-aligned tensor but its last numel % 4 elements; those few keep the historical
 *     v = fma(g, (1 - beta2) g, v beta2), which is the same value whenever v was 0 and at most one rounding of v away
 *     otherwise);
 *   - the coefficients come from adam_coef(step) with step = the state block's step counter + 1: the GLOBAL step of
 *     the state block, not a per-row count of how often the row was touched (so a row touched at steps 1 and 3 gets
 *     step 3's bias corrections at step 3, and nothing at step 2);
 *   - coupled L2 applies, g = weight_decay * p + g: weight decay acts on touched rows only;
 *   - a touched row whose summed gradient is exactly zero is still updated: its moments decay and weight decay acts;
 *   - after the update the row's gradient is set to 0 (a zeroed gradient row: a table's gradient buffer that was all
 *     zero before the backward scattered into it is all zero again after the call, with no fill).
 *
 * The rest.
 *   - A row touched by several samples is updated once.
 *   - Untouched rows keep the bits of param, exp_avg and exp_avg_sq; their grad is not read (nor written).
 *   - The call advances the state block's step counter once, the way dfwfm_adam_step_dev does: the last workgroup to
 *     finish in the call's last launch advances it, after every workgroup of the call has read it.
 *   - The call is stream-ordered: launches only, no host synchronisation, no allocation (not on the first call
 *     either: the table list travels as kernel arguments, up to 54 tables per launch), so it can be captured into a
 *     HIP graph; a replay reads xi, the gradients and the counter afresh.
 *   - Rows are independent, so the result does not depend on which thread claims a row: given equal gradients the
 *     result is bit-identical from run to run.
 *
 * Stamps.  A row is claimed by one atomic exchange on stamp[row] with this step's stamp; whoever reads back another
 * value owns the row.  The step's stamp is (step - 1) mod (2^32 - 1) + 1, never 0, so stamps start at zero together
 * with the state block (both zero-filled by the caller) and no step's stamp equals a never-touched row's.  After
 * 2^32 - 1 steps the stamps repeat: a row last touched exactly 2^32 - 1 steps earlier, and not since, would be
 * skipped once.  A table listed twice in one call (two columns sharing it) must share its stamp array; its rows are
 * then updated once for the union of the columns' keys.  Two tables must not share a stamp array otherwise.
 *
 * batch == 0 or n == 0: DFWFM_OK and no row is updated, but the step counter STILL advances (one empty workgroup), as
 * dfwfm_adam_step_dev does over an empty list: a trainer that keeps this state block in step with another one's
 * does not have to special-case an empty batch.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_LAZY_ADAM_H
#define DFWFM_LAZY_ADAM_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_LAZY_ADAM_ABI_VERSION 1

#define DFWFM_LAZY_PLAIN 0      /* row = key                         */
#define DFWFM_LAZY_QUOTIENT 1   /* row = key / c  (QR weight_q)      */
#define DFWFM_LAZY_REMAINDER 2  /* row = key % c  (QR weight_r)      */

/* One table of a lazy step.  Device pointers; rows of `width` floats, 4-byte aligned (no wider alignment assumed). */
typedef struct {
  float* param;        /* [rows, width]                                                        */
  float* grad;         /* [rows, width]; touched rows are read, then zeroed                     */
  float* exp_avg;      /* [rows, width]                                                        */
  float* exp_avg_sq;   /* [rows, width]                                                        */
  int32_t* stamp;      /* [rows], zero-filled once by the caller together with the state block */
  int64_t rows;        /* >= 1; every key of [0, key_range) must map to a row < rows           */
  int64_t key_range;   /* >= 1; keys outside [0, key_range) count as key 0                     */
  int64_t c;           /* QR collisions (>= 1) for the quotient / remainder kinds; else unused */
  int32_t width;       /* >= 1 floats per row                                                  */
  int32_t column;      /* >= 0: the table's column of xi                                       */
  int32_t kind;        /* DFWFM_LAZY_PLAIN / _QUOTIENT / _REMAINDER                            */
  int32_t reserved;
} dfwfm_lazy_adam_table;

int dfwfm_lazy_adam_abi_version(void);

/* The lazy step over `n` tables (a host array, read during the call) for the keys xi [batch, xi_stride] (device,
 * int64), with the dense call's hyper-parameters and state block (DFWFM_ADAM_STATE_BYTES of device memory, zero-filled
 * once).  Needs no model.
 * DFWFM_ERR_INVALID_ARG (and no launch): a null state block, n < 0, batch < 0, a null table array with n > 0, a null xi
 * or xi_stride < 1 with batch > 0; per table a null pointer, rows < 1, width < 1, key_range < 1, column < 0 or
 * >= xi_stride (batch > 0), a bad kind, c < 1 on a QR kind, or a key range that reaches past the table (plain:
 * key_range > rows; quotient: (key_range - 1) / c >= rows; remainder: min(c, key_range) > rows).
 * DFWFM_ERR_UNSUPPORTED: batch too large for a 32-bit grid. */
int dfwfm_lazy_adam_step_dev(const dfwfm_lazy_adam_table* tables, int32_t n, const int64_t* xi, int64_t xi_stride,
                             int64_t batch, double lr, double beta1, double beta2, double eps, double weight_decay,
                             void* state_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_LAZY_ADAM_H */
