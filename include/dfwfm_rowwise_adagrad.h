/*
 * dfwfm_rowwise_adagrad.h -- C ABI of the row-wise Adagrad step for embedding tables (libdfwfm.so, beside
 * include/dfwfm_lazy_optim.h).
 *
 * Every other table optimizer of this library keeps one state float per table ELEMENT.  Row-wise Adagrad -- the update
 * large embedding tables are normally trained with (FBGEMM / TorchRec EXACT_ROWWISE_ADAGRAD, DLRM) -- keeps ONE
 * accumulator per table ROW, fed with the mean of the row's squared gradient: at a row width of 10 floats the state of
 * a table is 4 bytes per row instead of 40.  Only the rows a batch touched are updated, as in
 * include/dfwfm_lazy_optim.h.  Opt-in: no other header changes, and nothing calls this unless asked to.
 *
 * The contract.  (The rules on touched rows, the claim, the stamps, the step counter and graph capture are those of
 * include/dfwfm_lazy_optim.h; they are restated here in full, and this header is the one that binds these calls.)
 *
 * Touched rows.  For each listed table, a row is *touched* by a call when at least one sample i < batch of the call
 * maps to it:
 *   - key = xi[i * xi_stride + column];
 *   - a key outside [0, key_range) counts as key 0 -- the clamp the forwards and the backward's scatter apply (they
 *     also raise the sticky index flag; this call does not);
 *   - the row is `key` for a plain (nn.Embedding / nn.EmbeddingBag) table, `key / c` for a QR quotient table and
 *     `key % c` for a QR remainder table.
 *
 * The update of a touched row, with p[width] its parameters, g[width] its gradient and acc its one accumulator.  All
 * of it is f32.  fmaf is ONE fused multiply-add; nothing else is fused (the code is compiled with contraction off).
 * The scalars wd = (float)weight_decay, -lr = (float)(-lr) and eps = (float)eps are formed in double and rounded once.
 *
 *     g'_e = fmaf(wd, p_e, g_e) when wd != 0, else g_e              e = 0 .. width-1
 *     ss   = 0;  for e = 0 .. width-1 in this order:  ss = fmaf(g'_e, g'_e, ss)
 *     acc  = acc + round(ss / (float)width)          (one correctly rounded division, one rounded sum)
 *     std  = sqrt(acc) + eps                         (the correctly rounded square root, one rounded sum)
 *     p_e  = p_e + round(round(-lr * g'_e) / std)    (the element-wise Adagrad's last line)
 *
 *   - The summation order IS the contract: the sequential chain in element order -- not a tree, not a per-lane
 *     partial sum.  It is what lets dfwfm_rowwise_adagrad_row_ref and every path of the kernel return the same 32
 *     bits (a pairwise tree gives another ss on some rows: the order is observable).
 *   - The step number does not enter the arithmetic (it enters only through a schedule, below).
 *   - Coupled L2 applies through g': weight decay acts on touched rows only.
 *   - A touched row whose summed gradient is exactly zero is still updated (weight decay acts on it).
 *   - eps == 0 is accepted.  A touched row with a zero gradient and a zero accumulator is then 0 / 0 (NaN), as in
 *     torch's Adagrad with eps == 0.
 *   - After the update the row's gradient is set to 0 (a zeroed gradient row: a table's gradient buffer that was all
 *     zero before the backward scattered into it is all zero again after the call, with no fill).
 *
 * `state` is [rows]: one float per row, zero-filled once by the caller, never NULL.
 *
 * The rest.
 *   - A row touched by several samples is updated once.
 *   - Untouched rows keep the bits of param and state; their grad is neither read nor written.
 *   - The call advances the state block's step counter once: every workgroup takes step = counter + 1, and the last
 *     workgroup to finish in the call's last launch advances it (a ticket in the state block, 0 again afterwards).  The
 *     state block is the one of include/dfwfm_optim.h (DFWFM_ADAM_STATE_BYTES of device memory, zero-filled once).
 *   - The call is stream-ordered: launches only, no host synchronisation, no allocation (not on the first call
 *     either: the table list travels as kernel arguments, up to 60 tables per launch; a longer list takes several
 *     launches with one counter advance), so it can be captured into a HIP graph; a replay reads xi, the gradients,
 *     the counter and the schedule afresh.
 *   - Rows are independent and a row's chain has one order, so the result does not depend on which thread claims a
 *     row: given equal gradients the result is bit-identical from run to run.
 *
 * Stamps.  A row is claimed by one atomic exchange on stamp[row] with this step's stamp; whoever reads back another
 * value owns the row.  The step's stamp is (step - 1) mod (2^32 - 1) + 1, never 0, so stamps start at zero together
 * with the state block (both zero-filled by the caller).  After 2^32 - 1 steps the stamps repeat: a row last touched
 * exactly 2^32 - 1 steps earlier, and not since, would be skipped once.  A table listed twice in one call (two columns
 * sharing it) must share its stamp array; its rows are then updated once for the union of the columns' keys.  Two
 * tables must not share a stamp array otherwise.
 *
 * batch == 0 or n == 0: DFWFM_OK and no row is updated, but the step counter STILL advances (one empty workgroup).
 *
 * dfwfm_rowwise_adagrad_step_dev_sched reads the rate from a schedule block (include/dfwfm_lr_schedule.h), evaluated
 * by every workgroup at counter + 1; hyper->lr is then unused (and not checked).  At step s its result equals, bit for
 * bit, the unscheduled call's with lr = dfwfm_lr_schedule_eval(s).
 *
 * Relation to the other optimizers.
 *   - This is NOT torch.optim.Adagrad, and not dfwfm_lazy_optim_step_dev with DFWFM_OPTIM_ADAGRAD: every element of a
 *     row is divided by the same std, that of the row's mean squared gradient.
 *   - Weight decay acts on touched rows only.
 *   - There is no dense form.  (With weight_decay == 0 and eps > 0 a dense sweep would leave an untouched row's bits
 *     alone anyway: its acc would gain 0 and its parameters -0 / std.)
 *   - The element-wise Adagrad coincides in one corner: weight_decay == 0, a width that is a power of two up to 16,
 *     and every gradient of the row equal to +-2^k for one k.  There ss / width is exactly 2^(2k), and acc + 2^(2k)
 *     rounded once is fmaf(g, g, acc): with its `sum` row equal to acc in every element, the element-wise step gives
 *     the same parameters, and a `sum` row that is the new acc in every element.
 *
 * Errors: DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for
 *   - the hyper-parameters: a null hyper, a kind other than DFWFM_OPTIM_ADAGRAD, a hyper-parameter (lr, weight_decay,
 *     momentum, alpha, eps) that is NaN, infinite or negative, alpha outside [0, 1) (momentum and alpha are checked as
 *     dfwfm_optim_step_dev checks them, and are not read otherwise);
 *   - a null state block or schedule block, n < 0, batch < 0, a null table array with n > 0, a null xi or
 *     xi_stride < 1 with batch > 0 and n > 0;
 *   - per table: a null param, grad, state or stamp, rows < 1, width < 1, key_range < 1, column < 0 or >= xi_stride
 *     (batch > 0), a bad kind, c < 1 on a QR kind, or a key range that reaches past the table (plain:
 *     key_range > rows; quotient: (key_range - 1) / c >= rows; remainder: min(c, key_range) > rows).
 * DFWFM_ERR_UNSUPPORTED: batch too large for a 32-bit grid.
 * dfwfm_rowwise_adagrad_row_ref: DFWFM_ERR_INVALID_ARG for the hyper-parameters as above, a null pointer, width < 1.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_ROWWISE_ADAGRAD_H
#define DFWFM_ROWWISE_ADAGRAD_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"
#include "dfwfm_lazy_adam.h"
#include "dfwfm_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_ROWWISE_ADAGRAD_ABI_VERSION 1

/* One table of a row-wise step: the layout of dfwfm_lazy_optim_table (include/dfwfm_lazy_optim.h) with one
 * difference, `state` is [rows].  Device pointers; rows of `width` floats, 4-byte aligned (no wider alignment
 * assumed).  `kind` is DFWFM_LAZY_PLAIN / _QUOTIENT / _REMAINDER (include/dfwfm_lazy_adam.h). */
typedef struct {
  float* param;        /* [rows, width]                                                        */
  float* grad;         /* [rows, width]; touched rows are read, then zeroed                     */
  float* state;        /* [rows]: the row's accumulator; zero-filled once by the caller; never NULL */
  int32_t* stamp;      /* [rows], zero-filled once by the caller together with the state block */
  int64_t rows;        /* >= 1; every key of [0, key_range) must map to a row < rows           */
  int64_t key_range;   /* >= 1; keys outside [0, key_range) count as key 0                     */
  int64_t c;           /* QR collisions (>= 1) for the quotient / remainder kinds; else unused */
  int32_t width;       /* >= 1 floats per row (any width)                                      */
  int32_t column;      /* >= 0: the table's column of xi                                       */
  int32_t kind;        /* DFWFM_LAZY_PLAIN / _QUOTIENT / _REMAINDER                            */
  int32_t reserved;
} dfwfm_rowwise_table;

int dfwfm_rowwise_adagrad_abi_version(void);

/* The row-wise Adagrad step over `n` tables (a host array, read during the call) for the keys xi [batch, xi_stride]
 * (device, int64).  Of the hyper-parameters lr, weight_decay and eps are read; kind must be DFWFM_OPTIM_ADAGRAD.
 * Needs no model. */
int dfwfm_rowwise_adagrad_step_dev(const dfwfm_rowwise_table* tables, int32_t n, const int64_t* xi, int64_t xi_stride,
                                   int64_t batch, const dfwfm_optim_hyper* hyper, void* state_dev, void* stream);

/* dfwfm_rowwise_adagrad_step_dev with the rate read from sched_dev (DFWFM_LR_SCHEDULE_BYTES, written by
 * dfwfm_lr_schedule_write) when the kernels run. */
int dfwfm_rowwise_adagrad_step_dev_sched(const dfwfm_rowwise_table* tables, int32_t n, const int64_t* xi,
                                         int64_t xi_stride, int64_t batch, const dfwfm_optim_hyper* hyper,
                                         const void* sched_dev, void* state_dev, void* stream);

/* Host only: one row by exactly the kernel's arithmetic.  p[width] and *acc are read and written, g[width] is only
 * read (the kernel's zeroing of the gradient row is not part of this function). */
int dfwfm_rowwise_adagrad_row_ref(const dfwfm_optim_hyper* hyper, int32_t width, float* p, const float* g, float* acc);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_ROWWISE_ADAGRAD_H */
