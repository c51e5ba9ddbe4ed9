/*
 * dfwfm_lazy_optim.h -- C ABI of the row-lazy SGD, Adagrad and RMSprop steps for embedding tables (libdfwfm.so, beside
 * include/dfwfm_optim.h and include/dfwfm_lazy_adam.h).
 *
 * dfwfm_optim_step_dev (include/dfwfm_optim.h) is torch.optim.SGD / Adagrad / RMSprop over nn.Embedding(sparse=False):
 * every row of every table, and of its state array, is read and written every step, although a batch touches a few
 * thousand of them.  This header adds for those three optimizers what include/dfwfm_lazy_adam.h adds for Adam: only the
 * rows a batch touched are updated -- the row-wise sparse update people who train large embedding tables run (sparse
 * Adagrad, torch.optim.SGD over nn.Embedding(sparse=True)).  Opt-in: nothing in include/dfwfm.h,
 * include/dfwfm_optim.h or include/dfwfm_lazy_adam.h changes, and nothing calls this unless asked to.
 *
 * The contract.
 *
 * Touched rows: exactly as in include/dfwfm_lazy_adam.h.  For each listed table, a row is *touched* by a call when at
 * least one sample i < batch of the call maps to it:
 *   - key = xi[i * xi_stride + column];
 *   - a key outside [0, key_range) counts as key 0 -- the clamp the forwards and the backward's scatter apply (they
 *     also raise the sticky index flag; this call does not);
 *   - the row is `key` for a plain (nn.Embedding / nn.EmbeddingBag) table, `key / c` for a QR quotient table and
 *     `key % c` for a QR remainder table.
 *
 * The update.  For every element of a touched row the call does exactly what dfwfm_optim_step_dev does for that
 * element given the same (p, g, state), the same hyper-parameters and the same step number -- the same bits:
 *   - the arithmetic is the dense kernels' per-element function (optim_elem, csrc/dfwfm_optim.h), compiled with
 *     contraction off as there, so the result has the same 32 bits as dfwfm_optim_elem_ref (include/dfwfm_optim.h: the
 *     forms, every rounding written out) at the step below;
 *   - the step is the state block's step counter + 1: the GLOBAL step of the state block, not a per-row count of how
 *     often the row was touched.  The step number matters to the arithmetic only for momentum-SGD's "copy the gradient
 *     at step 1": that branch is taken at global step 1 and at no other, so a row first touched at step 3 gets
 *     buf = round(0 * momentum) + g' from its zero-filled buffer (the same value as a copy, but for the sign of a -0
 *     gradient), and a row touched at steps 1 and 3 gets nothing at step 2;
 *   - coupled L2 applies, g' = fmaf(wd, p, g): weight decay acts on touched rows only;
 *   - a touched row whose summed gradient is exactly zero is still updated: weight decay acts, a momentum buffer or
 *     square_avg decays, the buffer moves the row;
 *   - after the update the row's gradient is set to 0 (a zeroed gradient row: a table's gradient buffer that was all
 *     zero before the backward scattered into it is all zero again after the call, with no fill).
 *
 * `state` is the kind's one state array -- momentum buffer, `sum` or `square_avg` --, zero-filled once by the caller.
 * SGD with momentum == 0 carries none: `state` may be NULL and is then never touched (no address is formed from it).
 *
 * Versus the dense update (dfwfm_optim_step_dev over the whole table, after a backward that left untouched rows'
 * gradients exactly zero):
 *   - plain SGD (momentum == 0) with weight_decay == 0 coincides bit for bit: the dense step gives an untouched row
 *     p = fmaf(0, -lr, p), which is p;
 *   - Adagrad with weight_decay == 0 and eps > 0 coincides bit for bit: the dense step gives an untouched row
 *     sum = fmaf(0, 0, sum) and p = p + (-0 / std), which leave the bits alone (with eps == 0 a never-touched row
 *     would be 0 / 0 in the dense step);
 *   - momentum-SGD, RMSprop and any weight_decay != 0 do NOT coincide -- that is ANOTHER optimizer, as lazy Adam is:
 *     an untouched row's momentum buffer or square_avg does not decay, a momentum-SGD row is not moved by its buffer
 *     while it is untouched, and an untouched row gets no L2 that step.  From zero-filled state they still coincide
 *     for one step when weight_decay == 0.
 *
 * The rest, as in include/dfwfm_lazy_adam.h.
 *   - A row touched by several samples is updated once.
 *   - Untouched rows keep the bits of param and state; their grad is neither read nor written.
 *   - The call advances the state block's step counter once, the way dfwfm_optim_step_dev does: every workgroup takes
 *     step = counter + 1, and the last workgroup to finish in the call's last launch advances it (the ticket scheme of
 *     include/dfwfm_optim.h; the ticket is 0 again afterwards).
 *   - The call is stream-ordered: launches only, no host synchronisation, no allocation (not on the first call
 *     either: the table list travels as kernel arguments, up to 60 tables per launch; a longer list takes several
 *     launches), so it can be captured into a HIP graph; a replay reads xi, the gradients, the counter and the
 *     schedule afresh.
 *   - Rows are independent, so the result does not depend on which thread claims a row: given equal gradients the
 *     result is bit-identical from run to run.
 *
 * Stamps: the scheme of include/dfwfm_lazy_adam.h.  A row is claimed by one atomic exchange on stamp[row] with this
 * step's stamp; whoever reads back another value owns the row.  The step's stamp is (step - 1) mod (2^32 - 1) + 1,
 * never 0, so stamps start at zero together with the state block (both zero-filled by the caller).  After 2^32 - 1
 * steps the stamps repeat: a row last touched exactly 2^32 - 1 steps earlier, and not since, would be skipped once.  A
 * table listed twice in one call (two columns sharing it) must share its stamp array; its rows are then updated once
 * for the union of the columns' keys.  Two tables must not share a stamp array otherwise.
 *
 * batch == 0 or n == 0: DFWFM_OK and no row is updated, but the step counter STILL advances (one empty workgroup), as
 * dfwfm_optim_step_dev does over an empty list.
 *
 * dfwfm_lazy_optim_step_dev_sched reads the rate from a schedule block (include/dfwfm_lr_schedule.h), evaluated by
 * every workgroup at counter + 1, as dfwfm_optim_step_dev_sched does; hyper->lr is then unused (and not checked).  At
 * step s its result equals, bit for bit, the unscheduled call's with lr = dfwfm_lr_schedule_eval(s).
 *
 * Errors: DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for
 *   - the hyper-parameters, as dfwfm_optim_step_dev checks them: a null hyper, an unknown kind, a hyper-parameter (lr,
 *     weight_decay, momentum, alpha, eps) that is NaN, infinite or negative, alpha outside [0, 1);
 *   - a null state block or schedule block, n < 0, batch < 0, a null table array with n > 0, a null xi or
 *     xi_stride < 1 with batch > 0 and n > 0;
 *   - per table, as dfwfm_lazy_adam_step_dev checks them: a null param, grad or stamp, rows < 1, width < 1,
 *     key_range < 1, column < 0 or >= xi_stride (batch > 0), a bad kind, c < 1 on a QR kind, or a key range that
 *     reaches past the table (plain: key_range > rows; quotient: (key_range - 1) / c >= rows; remainder:
 *     min(c, key_range) > rows); and a null state where the optimizer needs one (every kind but SGD with
 *     momentum == 0).
 * DFWFM_ERR_UNSUPPORTED: batch too large for a 32-bit grid.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_LAZY_OPTIM_H
#define DFWFM_LAZY_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"
#include "dfwfm_lazy_adam.h"
#include "dfwfm_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_LAZY_OPTIM_ABI_VERSION 1

/* One table of a lazy step: dfwfm_lazy_adam_table with one state array.  Device pointers; rows of `width` floats,
 * 4-byte aligned (no wider alignment assumed).  `kind` is DFWFM_LAZY_PLAIN / _QUOTIENT / _REMAINDER
 * (include/dfwfm_lazy_adam.h). */
typedef struct {
  float* param;        /* [rows, width]                                                        */
  float* grad;         /* [rows, width]; touched rows are read, then zeroed                     */
  float* state;        /* [rows, width]: momentum buffer / sum / square_avg; NULL for plain SGD */
  int32_t* stamp;      /* [rows], zero-filled once by the caller together with the state block */
  int64_t rows;        /* >= 1; every key of [0, key_range) must map to a row < rows           */
  int64_t key_range;   /* >= 1; keys outside [0, key_range) count as key 0                     */
  int64_t c;           /* QR collisions (>= 1) for the quotient / remainder kinds; else unused */
  int32_t width;       /* >= 1 floats per row                                                  */
  int32_t column;      /* >= 0: the table's column of xi                                       */
  int32_t kind;        /* DFWFM_LAZY_PLAIN / _QUOTIENT / _REMAINDER                            */
  int32_t reserved;
} dfwfm_lazy_optim_table;

int dfwfm_lazy_optim_abi_version(void);

/* The lazy step over `n` tables (a host array, read during the call) for the keys xi [batch, xi_stride] (device,
 * int64), with the dense call's hyper-parameters (include/dfwfm_optim.h) and state block (DFWFM_ADAM_STATE_BYTES of
 * device memory, zero-filled once).  Needs no model. */
int dfwfm_lazy_optim_step_dev(const dfwfm_lazy_optim_table* tables, int32_t n, const int64_t* xi, int64_t xi_stride,
                              int64_t batch, const dfwfm_optim_hyper* hyper, void* state_dev, void* stream);

/* dfwfm_lazy_optim_step_dev with the rate read from sched_dev (DFWFM_LR_SCHEDULE_BYTES, written by
 * dfwfm_lr_schedule_write) when the kernels run. */
int dfwfm_lazy_optim_step_dev_sched(const dfwfm_lazy_optim_table* tables, int32_t n, const int64_t* xi,
                                    int64_t xi_stride, int64_t batch, const dfwfm_optim_hyper* hyper,
                                    const void* sched_dev, void* state_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_LAZY_OPTIM_H */
