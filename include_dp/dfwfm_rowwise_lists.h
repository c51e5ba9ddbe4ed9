/*
 * dfwfm_rowwise_lists.h -- C ABI of the row-wise Adagrad step driven by exchanged touched-row lists (libdfwfm.so,
 * beside include/dfwfm_lazy_lists.h and include/dfwfm_rowwise_adagrad.h, its two parents).
 *
 * dfwfm_rowwise_adagrad_step_dev finds the touched rows from the keys of the batch the process itself ran.  Under data
 * parallelism a rank sees only its slice of the global batch, while every replica has to update the rows the GLOBAL
 * batch touched: the union of every rank's touched-row list, which every rank already holds after the exchange and
 * which dfwfm_sparse_grads_apply (include/dfwfm.h) walks to add the rows' gradients.  dfwfm_lazy_optim_lists_step_dev
 * takes its rows from those lists, but walks flat buffers with ONE offset per span for gradient and state, and
 * row-wise state is one float per ROW: it has another shape than the gradient.  The calls of this header take the
 * touched rows from the lists and the accumulators from a state pointer per span.  Opt-in: no other header changes,
 * and nothing calls this unless asked to.
 *
 * The header lives in include_dp/, beside include/: it names the types and calls of two headers of include/, and the
 * tests that bind those two hold every other file of include/ free of their names.
 *
 * The contract.  (It has two sources and is restated here in full; this header is the one that binds these calls.)
 *
 * -- From include/dfwfm_lazy_lists.h, unchanged: which rows, and how the call runs.
 *
 * Spans.  A span is one table: its own `param` tensor [rows, width], its accumulators `state` [rows], its `stamp`
 * array [rows], and `offset`, the index in floats at which its rows start in the flat `grad` array.  The offset
 * indexes the gradient ONLY: parameters, accumulators and stamps are the span's own arrays.  Spans may come in any
 * order; their gradient ranges [offset, offset + rows * width) must not overlap.
 *
 * Lists.  A list is dfwfm_lazy_lists_list, what dfwfm_sparse_grads_local writes and dfwfm_sparse_grads_apply reads:
 * `dest` (device, int64), `count` (device, one int32) and the capacity `cap`, for rows of `width` floats.  dest[e] is
 * the offset in floats of a row's first element in the flat gradient buffer; destinations are unique within a list;
 * the reader stops at min(*count, cap) (a count below 0 reads nothing).
 *
 * Touched rows.  A row is *touched* by a call when at least one list names its destination: dest[e] ==
 * span.offset + row * span.width for a span of the list's width and a row < span.rows.  A dest that falls in no span
 * of the list's width, or between two rows of one, is skipped: it is not written, it is not an error, and no address
 * is formed from it.
 *
 *   - A row named by several lists (several ranks touched it) is updated once.
 *   - Untouched rows keep the bits of param and state; their grad is neither read nor written.
 *   - The call advances the state block's step counter exactly once: every workgroup takes step = counter + 1, and the
 *     last workgroup to finish in the call's last launch advances it (a ticket in the state block, 0 again
 *     afterwards).  The state block is the one of include/dfwfm_optim.h (DFWFM_ADAM_STATE_BYTES of device memory,
 *     zero-filled once).  With no span, no list or all counts zero no row is updated and the step counter STILL
 *     advances (one empty workgroup).
 *   - The call is stream-ordered: launches only, no host synchronisation, no allocation on the device (not on the first
 *     call either).  Spans and list descriptors travel as kernel arguments, up to DFWFM_ROWWISE_LISTS_SPANS_PER_LAUNCH
 *     (60) spans and DFWFM_ROWWISE_LISTS_LISTS_PER_LAUNCH (24) lists per launch -- a span carries one pointer more
 *     than a dfwfm_lazy_lists_span, so fewer fit the 4 KiB of a launch; longer arrays take several launches (one per
 *     pair of a 60-span piece and a 24-list piece) with one counter advance.  The call can be captured into a HIP
 *     graph; a replay reads the counts, the destinations, the gradients, the counter and the schedule afresh.
 *   - Rows are independent and a row's chain has one order, so the result does not depend on which thread claims a
 *     row: given equal gradients the result is bit-identical from run to run.
 *
 * Stamps: the scheme of include/dfwfm_lazy_adam.h.  A row is claimed by a device-scope look at stamp[row] and, unless
 * it already holds this step's stamp, one atomic exchange with it; whoever reads back another value owns the row.
 * The step's stamp is (step - 1) mod (2^32 - 1) + 1, never 0, so stamps start at zero together with the state block
 * (both zero-filled by the caller).  After 2^32 - 1 steps the stamps repeat.  Two spans must not share stamps.
 *
 * -- From include/dfwfm_rowwise_adagrad.h, unchanged: what happens to a touched row.
 *
 * With p[width] the row's parameters, g[width] its gradient (grad[dest ..]) and acc = state[row] its one accumulator.
 * All of it is f32.  fmaf is ONE fused multiply-add; nothing else is fused (the code is compiled with contraction
 * off).  The scalars wd = (float)weight_decay, -lr = (float)(-lr) and eps = (float)eps are formed in double and
 * rounded once.
 *
 *     g'_e = fmaf(wd, p_e, g_e) when wd != 0, else g_e              e = 0 .. width-1
 *     ss   = 0;  for e = 0 .. width-1 in this order:  ss = fmaf(g'_e, g'_e, ss)
 *     acc  = acc + round(ss / (float)width)          (one correctly rounded division, one rounded sum)
 *     std  = sqrt(acc) + eps                         (the correctly rounded square root, one rounded sum)
 *     p_e  = p_e + round(round(-lr * g'_e) / std)    (the element-wise Adagrad's last line)
 *
 *   - These are the bits of dfwfm_rowwise_adagrad_row_ref, and of dfwfm_rowwise_adagrad_step_dev on keys that touch
 *     the same rows: the kernels call one copy of the row's arithmetic.
 *   - The summation order IS the contract: the sequential chain in element order -- not a tree, not a per-lane
 *     partial sum.
 *   - The step number does not enter the arithmetic (it enters only through a schedule, below); it is the GLOBAL step,
 *     the state block's counter + 1, not a per-row count.
 *   - Coupled L2 applies through g': weight decay acts on touched rows only.
 *   - A touched row whose summed gradient is exactly zero is still updated (weight decay acts on it).
 *   - eps == 0 is accepted (a touched row with a zero gradient and a zero accumulator is then 0 / 0, NaN).
 *   - After the update the row's gradient is set to 0 (a zeroed gradient row: a tables' gradient region that was all
 *     zero before the lists' rows were added is all zero again after the call, with no fill).
 *
 * The _sched call reads the rate from a schedule block (include/dfwfm_lr_schedule.h), evaluated by every workgroup at
 * counter + 1; hyper->lr is then unused (and not checked).  At step s its result equals, bit for bit, the unscheduled
 * call's with lr = dfwfm_lr_schedule_eval(s).
 *
 * -- As the two parents check their arguments: the errors.
 *
 * DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for
 *   - the hyper-parameters: a null hyper, a kind other than DFWFM_OPTIM_ADAGRAD, a hyper-parameter (lr, weight_decay,
 *     momentum, alpha, eps) that is NaN, infinite or negative, alpha outside [0, 1) (momentum and alpha are checked as
 *     dfwfm_optim_step_dev checks them, and are not read otherwise);
 *   - a null state block or schedule block, a null grad, a null span array with n_spans > 0, a null list array with
 *     n_lists > 0, n_spans < 0, n_lists < 0;
 *   - per span: a null param, state or stamp, rows < 1, width < 1, offset < 0, a span that overlaps another or whose
 *     end does not fit 63 bits;
 *   - per list: cap < 0, a null dest or count, width < 1 or a width that matches no span.
 * DFWFM_ERR_UNSUPPORTED: a list too long for a 32-bit grid (cap / 256 above 2^30).
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_ROWWISE_LISTS_H
#define DFWFM_ROWWISE_LISTS_H

#include <stddef.h>
#include <stdint.h>

#include "../include/dfwfm.h"
#include "../include/dfwfm_lazy_lists.h"
#include "../include/dfwfm_optim.h"
#include "../include/dfwfm_rowwise_adagrad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_ROWWISE_LISTS_ABI_VERSION 1

#define DFWFM_ROWWISE_LISTS_SPANS_PER_LAUNCH 60
#define DFWFM_ROWWISE_LISTS_LISTS_PER_LAUNCH 24

/* One table: dfwfm_lazy_lists_span plus its accumulators.  Device pointers; rows of `width` floats, 4-byte aligned. */
typedef struct {
  float* param;        /* [rows, width]: the table's own tensor                                  */
  float* state;        /* [rows]: the rows' accumulators; zero-filled once by the caller; never NULL */
  int32_t* stamp;      /* [rows], zero-filled once by the caller together with the state block   */
  int64_t offset;      /* >= 0: floats from the start of grad (the gradient only)                */
  int64_t rows;        /* >= 1                                                                   */
  int32_t width;       /* >= 1 floats per row                                                    */
  int32_t reserved;
} dfwfm_rowwise_lists_span;

int dfwfm_rowwise_lists_abi_version(void);

/* The row-wise Adagrad step over the rows the lists name.  spans and lists are host arrays, read during the call; grad
 * is the flat device array the spans' offsets and the lists' destinations index.  Of the hyper-parameters lr,
 * weight_decay and eps are read; kind must be DFWFM_OPTIM_ADAGRAD.  Needs no model. */
int dfwfm_rowwise_adagrad_lists_step_dev(const dfwfm_rowwise_lists_span* spans, int32_t n_spans,
                                         const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad,
                                         const dfwfm_optim_hyper* hyper, void* state_dev, void* stream);

/* ... with the rate read from sched_dev (DFWFM_LR_SCHEDULE_BYTES, written by dfwfm_lr_schedule_write) when the
 * kernels run. */
int dfwfm_rowwise_adagrad_lists_step_dev_sched(const dfwfm_rowwise_lists_span* spans, int32_t n_spans,
                                               const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad,
                                               const dfwfm_optim_hyper* hyper, const void* sched_dev, void* state_dev,
                                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_ROWWISE_LISTS_H */
