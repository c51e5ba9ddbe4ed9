/*
 * dfwfm_lazy_lists.h -- C ABI of the row-lazy table optimizers driven by exchanged touched-row lists (libdfwfm.so,
 * beside include/dfwfm_lazy_adam.h and include/dfwfm_lazy_optim.h).
 *
 * dfwfm_lazy_adam_step_dev and dfwfm_lazy_optim_step_dev find the touched rows from the keys of the batch the process
 * itself ran.  Under data parallelism a rank sees only its slice of the global batch, while every replica has to update
 * the rows the GLOBAL batch touched: the union of every rank's touched-row list, which every rank already holds after
 * the exchange and which dfwfm_sparse_grads_apply (include/dfwfm.h) walks to add the rows' gradients.  The calls of
 * this header take the touched rows from those lists instead of from keys.  Opt-in: no other header changes, and
 * nothing calls this unless asked to.
 *
 * The contract.
 *
 * Spans.  A span is one table as a slice of the caller's flat buffers: its own `param` tensor [rows, width], its
 * `stamp` array [rows], and `offset`, the index in floats at which its rows start in the flat `grad` array and in the
 * flat moment / state arrays (exp_avg and exp_avg_sq, or opt_state) -- ONE offset for all of them, the layout of a
 * trainer that keeps gradients and optimizer state in flat buffers of the same shape.  Spans may come in any order;
 * they must not overlap.
 *
 * Lists.  A list is what dfwfm_sparse_grads_local writes and dfwfm_sparse_grads_apply reads: `dest` (device, int64),
 * `count` (device, one int32) and the capacity `cap`, for rows of `width` floats.  dest[e] is the offset in floats of
 * a row's first element in the flat gradient buffer; destinations are unique within a list; the reader stops at
 * min(*count, cap) (a count below 0 reads nothing).  One list per (rank, table family) of a data-parallel step.
 *
 * Touched rows.  A row is *touched* by a call when at least one list names its destination: dest[e] ==
 * span.offset + row * span.width for a span of the list's width and a row < span.rows.  A dest that falls in no span
 * of the list's width, or between two rows of one, is skipped: it is not written, it is not an error, and no address
 * is formed from it.
 *
 * The update.  For every element of a touched row the call does exactly what dfwfm_adam_step_dev (include/dfwfm.h) /
 * dfwfm_optim_step_dev (include/dfwfm_optim.h) does for that element given the same (p, g, m, v | state), the same
 * hyper-parameters and the same step number -- the same bits:
 *   - the arithmetic is the dense kernels' per-element function (adam_elem, csrc/dfwfm_adam.h: the form of
 *     include/dfwfm_lazy_adam.h; optim_elem, csrc/dfwfm_optim.h, compiled with contraction off as there: the bits of
 *     dfwfm_optim_elem_ref);
 *   - the step is the state block's step counter + 1: the GLOBAL step, not a per-row count of how often the row was
 *     touched (a row listed at steps 1 and 3 gets step 3's coefficients at step 3, and nothing at step 2);
 *   - coupled L2 applies: weight decay acts on touched rows only;
 *   - a touched row whose summed gradient is exactly zero is still updated;
 *   - after the update the row's gradient is set to 0 (a zeroed gradient row: a tables' gradient region that was all
 *     zero before the lists' rows were added is all zero again after the call, with no fill).
 * Versus the dense update the statements of include/dfwfm_lazy_adam.h and include/dfwfm_lazy_optim.h hold unchanged:
 * plain SGD and Adagrad (eps > 0) with weight_decay == 0 coincide bit for bit, Adam with weight_decay == 0 for the
 * first step from zero-filled moments; everything else is ANOTHER optimizer.
 *
 * The rest.
 *   - A row named by several lists (several ranks touched it) is updated once.
 *   - Untouched rows keep the bits of param and of the moments / state; their grad is neither read nor written.
 *   - `opt_state` is the kind's one flat state array; SGD with momentum == 0 carries none: it may be NULL and no
 *     address is formed from it.
 *   - The call advances the state block's step counter exactly once: every workgroup takes step = counter + 1, and the
 *     last workgroup to finish in the call's last launch advances it (the ticket scheme of the dense calls).  With no
 *     span, no list or all counts zero no row is updated and the step counter STILL advances (one empty workgroup).
 *   - The call is stream-ordered: launches only, no host synchronisation, no allocation on the device (not on the first
 *     call either).  Spans and list descriptors travel as kernel arguments, up to DFWFM_LAZY_LISTS_SPANS_PER_LAUNCH (64)
 *     spans and DFWFM_LAZY_LISTS_LISTS_PER_LAUNCH (32) lists per launch; longer arrays take several launches (one per
 *     pair of a 64-span piece and a 32-list piece).  The call can be captured into a HIP graph; a replay reads the
 *     counts, the destinations, the gradients, the counter and the schedule afresh.
 *   - Rows are independent, so the result does not depend on which thread claims a row: given equal gradients the
 *     result is bit-identical from run to run.
 *
 * Stamps: the scheme of include/dfwfm_lazy_adam.h.  A row is claimed by a device-scope look at stamp[row] and, unless
 * it already holds this step's stamp, one atomic exchange with it; whoever reads back another value owns the row.
 * The step's stamp is (step - 1) mod (2^32 - 1) + 1, never 0, so stamps start at zero together with the state block
 * (both zero-filled by the caller).  After 2^32 - 1 steps the stamps repeat.  Two spans must not share stamps.
 *
 * The _sched calls read the rate from a schedule block (include/dfwfm_lr_schedule.h), evaluated by every workgroup at
 * counter + 1; `lr` / hyper->lr is then unused (and not checked).  At step s the result equals, bit for bit, the
 * unscheduled call's with lr = dfwfm_lr_schedule_eval(s).
 *
 * Errors: DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for
 *   - a null state block or schedule block, a null grad, a null exp_avg or exp_avg_sq (Adam), a null opt_state where
 *     the optimizer needs one (every kind but SGD with momentum == 0), a null span array with n_spans > 0, a null list
 *     array with n_lists > 0, n_spans < 0, n_lists < 0;
 *   - the hyper-parameters, as the dense calls check them (dfwfm_optim_step_dev: a null hyper, an unknown kind, a
 *     hyper-parameter that is NaN, infinite or negative, alpha outside [0, 1); dfwfm_adam_step_dev checks none);
 *   - per span: a null param or stamp, rows < 1, width < 1, offset < 0, a span that overlaps another or whose end
 *     does not fit 63 bits;
 *   - per list: cap < 0, a null dest or count, width < 1 or a width that matches no span.
 * DFWFM_ERR_UNSUPPORTED: a list too long for a 32-bit grid (cap / 256 above 2^30).
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_LAZY_LISTS_H
#define DFWFM_LAZY_LISTS_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"
#include "dfwfm_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_LAZY_LISTS_ABI_VERSION 1

#define DFWFM_LAZY_LISTS_SPANS_PER_LAUNCH 64
#define DFWFM_LAZY_LISTS_LISTS_PER_LAUNCH 32

/* One table as a slice of the flat buffers.  Device pointers; rows of `width` floats, 4-byte aligned. */
typedef struct {
  float* param;        /* [rows, width]: the table's own tensor                                  */
  int32_t* stamp;      /* [rows], zero-filled once by the caller together with the state block   */
  int64_t offset;      /* >= 0: floats from the start of grad / the moments / opt_state          */
  int64_t rows;        /* >= 1                                                                   */
  int32_t width;       /* >= 1 floats per row                                                    */
  int32_t reserved;
} dfwfm_lazy_lists_span;

/* One exchanged touched-row list (the dest / count / capacity of dfwfm_sparse_grads_apply). */
typedef struct {
  const int64_t* dest;   /* [cap] device: float offsets of rows' first elements in grad, unique  */
  const int32_t* count;  /* device: entries written; read up to min(*count, cap)                 */
  int64_t cap;           /* >= 0                                                                 */
  int32_t width;         /* >= 1: the width of the rows the list names                           */
  int32_t reserved;
} dfwfm_lazy_lists_list;

int dfwfm_lazy_lists_abi_version(void);

/* The lazy Adam step over the rows the lists name, with dfwfm_adam_step_dev's hyper-parameters and state block
 * (DFWFM_ADAM_STATE_BYTES of device memory, zero-filled once).  spans and lists are host arrays, read during the
 * call; grad, exp_avg and exp_avg_sq are the flat device arrays the spans' offsets index.  Needs no model. */
int dfwfm_lazy_adam_lists_step_dev(const dfwfm_lazy_lists_span* spans, int32_t n_spans,
                                   const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad, float* exp_avg,
                                   float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, void* state_dev, void* stream);

/* ... with the rate read from sched_dev (DFWFM_LR_SCHEDULE_BYTES, written by dfwfm_lr_schedule_write) when the
 * kernels run. */
int dfwfm_lazy_adam_lists_step_dev_sched(const dfwfm_lazy_lists_span* spans, int32_t n_spans,
                                         const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad,
                                         float* exp_avg, float* exp_avg_sq, const void* sched_dev, double beta1,
                                         double beta2, double eps, double weight_decay, void* state_dev, void* stream);

/* The lazy SGD / Adagrad / RMSprop step over the rows the lists name, with dfwfm_optim_step_dev's hyper-parameters
 * and state block; opt_state is the kind's flat state array (NULL for SGD with momentum == 0). */
int dfwfm_lazy_optim_lists_step_dev(const dfwfm_lazy_lists_span* spans, int32_t n_spans,
                                    const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad, float* opt_state,
                                    const dfwfm_optim_hyper* hyper, void* state_dev, void* stream);

/* ... with the rate read from sched_dev when the kernels run. */
int dfwfm_lazy_optim_lists_step_dev_sched(const dfwfm_lazy_lists_span* spans, int32_t n_spans,
                                          const dfwfm_lazy_lists_list* lists, int32_t n_lists, float* grad,
                                          float* opt_state, const dfwfm_optim_hyper* hyper, const void* sched_dev,
                                          void* state_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_LAZY_LISTS_H */
