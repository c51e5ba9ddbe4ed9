/*
 * dfwfm_lr_schedule.h -- C ABI of device-resident learning-rate schedules for the graph-replayable Adam steps
 * (libdfwfm.so, beside include/dfwfm.h and include/dfwfm_lazy_adam.h).
 *
 * dfwfm_adam_step_dev and dfwfm_lazy_adam_step_dev read the step counter, the bias corrections and the dropout seed
 * from device memory when their kernels run, which is what lets one captured HIP graph serve every step.  The learning
 * rate alone is a kernel argument, baked into a graph at capture.  This header adds the same two steps with the rate
 * read from a small device block instead: a schedule.  Opt-in: nothing in include/dfwfm.h or include/dfwfm_lazy_adam.h
 * changes, and nothing calls this unless asked to.
 *
 * The contract.
 *
 * A schedule is a piecewise-linear table of n knots (step[i], lr[i]), 1 <= n <= DFWFM_LR_MAX_KNOTS, in a device block
 * of DFWFM_LR_SCHEDULE_BYTES (16-byte aligned): an int32 knot count, padding to 16 bytes, then DFWFM_LR_MAX_KNOTS
 * knots.  The knot steps are strictly increasing and at least 1; every lr is finite and >= 0.
 *
 * The schedule's value at step s, evaluated in double with every rounding fixed:
 *   - s <= step[0]:     lr[0];
 *   - s >= step[n-1]:   lr[n-1];
 *   - otherwise, with step[i] <= s < step[i+1]:
 *       t  = (double)(s - step[i]) / (double)(step[i+1] - step[i])      (the integer differences are exact; each
 *                                                                        conversion and the quotient round once)
 *       lr = fma(lr[i+1] - lr[i], t, lr[i])                             (the difference rounds once; then ONE explicit
 *                                                                        fma: a product and a sum written separately
 *                                                                        are fused or not per call site under this
 *                                                                        compiler, an fma cannot be split)
 * dfwfm_lr_schedule_eval (host, std::fma) and the device kernels use this order and give the same 64 bits for every
 * input.
 *
 * Where it is evaluated.  Every workgroup of a scheduled Adam launch evaluates the schedule at the step it is about to
 * take -- its state block's step counter + 1 -- beside the bias corrections, and uses the result where the unscheduled
 * call uses its kernel argument lr.  The knots are loaded lane-parallel (lane k loads knot k) together with the
 * counter, so the schedule adds no dependent memory round trip.
 *
 * The update.  At step s the scheduled calls do for every element exactly what dfwfm_adam_step_dev /
 * dfwfm_lazy_adam_step_dev do with lr = schedule(s) -- the same bits: adam_coef gets that double, the per-element
 * arithmetic is theirs, and so are the counter advance, the empty-list / empty-batch behaviour and the lazy step's
 * touched rows and stamps.  State blocks that advance in lockstep see the same rate.
 *
 * Rewriting.  dfwfm_lr_schedule_write is one tiny launch that takes the knots as kernel arguments (no host staging, no
 * synchronisation, no allocation) and is stream-ordered: the host may rewrite the block between steps and the next
 * replay of a captured graph uses the new schedule -- no recapture.  The write itself can be captured.  A constant
 * rate chosen on the host is the single knot (1, lr).
 *
 * Errors: DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for a null pointer, n < 1 or
 * n > DFWFM_LR_MAX_KNOTS, a first step below 1, steps not strictly increasing, an lr that is NaN, infinite or negative
 * (0 is allowed).  The scheduled step calls keep every check of their unscheduled twins, and need a non-null
 * schedule block (whose contents they cannot check: it is device memory written by dfwfm_lr_schedule_write).
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_LR_SCHEDULE_H
#define DFWFM_LR_SCHEDULE_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"
#include "dfwfm_lazy_adam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_LR_SCHEDULE_ABI_VERSION 1

#define DFWFM_LR_MAX_KNOTS 64

typedef struct {
  int64_t step; /* >= 1, strictly increasing along the table */
  double lr;    /* finite, >= 0                              */
} dfwfm_lr_knot;

/* the device block: int32 count, 12 bytes of padding, DFWFM_LR_MAX_KNOTS knots; 16-byte aligned */
#define DFWFM_LR_SCHEDULE_BYTES (16 + 16 * DFWFM_LR_MAX_KNOTS)

int dfwfm_lr_schedule_abi_version(void);

/* Host only, no GPU needed: *lr = the schedule's value at `step` (any int64), by the arithmetic above. */
int dfwfm_lr_schedule_eval(const dfwfm_lr_knot* knots, int32_t n, int64_t step, double* lr);

/* Stream-ordered rewrite of the device block sched_dev (DFWFM_LR_SCHEDULE_BYTES) with the n knots of a host array,
 * read during the call. */
int dfwfm_lr_schedule_write(void* sched_dev, const dfwfm_lr_knot* knots, int32_t n, void* stream);

/* dfwfm_adam_step_dev (include/dfwfm.h) with the rate read from sched_dev when the kernels run. */
int dfwfm_adam_step_dev_sched(const dfwfm_adam_tensor* tensors, int32_t n, const void* sched_dev, double beta1,
                              double beta2, double eps, double weight_decay, void* state_dev, void* stream);

/* dfwfm_lazy_adam_step_dev (include/dfwfm_lazy_adam.h) with the rate read from sched_dev when the kernels run. */
int dfwfm_lazy_adam_step_dev_sched(const dfwfm_lazy_adam_table* tables, int32_t n, const int64_t* xi,
                                   int64_t xi_stride, int64_t batch, const void* sched_dev, double beta1, double beta2,
                                   double eps, double weight_decay, void* state_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_LR_SCHEDULE_H */
