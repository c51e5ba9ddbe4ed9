/*
 * dfwfm_optim.h -- C ABI of the SGD, Adagrad and RMSprop steps of the fused training step (libdfwfm.so, beside
 * include/dfwfm.h, include/dfwfm_lazy_adam.h and include/dfwfm_lr_schedule.h).
 *
 * The reference's fit() builds one of four optimizers: torch.optim.SGD(lr, momentum, weight_decay) unless its
 * optimizer_type is 'adam', 'rmsp' or 'adag'.  dfwfm_adam_step_dev is the first; this header adds the other three as
 * graph-replayable steps over a tensor list, with the step counter (and optionally the learning rate) read from
 * device memory.  Opt-in: nothing in include/dfwfm.h, include/dfwfm_lazy_adam.h or include/dfwfm_lr_schedule.h
 * changes, and nothing calls this unless asked to.
 *
 * The contract.
 *
 * The optimizers are torch.optim's, as the reference constructs them (single-tensor forms):
 *   - DFWFM_OPTIM_SGD      torch.optim.SGD(lr, momentum, weight_decay): dampening 0, no Nesterov;
 *   - DFWFM_OPTIM_ADAGRAD  torch.optim.Adagrad(lr, weight_decay, eps): lr_decay 0, initial_accumulator_value 0;
 *   - DFWFM_OPTIM_RMSPROP  torch.optim.RMSprop(lr, alpha, eps, weight_decay): momentum 0, not centered.
 * Each carries at most ONE state array per tensor (`state`): the momentum buffer, `sum` or `square_avg`, zero-filled
 * once by the caller.  SGD with momentum == 0 carries none (state may be NULL and is never touched).  Per parameter a
 * step moves 20 bytes (12 for plain SGD) where Adam moves 28.
 *
 * The arithmetic, per element, in f32, every rounding written out (round(x) is one rounding to f32; fmaf is ONE fused
 * multiply-add with a single rounding, explicit, because this compiler otherwise fuses a product into a sum or not per
 * call site; products and sums outside an fmaf are never fused: the function is compiled with contraction off):
 *   all kinds   g' = fmaf(wd, p, g) when wd != 0, else g' = g                        (grad.add(param, alpha=wd))
 *   SGD         momentum != 0:  buf = g' at step 1 (torch clones the gradient: a branch on the step number, so that
 *                               a -0 keeps its sign), else buf = round(buf * momentum) + g';   d = buf
 *               momentum == 0:  d = g'
 *               p = fmaf(d, -lr, p)
 *   Adagrad     sum = fmaf(g', g', sum);   std = sqrt(sum) + eps;   p = p + round(round(-lr * g') / std)
 *   RMSprop     sq = fmaf(g', round((1 - alpha) * g'), round(sq * alpha));   avg = sqrt(sq) + eps;
 *               p = p + round(round(-lr * g') / avg)
 * The scalars -lr, wd, momentum, alpha, 1 - alpha and eps are formed in double from the hyper-parameters (the Python
 * floats torch starts from) and rounded to f32 once.  The updates contain no pow and no transcendental: only fmaf,
 * products, sums, one correctly rounded sqrt and one correctly rounded division.  So the host function
 * dfwfm_optim_elem_ref and the kernels give the same 32 bits for every input, on the 16-byte path and on the
 * element-wise path alike (arrays off the 16-byte grid, the last numel % 4 elements of a tensor).
 *
 * Against torch.optim 2.10 on the CPU: SGD's parameters and momentum buffer, Adagrad's sum and RMSprop's square_avg
 * are bit-identical; Adagrad's and RMSprop's parameters differ in a few elements per thousand by one rounding (ATen's
 * vector path forms the quotient differently).
 *
 * The step number.  dfwfm_optim_step takes it from the host.  dfwfm_optim_step_dev reads a device block of
 * DFWFM_ADAM_STATE_BYTES (include/dfwfm.h: the block of dfwfm_adam_step_dev, zero-filled once; its int64 step counter
 * comes first, where dfwfm_set_step_source reads it): every workgroup takes step = counter + 1, and the last
 * workgroup to finish in the call's last launch advances the counter (the same ticket scheme; the ticket is 0 again
 * afterwards).  A call with no tensor to step still advances it (one empty workgroup).  The step number matters to
 * the arithmetic only for momentum-SGD's first step.
 *
 * dfwfm_optim_step_dev_sched reads the rate from a schedule block (include/dfwfm_lr_schedule.h), evaluated by every
 * workgroup at counter + 1; hyper->lr is then unused (and not checked).  At step s its result equals, bit for bit,
 * the unscheduled call's with lr = dfwfm_lr_schedule_eval(s).
 *
 * The calls are stream-ordered: launches only, no host synchronisation, no allocation; the tensor list travels in
 * the kernel arguments (up to 108 tensors per launch; a longer list takes several launches).  They can be captured
 * into a HIP graph; a replay reads gradients, counter and schedule afresh.  Tensors must not alias.  A tensor with a
 * NULL grad or numel <= 0 is skipped.
 *
 * Errors: DFWFM_ERR_INVALID_ARG with dfwfm_last_error set and no launch for a null hyper / state block / schedule
 * block / tensor array (n > 0), n < 0, an unknown kind, a hyper-parameter (lr, weight_decay, momentum, alpha, eps)
 * that is NaN, infinite or negative, alpha outside [0, 1), step < 1 (dfwfm_optim_step), and per stepped tensor a null
 * param, or a null state where the kind needs one (every kind but SGD with momentum == 0).
 * DFWFM_ERR_UNSUPPORTED: a tensor of more than 2^31 - 1 blocks of 4096 elements.
 *
 * Status codes and dfwfm_last_error as in dfwfm.h.  No call aborts.
 */
#ifndef DFWFM_OPTIM_H
#define DFWFM_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#include "dfwfm.h"
#include "dfwfm_lr_schedule.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFWFM_OPTIM_ABI_VERSION 1

typedef enum {
  DFWFM_OPTIM_SGD = 0,
  DFWFM_OPTIM_ADAGRAD = 1,
  DFWFM_OPTIM_RMSPROP = 2
} dfwfm_optim_kind;

/* One tensor of a step.  Device pointers, 4-byte aligned (16-byte aligned arrays take the 16-byte path). */
typedef struct {
  float* param;
  const float* grad; /* NULL: the tensor is skipped                                          */
  float* state;      /* momentum buffer / sum / square_avg; NULL for SGD with momentum == 0  */
  int64_t numel;
} dfwfm_optim_tensor;

/* The hyper-parameters, as the Python floats torch starts from.  The reference's defaults: RMSprop alpha = 0.99,
 * eps = 1e-8; Adagrad eps = 1e-10; SGD momentum = 0.  momentum is read by SGD, alpha by RMSprop, eps by Adagrad and
 * RMSprop; all of them are checked for every kind. */
typedef struct {
  int32_t kind; /* dfwfm_optim_kind */
  int32_t reserved;
  double lr, weight_decay, momentum, alpha, eps;
} dfwfm_optim_hyper;

int dfwfm_optim_abi_version(void);

/* Step number `step` (1-based, from the host) over n tensors (a host array, read during the call). */
int dfwfm_optim_step(const dfwfm_optim_tensor* tensors, int32_t n, const dfwfm_optim_hyper* hyper, int64_t step,
                     void* stream);

/* The same with the step number read from state_dev (DFWFM_ADAM_STATE_BYTES of device memory) when the kernels run,
 * and advanced once by the call. */
int dfwfm_optim_step_dev(const dfwfm_optim_tensor* tensors, int32_t n, const dfwfm_optim_hyper* hyper,
                         void* state_dev, void* stream);

/* dfwfm_optim_step_dev with the rate read from sched_dev (DFWFM_LR_SCHEDULE_BYTES, written by
 * dfwfm_lr_schedule_write) when the kernels run. */
int dfwfm_optim_step_dev_sched(const dfwfm_optim_tensor* tensors, int32_t n, const dfwfm_optim_hyper* hyper,
                               const void* sched_dev, void* state_dev, void* stream);

/* Host only, no GPU needed: one element of step `step` by exactly the arithmetic the kernels use.  *p and *state are
 * read and written (state may be NULL for SGD with momentum == 0). */
int dfwfm_optim_elem_ref(const dfwfm_optim_hyper* hyper, int64_t step, float* p, float g, float* state);

#ifdef __cplusplus
}
#endif

#endif /* DFWFM_OPTIM_H */
