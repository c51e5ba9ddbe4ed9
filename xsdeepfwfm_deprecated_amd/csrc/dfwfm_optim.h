// dfwfm_optim.h -- the per-element arithmetic of torch.optim.SGD / Adagrad / RMSprop and the step's scalars
// (include/dfwfm_optim.h: the contract), shared by the kernels (dfwfm_optim.hip) and the host's
// dfwfm_optim_elem_ref (dfwfm_capi.hip), so that an element gets the same bits from either.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dfwfm_internal.h"

namespace dfwfm {

// the kernels' kinds: include/dfwfm_optim.h's, with plain SGD (no state array) apart from momentum-SGD
enum OptimKind { kOptSgd = 0, kOptSgdMom = 1, kOptAdagrad = 2, kOptRmsprop = 3 };

struct OptimHyper {
  double lr, wd, momentum, alpha, eps;
};

// the step's f32 scalars: formed in double from the Python floats, rounded once per use (as adam_coef does)
struct OptimCoef {
  float neg_lr, wd, mom, alpha, oma, eps;
  int32_t first;  // step 1: momentum-SGD's buffer is a copy of the gradient
};

__host__ __device__ inline OptimCoef optim_coef(int64_t step, const OptimHyper& h, double lr) {
  return OptimCoef{(float)(-lr), (float)h.wd, (float)h.momentum, (float)h.alpha, (float)(1.0 - h.alpha), (float)h.eps,
                   step == 1 ? 1 : 0};
}

// one element.  Every fused multiply-add is an fmaf; with contraction off no other product meets a sum, so the host
// compiler and the device compiler have no choice left, whatever the call site.  sqrt and the division are the
// correctly rounded ones on both sides.
template <int K>
__host__ __device__ __forceinline__ void optim_elem(const OptimCoef& c, float& p, float g, float& s) {
#pragma clang fp contract(off)
  if (c.wd != 0.f) g = fmaf(c.wd, p, g);  // grad.add(param, alpha=wd)
  if (K == kOptSgd) {
    p = fmaf(g, c.neg_lr, p);  // param.add_(grad, alpha=-lr)
    return;
  }
  if (K == kOptSgdMom) {
    if (c.first) {
      s = g;  // torch.clone(grad)
    } else {
      const float t = s * c.mom;  // buf.mul_(momentum).add_(grad)
      s = t + g;
    }
    p = fmaf(s, c.neg_lr, p);
    return;
  }
  if (K == kOptAdagrad) s = fmaf(g, g, s);                                // state_sum.addcmul_(grad, grad)
  else s = fmaf(g, c.oma * g, s * c.alpha);                               // square_avg.mul_(alpha).addcmul_(g, g, 1-alpha)
  // sqrtf and `/` are IEEE on both sides: the library is built with hipcc's default correctly rounded f32 division and
  // square root.  (__fsqrt_rn is NOT: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define it as the native,
  // 1-ulp square root, and some elements then get another parameter than the host's.)
  const float den = sqrtf(s) + c.eps;                                     // sqrt().add_(eps)
  const float num = c.neg_lr * g;
  p = p + num / den;                                                      // param.addcdiv_(grad, den, value=-lr)
}

// the last workgroup of a step's last launch (ticket == nwg - 1): advance the counter.  The block's f32 slots hold
// the last step's scalars for diagnostics, as after an Adam step: the rate's slot gets lr, the others what applies.
// (Shared by the dense kernels, dfwfm_optim.hip, and the row-lazy one, dfwfm_lazy_optim.hip.)
__device__ __forceinline__ void optim_advance(AdamDevState* __restrict__ st, const OptimCoef& c, int64_t step) {
  st->step_size = -c.neg_lr;
  st->omb1 = c.mom;
  st->b2 = c.alpha;
  st->omb2 = c.oma;
  st->eps = c.eps;
  st->wd = c.wd;
  st->bc2_sqrt = 0.f;
  st->ticket = 0;
  st->step = step;
}

// One tensor of a launch: 32 bytes, so that more tensors than Adam's 91 fit a launch's arguments.
struct OptimTensor {
  float* p;
  const float* g;
  float* s;  // null for kOptSgd
  int64_t n;
};
constexpr int kOptimList = 108;  // tensors per launch (the list is a kernel argument, < 4 KiB with the rest)
struct OptimList {
  OptimTensor t[kOptimList];
  int32_t block0[kOptimList];  // first block of each tensor
  int32_t n;
  int32_t pad;
};
// the rest of a launch's arguments
struct OptimArgs {
  AdamDevState* st;         // null: the step number is `step` (dfwfm_optim_step), nothing advances
  const LrSchedule* sched;  // non-null: the rate is its value at the step, h.lr unused
  OptimHyper h;
  int64_t step;
  int32_t bump, nblocks;
};
static_assert(sizeof(OptimTensor) == 32, "optim tensor entry");
static_assert(sizeof(OptimList) + sizeof(OptimArgs) + 64 <= 4096, "optim launch arguments over 4 KiB");

// one launch of `kind` over the list's nblocks blocks of kAdamBlock elements (a bounded grid of kAdamGrid workgroups)
hipError_t launch_optim(int kind, const OptimList& list, const OptimArgs& a, hipStream_t s);

}  // namespace dfwfm
