// dfwfm_adam.h -- the per-element arithmetic of torch.optim.Adam and the step's scalars, shared by the dense kernels
// (dfwfm_train.hip: adam_kernel, adam_dev_kernel) and the row-lazy one (dfwfm_lazy_adam.hip), so that an element
// updated by either gets the same bits.
// Adam (torch.optim.Adam, single-tensor form, torch/optim/adam.py _single_tensor_adam):
// g += wd * p; m = lerp(m, g, 1 - b1);
// v = v * b2 + (1 - b2) * g * g; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_internal.h"

namespace dfwfm {

// one element of torch.optim.Adam: torch's CPU kernels' evaluation order -- fmadd where ATen's vector path
// uses one, every other product / sum rounded on its own.
// The second moment's sum is ONE fused multiply-add, written out.  The __f*_rn intrinsics are plain operators under
// this compiler, so with the products and the sum as separate statements it was the compiler's choice per call site
// what fused: adam_dev_kernel's 16-byte path fused v b2 into the sum (kAdamFuseV), its element-wise path and
// adam_kernel's 16-byte path fused g ((1-b2) g) instead (kAdamFuseG), and adam_kernel's element-wise path (unaligned
// tensors, the last numel % 4 elements) fused nothing -- one element's bits depended on the kernel and on where it
// sat in its tensor.  An explicit fmaf cannot be split, and the remaining products have no sum left to fuse with.
//   kAdamFuseV  v = fma(v, b2, ((1-b2) g) g): THE form -- dfwfm_adam_step (adam_kernel) on every path, the row-lazy
//               kernel (include/dfwfm_lazy_adam.h: its contract rests on one element having one result), and
//               adam_dev_kernel's 16-byte path, i.e. all of the fused training step but the elements below;
//   kAdamFuseG  v = fma(g, (1-b2) g, v b2): adam_dev_kernel's element-wise path only (in the fused step, whose
//               tensors are all 16-byte aligned: the last numel % 4 elements of a tensor), kept so that the fused
//               step's bits stay what they were.  The two forms agree whenever v is 0 and differ by at most one
//               rounding of v otherwise.
struct AdamCoef {
  float step_size, omb1, b2, omb2, eps, wd, bc2_sqrt;
};
enum AdamForm { kAdamFuseV = 0, kAdamFuseG = 1 };
template <int FORM = kAdamFuseV>
__device__ __forceinline__ void adam_elem(const AdamCoef& c, float& p, float g, float& m, float& v) {
  if (c.wd != 0.f) g = fmaf(c.wd, p, g);                          // grad.add(param, alpha=wd): ATen's fmadd
  m = fmaf(c.omb1, __fsub_rn(g, m), m);                            // exp_avg.lerp_(grad, 1-b1): fmadd, w < 0.5
  if (FORM == kAdamFuseV)                                           // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    v = fmaf(v, c.b2, __fmul_rn(__fmul_rn(c.omb2, g), g));
  else
    v = fmaf(g, __fmul_rn(c.omb2, g), __fmul_rn(v, c.b2));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bc2_sqrt), c.eps);  // sqrt(v)/sqrt(bc2) + eps
  p = __fadd_rn(p, __fdiv_rn(__fmul_rn(-c.step_size, m), denom));  // addcdiv_(m, denom, -lr/bc1)
}

// Graph-replayable Adam: every workgroup derives the step's scalars from the device counter + 1 (in double, as
// torch does from Python floats, then f32) -- no separate prep launch; in the step's last launch the last workgroup
// to finish (a ticket counter) advances the counter, after every workgroup of the step has read it.
__device__ __forceinline__ AdamCoef adam_coef(int64_t step, const AdamHyper& h) {
  const double bc1 = 1.0 - pow(h.b1, (double)step);
  const double bc2 = 1.0 - pow(h.b2, (double)step);
  return AdamCoef{(float)(h.lr / bc1), (float)(1.0 - h.b1), (float)h.b2, (float)(1.0 - h.b2), (float)h.eps,
                  (float)h.wd, (float)sqrt(bc2)};
}

// A device-resident learning-rate schedule's value at step s (include/dfwfm_lr_schedule.h: the contract), by the 64
// lanes of one wave, all of which call this and get the value.  Lane k loads knot k (the block always holds kLrKnots
// of them, so the load needs no count first); these loads, the count's and the caller's load of the step counter do
// not depend on one another and are in flight together: the schedule adds no memory round trip to the head of a
// launch's workgroups, where a search by one thread would add five or six.  The lane that holds the segment (or the
// end) evaluates it -- lr_segment, the host's own function -- and the wave reads its result.  The cases exclude one
// another in a valid table, in the contract's order; a block that was never written yields some knot's lr, no fault.
__device__ __forceinline__ double lr_schedule_value(const LrSchedule* __restrict__ sd, int64_t s) {
  const int lane = threadIdx.x & 63;
  const int n = sd->n;
  const LrKnot a = sd->k[lane];
  const int64_t step_j = (int64_t)__shfl_down((long long)a.step, 1);  // knot lane + 1 (lane 63: its own, unused)
  const double lr_j = __shfl_down(a.lr, 1);
  // (the three cases as flags formed ahead of any branch: with the count first used inside a branch the compiler
  // sinks its load there, behind the wait for the knots -- the dependent round trip this layout is there to avoid)
  const bool first = (lane == 0) & (s <= a.step);
  const bool last = (lane == n - 1) & (s >= a.step);
  const bool seg = (lane + 1 < n) & (a.step <= s) & (s < step_j) & !first;
  const bool hit = first | last | seg;
  double v = a.lr;
  if (seg) v = lr_segment(a.step, a.lr, step_j, lr_j, s);
  const unsigned long long hits = __ballot(hit);
  return __shfl(v, hits ? __ffsll(hits) - 1 : 0);
}

// the last workgroup of a step's last launch (ticket == nwg - 1): record the step's scalars and advance the counter
__device__ __forceinline__ void adam_advance(AdamDevState* __restrict__ st, const AdamCoef& c, int64_t step) {
  st->step_size = c.step_size;
  st->omb1 = c.omb1;
  st->b2 = c.b2;
  st->omb2 = c.omb2;
  st->eps = c.eps;
  st->wd = c.wd;
  st->bc2_sqrt = c.bc2_sqrt;
  st->ticket = 0;
  st->step = step;
}

}  // namespace dfwfm
