// dfwfm_rowwise_adagrad.h -- the arithmetic and the launch arguments of the row-wise Adagrad step
// (include/dfwfm_rowwise_adagrad.h: the contract; dfwfm_rowwise_adagrad.hip: the kernel).  The arithmetic's pieces
// are shared by the kernel and the host's dfwfm_rowwise_adagrad_row_ref (dfwfm_capi.hip), so that a row gets the same
// bits from either.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dfwfm_internal.h"
#include "dfwfm_lazy_optim.h"
#include "dfwfm_optim.h"

namespace dfwfm {

// The pieces of one row's update.  Every fused multiply-add is an fmaf; with contraction off no other product meets a
// sum, so the host compiler and the device compiler have no choice left, whatever the call site.  sqrtf and `/` are
// the correctly rounded ones on both sides (dfwfm_optim.h: optim_elem).
// g' = grad.add(param, alpha=wd)
__host__ __device__ __forceinline__ float rowwise_grad(const OptimCoef& c, float p, float g) {
#pragma clang fp contract(off)
  return c.wd != 0.f ? fmaf(c.wd, p, g) : g;
}
// one link of the row's chain, ss = fmaf(g', g', ss): the links run in element order, on one thread or on every lane
// of a group alike
__host__ __device__ __forceinline__ float rowwise_link(float gp, float ss) {
#pragma clang fp contract(off)
  return fmaf(gp, gp, ss);
}
// the accumulator takes the row's mean squared gradient; returns std = sqrt(acc) + eps
__host__ __device__ __forceinline__ float rowwise_std(const OptimCoef& c, float ss, int32_t width, float& acc) {
#pragma clang fp contract(off)
  const float mean = ss / (float)width;
  acc = acc + mean;
  return sqrtf(acc) + c.eps;
}
// one element: param.addcdiv_(g', std, value=-lr)
__host__ __device__ __forceinline__ float rowwise_elem(const OptimCoef& c, float p, float gp, float std) {
#pragma clang fp contract(off)
  const float num = c.neg_lr * gp;
  return p + num / std;
}

// A launch takes the row-lazy step's arguments (dfwfm_lazy_optim.h): LazyOptimTable with `s` one float per ROW, never
// null; up to kLazyOptimList tables, nblocks work blocks of 256 samples; a.h.lr / wd / eps are read.  With `bump` (the
// call's last launch) the last workgroup to finish advances the counter.
hipError_t launch_rowwise_adagrad(const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s);

}  // namespace dfwfm
