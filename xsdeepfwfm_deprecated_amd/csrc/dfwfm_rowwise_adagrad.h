// dfwfm_rowwise_adagrad.h -- the arithmetic and the launch arguments of the row-wise Adagrad step
// (include/dfwfm_rowwise_adagrad.h: the contract; dfwfm_rowwise_adagrad.hip: the key-driven kernel;
// dfwfm_rowwise_lists.hip: the list-driven one).  The arithmetic's pieces are shared by the kernels and the host's
// dfwfm_rowwise_adagrad_row_ref (dfwfm_capi.hip), and the two row functions by both kernels, so that a row gets the
// same bits from any of them.
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

// an owned row of width 1, by its owning lane (p, g: the row's one parameter and gradient; acc: its accumulator)
__device__ __forceinline__ void rowwise_update_one(const OptimCoef& c, float* __restrict__ p, float* __restrict__ g,
                                                   float* __restrict__ acc) {
  const float pv = *p;
  const float gp = rowwise_grad(c, pv, *g);
  float a = *acc;
  const float std = rowwise_std(c, rowwise_link(gp, 0.f), 1, a);
  *acc = a;
  *p = rowwise_elem(c, pv, gp, std);
  *g = 0.f;
}

// an owned row by the kLazyGroup lanes of one group, all of which call this with the same row (p, g: the row's first
// parameter and gradient element; acc: its accumulator; W: its width; l: the lane's place in its group).  The shuffles
// stay inside the group and run under group-uniform control flow only: a lane whose element lies past the row's end
// still takes part, holding a value no link reads.
__device__ __forceinline__ void rowwise_update_group(const OptimCoef& c, float* __restrict__ p, float* __restrict__ g,
                                                     float* __restrict__ acc, int W, int l) {
  float a = *acc;
  float ss = 0.f, p0 = 0.f, g0 = 0.f, p1 = 0.f, g1 = 0.f;  // (p0, g0), (p1, g1): elements l and l + kLazyGroup
  for (int base = 0; base < W; base += kLazyGroup) {
    const int e = base + l;
    float pv = 0.f, gp = 0.f;
    if (e < W) {
      pv = p[e];
      gp = rowwise_grad(c, pv, g[e]);
    }
    if (base == 0) {
      p0 = pv;
      g0 = gp;
    } else if (base == kLazyGroup) {
      p1 = pv;
      g1 = gp;
    }
    const int m = W - base < kLazyGroup ? W - base : kLazyGroup;
    for (int j = 0; j < m; ++j) ss = rowwise_link(__shfl(gp, j, kLazyGroup), ss);  // element base + j, in order
  }
  const float std = rowwise_std(c, ss, W, a);
  if (l == 0) *acc = a;
  if (l < W) {
    p[l] = rowwise_elem(c, p0, g0, std);
    g[l] = 0.f;
  }
  if (l + kLazyGroup < W) {
    p[l + kLazyGroup] = rowwise_elem(c, p1, g1, std);
    g[l + kLazyGroup] = 0.f;
  }
  for (int e = 2 * kLazyGroup + l; e < W; e += kLazyGroup) {  // wider than two registers per lane: re-read
    const float pv = p[e];
    const float gp = rowwise_grad(c, pv, g[e]);
    p[e] = rowwise_elem(c, pv, gp, std);
    g[e] = 0.f;
  }
}

// A launch takes the row-lazy step's arguments (dfwfm_lazy_optim.h): LazyOptimTable with `s` one float per ROW, never
// null; up to kLazyOptimList tables, nblocks work blocks of 256 samples; a.h.lr / wd / eps are read.  With `bump` (the
// call's last launch) the last workgroup to finish advances the counter.
hipError_t launch_rowwise_adagrad(const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s);

}  // namespace dfwfm
