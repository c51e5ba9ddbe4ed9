// dfwfm_optim.hip -- the SGD, Adagrad and RMSprop steps over a tensor list (include/dfwfm_optim.h: the contract).
//
// The shape is the dense Adam's (adam_block / adam_dev_part, dfwfm_train.hip): the tensor list travels in the kernel
// arguments, a binary search over block0 finds a block's tensor, a bounded grid of kAdamGrid workgroups walks the
// kAdamBlock-element blocks, and every 16-byte load of a block (12: parameter, gradient, state; 8 for plain SGD)
// issues before the first update.  Every workgroup reads the step counter first; the last one to finish in the
// call's last launch advances it (the dense kernel's ticket).  One template over the kind: plain SGD never forms an
// address from its (null) state pointer.  No LDS beyond the step's scalars.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_adam.h"
#include "dfwfm_internal.h"
#include "dfwfm_optim.h"

namespace dfwfm {

template <int K>
__device__ __forceinline__ void optim_block(const OptimList& list, const OptimCoef& c, int bid) {
  constexpr bool kState = K != kOptSgd;
  if (list.n <= 0) return;
  int lo = 0, hi = list.n - 1;
  while (lo < hi) {  // last tensor whose block0 <= bid
    const int mid = (lo + hi + 1) >> 1;
    if (list.block0[mid] <= bid) lo = mid;
    else hi = mid - 1;
  }
  const OptimTensor T = list.t[lo];
  const int64_t i0 = (int64_t)(bid - list.block0[lo]) * kAdamBlock;
  const bool vec = (((uintptr_t)T.p | (uintptr_t)T.g | (kState ? (uintptr_t)T.s : (uintptr_t)0)) & 15) == 0;
  if (!vec) {
    // arrays off the 16-byte grid: lane-consecutive elements
    for (int64_t j = i0 + threadIdx.x; j < i0 + kAdamBlock && j < T.n; j += 256) {
      float p = T.p[j], s = 0.f;
      if (kState) s = T.s[j];
      optim_elem<K>(c, p, T.g[j], s);
      if (kState) T.s[j] = s;
      T.p[j] = p;
    }
    return;
  }
  constexpr int U = kAdamBlock / 1024;
  float4 p[U], g[U], s[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + 1024 * u + 4 * threadIdx.x;
    if (i + 3 < T.n) {
      p[u] = *reinterpret_cast<const float4*>(T.p + i);
      g[u] = *reinterpret_cast<const float4*>(T.g + i);
      if (kState) s[u] = *reinterpret_cast<const float4*>(T.s + i);
      else s[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + 1024 * u + 4 * threadIdx.x;
    if (i + 3 < T.n) {
      optim_elem<K>(c, p[u].x, g[u].x, s[u].x);
      optim_elem<K>(c, p[u].y, g[u].y, s[u].y);
      optim_elem<K>(c, p[u].z, g[u].z, s[u].z);
      optim_elem<K>(c, p[u].w, g[u].w, s[u].w);
      if (kState) *reinterpret_cast<float4*>(T.s + i) = s[u];
      *reinterpret_cast<float4*>(T.p + i) = p[u];
    } else {
      for (int k = 0; k < 4; ++k) {  // the last numel % 4 elements
        if (i + k >= T.n) break;
        float pp = T.p[i + k], ss = 0.f;
        if (kState) ss = T.s[i + k];
        optim_elem<K>(c, pp, T.g[i + k], ss);
        if (kState) T.s[i + k] = ss;
        T.p[i + k] = pp;
      }
    }
  }
}

// SCHED: the first wave evaluates the schedule at the step (lr_schedule_value, dfwfm_adam.h) and its lane 0 forms the
// scalars with that double in the place of a.h.lr; nothing else differs.
template <int K, bool SCHED>
__global__ void __launch_bounds__(256) optim_kernel(const OptimList list, const OptimArgs a) {
  __shared__ OptimCoef sc;
  __shared__ int64_t s_step;
  if constexpr (SCHED) {
    if (threadIdx.x < 64) {
      const int64_t step = a.st ? a.st->step + 1 : a.step;
      const double lr = lr_schedule_value(a.sched, step);
      if (threadIdx.x == 0) {
        s_step = step;
        sc = optim_coef(step, a.h, lr);
      }
    }
  } else {
    if (threadIdx.x == 0) {
      s_step = a.st ? a.st->step + 1 : a.step;
      sc = optim_coef(s_step, a.h, a.h.lr);
    }
  }
  __syncthreads();
  const OptimCoef c = sc;
  const int nwg = gridDim.x;
  for (int b = blockIdx.x; b < a.nblocks; b += nwg) optim_block<K>(list, c, b);
  if (a.bump && threadIdx.x == 0 && atomicAdd(&a.st->ticket, 1) == nwg - 1) optim_advance(a.st, c, s_step);
}

template <int K>
static hipError_t launch_optim_k(const OptimList& list, const OptimArgs& a, hipStream_t s) {
  const int total = a.nblocks < 1 ? 1 : a.nblocks;  // a call without tensors still advances the counter: one workgroup
  const int grid = total < kAdamGrid ? total : kAdamGrid;
  if (a.sched) hipLaunchKernelGGL((optim_kernel<K, true>), dim3(grid), dim3(256), 0, s, list, a);
  else hipLaunchKernelGGL((optim_kernel<K, false>), dim3(grid), dim3(256), 0, s, list, a);
  return hipGetLastError();
}

hipError_t launch_optim(int kind, const OptimList& list, const OptimArgs& a, hipStream_t s) {
  if (a.bump && !a.st) return hipErrorInvalidValue;
  switch (kind) {
    case kOptSgd: return launch_optim_k<kOptSgd>(list, a, s);
    case kOptSgdMom: return launch_optim_k<kOptSgdMom>(list, a, s);
    case kOptAdagrad: return launch_optim_k<kOptAdagrad>(list, a, s);
    case kOptRmsprop: return launch_optim_k<kOptRmsprop>(list, a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dfwfm
