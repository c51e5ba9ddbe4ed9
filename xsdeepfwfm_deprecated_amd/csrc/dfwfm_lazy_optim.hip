// dfwfm_lazy_optim.hip -- the row-lazy SGD / Adagrad / RMSprop step of the categorical tables
// (include/dfwfm_lazy_optim.h: the contract).
//
// The shape is the lazy Adam's (dfwfm_lazy_adam.hip).  A work block is 256 samples of ONE table, one lane per
// (table, sample).  The lane reads its sample's key and maps it to the table's row.  Claim: the lanes of a wave that
// hold the same row elect one of them (up to kLazyRounds distinct rows per wave by ballot; a Criteo batch hits the few
// rows of a small table thousands of times, and that many exchanges on one address serialise); the elected lane looks
// at stamp[row] and, unless it already holds this step's stamp, claims the row by an atomic exchange of the stamp:
// whoever reads back another value is the first of this step and owns the row.  Update: optim_elem<K> (dfwfm_optim.h,
// the dense kernels' own arithmetic, contraction off inside it) on each element, then the gradient element is zeroed --
// by the owning lane itself at width 1, else the wave's owned rows are compacted through LDS and each taken by
// kLazyGroup = 16 lanes (D = 4..32: at most two elements per lane).  A row touched by many samples is updated once,
// and since rows are independent it does not matter by whom.
// A bounded grid walks the work blocks; every workgroup reads the step counter first and the last one to finish in the
// call's last launch advances it (the dense kernels' ticket).  One template over the kind and the schedule: plain SGD
// never forms an address from its (null) state pointer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_adam.h"
#include "dfwfm_internal.h"
#include "dfwfm_lazy_optim.h"
#include "dfwfm_optim.h"
#include "../../include/dfwfm_lazy_adam.h"

namespace dfwfm {

// the step's stamp, the lazy Adam's scheme: (step - 1) mod (2^32 - 1) + 1, never 0 (stamps start zero-filled)
__device__ __forceinline__ int32_t lazy_optim_stamp(int64_t step) {
  return (int32_t)(uint32_t)((uint64_t)(step - 1) % 0xffffffffull + 1ull);
}

// one element of an owned row: the dense kernels' function, then the gradient's zero
template <int K>
__device__ __forceinline__ void lazy_optim_update(const OptimCoef& c, const LazyOptimTable& T, int64_t j) {
  constexpr bool kState = K != kOptSgd;
  float p = T.p[j], s = 0.f;
  if (kState) s = T.s[j];
  optim_elem<K>(c, p, T.g[j], s);
  if (kState) T.s[j] = s;
  T.p[j] = p;
  T.g[j] = 0.f;
}

// SCHED: the first wave evaluates the schedule at the step (lr_schedule_value, dfwfm_adam.h) and its lane 0 forms the
// scalars with that double in the place of a.h.lr; nothing else differs.
template <int K, bool SCHED>
__global__ void __launch_bounds__(256) lazy_optim_kernel(const LazyOptimList list, const LazyOptimArgs a) {
  __shared__ OptimCoef sc;
  __shared__ int64_t s_step;
  if constexpr (SCHED) {
    if (threadIdx.x < 64) {
      const int64_t step = a.st->step + 1;
      const double lr = lr_schedule_value(a.sched, step);
      if (threadIdx.x == 0) {
        s_step = step;
        sc = optim_coef(step, a.h, lr);
      }
    }
  } else {
    if (threadIdx.x == 0) {
      s_step = a.st->step + 1;
      sc = optim_coef(s_step, a.h, a.h.lr);
    }
  }
  __syncthreads();
  const OptimCoef c = sc;
  const int32_t stamp = lazy_optim_stamp(s_step);
  __shared__ int64_t s_rows[4][64];  // per wave: the rows it owns, compacted (tables wider than one float)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = blockIdx.x; b < a.nblocks; b += gridDim.x) {
    int lo = 0, hi = list.n - 1;
    while (lo < hi) {  // last table whose block0 <= b
      const int mid = (lo + hi + 1) >> 1;
      if (list.t[mid].block0 <= b) lo = mid;
      else hi = mid - 1;
    }
    const LazyOptimTable T = list.t[lo];
    const int64_t i = (int64_t)(b - T.block0) * 256 + threadIdx.x;
    int64_t row = -1;
    if (i < a.batch) {
      int64_t key = a.xi[i * a.xi_stride + T.column];
      if (key < 0 || key >= T.key_range) key = 0;  // the forwards' and the scatter's clamp
      row = T.kind == DFWFM_LAZY_QUOTIENT ? key / T.c : (T.kind == DFWFM_LAZY_REMAINDER ? key % T.c : key);
    }
    // one claimant per distinct row of the wave (the first kLazyRounds distinct rows; the rest claim for themselves)
    bool pending = row >= 0, claimant = false;
    for (int it = 0; it < kLazyRounds; ++it) {
      const unsigned long long todo = __ballot(pending);
      if (!todo) break;  // (wave-uniform)
      const int first = __ffsll(todo) - 1;
      const int64_t r = __shfl(row, first);
      if (pending && row == r) {
        pending = false;
        claimant = lane == first;
      }
    }
    claimant = claimant || pending;
    // (the look is a device-scope load: a stale "not yet claimed" only costs the exchange it would have saved)
    const bool mine = claimant &&
                      __hip_atomic_load(T.stamp + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != stamp &&
                      atomicExch(T.stamp + row, stamp) != stamp;
    if (T.width == 1) {
      if (mine) lazy_optim_update<K>(c, T, row);
      continue;  // (T is uniform over the workgroup)
    }
    const unsigned long long own = __ballot(mine);
    if (mine) s_rows[wave][__popcll(own & ((1ull << lane) - 1ull))] = row;
    __syncthreads();
    const int n = __popcll(own);
    for (int k = lane / kLazyGroup; k < n; k += 64 / kLazyGroup) {
      const int64_t r0 = s_rows[wave][k] * T.width;
      for (int e = lane % kLazyGroup; e < T.width; e += kLazyGroup) lazy_optim_update<K>(c, T, r0 + e);
    }
    __syncthreads();  // s_rows is rewritten by the next work block
  }
  if (a.bump && threadIdx.x == 0 && atomicAdd(&a.st->ticket, 1) == (int)gridDim.x - 1) optim_advance(a.st, c, s_step);
}

template <int K>
static hipError_t launch_lazy_optim_k(const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s) {
  const int total = a.nblocks < 1 ? 1 : a.nblocks;  // an empty call still advances the counter: one workgroup
  const int grid = total < kAdamGrid ? total : kAdamGrid;
  if (a.sched) hipLaunchKernelGGL((lazy_optim_kernel<K, true>), dim3(grid), dim3(256), 0, s, list, a);
  else hipLaunchKernelGGL((lazy_optim_kernel<K, false>), dim3(grid), dim3(256), 0, s, list, a);
  return hipGetLastError();
}

hipError_t launch_lazy_optim(int kind, const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s) {
  if (!a.st) return hipErrorInvalidValue;
  switch (kind) {
    case kOptSgd: return launch_lazy_optim_k<kOptSgd>(list, a, s);
    case kOptSgdMom: return launch_lazy_optim_k<kOptSgdMom>(list, a, s);
    case kOptAdagrad: return launch_lazy_optim_k<kOptAdagrad>(list, a, s);
    case kOptRmsprop: return launch_lazy_optim_k<kOptRmsprop>(list, a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dfwfm
