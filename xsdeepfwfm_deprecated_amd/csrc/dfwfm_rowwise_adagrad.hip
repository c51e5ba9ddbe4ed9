// dfwfm_rowwise_adagrad.hip -- the row-wise Adagrad step of the categorical tables
// (include/dfwfm_rowwise_adagrad.h: the contract).
//
// The shape is the row-lazy kernels' (dfwfm_lazy_optim.hip).  A work block is 256 samples of ONE table, one lane per
// (table, sample).  The lane reads its sample's key and maps it to the table's row.  Claim: the lanes of a wave that
// hold the same row elect one of them (up to kLazyRounds distinct rows per wave by ballot); the elected lane looks at
// stamp[row] and, unless it already holds this step's stamp, claims the row by an atomic exchange of the stamp:
// whoever reads back another value is the first of this step and owns the row.  Only an owned row's number ever
// becomes an address.
// Update: what is new here is a reduction ACROSS the row, ss = the chain of fmaf(g', g', ss) in element order, which
// the contract fixes as sequential.  At width 1 the owning lane does the row alone.  Else the wave's owned rows are
// compacted through LDS and each taken by kLazyGroup = 16 lanes: lane l loads elements l, l + 16, ... and forms their
// g'; 16 elements at a time, every lane of the group reads the group's g' by lane shuffles in element order and runs
// the same chain, so that all 16 lanes end with the same ss -- no LDS round trip and no second order of summation.
// Every lane then forms the row's std from the one accumulator (lane 0 of the group stores it) and lane l updates
// its elements: the first two from registers (all of a row up to 32 wide), the rest re-read -- the same bits, since
// an element of p and g is written only there, by the lane that re-reads it.
// A bounded grid walks the work blocks; every workgroup reads the step counter first and the last one to finish in the
// call's last launch advances it (the dense kernels' ticket).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_adam.h"
#include "dfwfm_internal.h"
#include "dfwfm_rowwise_adagrad.h"
#include "../../include/dfwfm_lazy_adam.h"

namespace dfwfm {

// the step's stamp, the lazy kernels' scheme: (step - 1) mod (2^32 - 1) + 1, never 0 (stamps start zero-filled)
__device__ __forceinline__ int32_t rowwise_stamp(int64_t step) {
  return (int32_t)(uint32_t)((uint64_t)(step - 1) % 0xffffffffull + 1ull);
}

// (the two row functions, rowwise_update_one and rowwise_update_group, live in dfwfm_rowwise_adagrad.h: the
// list-driven kernel calls the same ones)

// SCHED: the first wave evaluates the schedule at the step (lr_schedule_value, dfwfm_adam.h) and its lane 0 forms the
// scalars with that double in the place of a.h.lr; nothing else differs.
template <bool SCHED>
__global__ void __launch_bounds__(256) rowwise_adagrad_kernel(const LazyOptimList list, const LazyOptimArgs a) {
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
  const int32_t stamp = rowwise_stamp(s_step);
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
      if (mine) rowwise_update_one(c, T.p + row, T.g + row, T.s + row);
      continue;  // (T is uniform over the workgroup)
    }
    const unsigned long long own = __ballot(mine);
    if (mine) s_rows[wave][__popcll(own & ((1ull << lane) - 1ull))] = row;
    __syncthreads();
    const int n = __popcll(own);
    // (a group's lanes share k, so they enter and leave this loop together: the group's shuffles see all 16 of them)
    for (int k = lane / kLazyGroup; k < n; k += 64 / kLazyGroup) {
      const int64_t r = s_rows[wave][k];
      rowwise_update_group(c, T.p + r * T.width, T.g + r * T.width, T.s + r, T.width, lane % kLazyGroup);
    }
    __syncthreads();  // s_rows is rewritten by the next work block
  }
  if (a.bump && threadIdx.x == 0 && atomicAdd(&a.st->ticket, 1) == (int)gridDim.x - 1) optim_advance(a.st, c, s_step);
}

hipError_t launch_rowwise_adagrad(const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s) {
  if (!a.st) return hipErrorInvalidValue;
  const int total = a.nblocks < 1 ? 1 : a.nblocks;  // an empty call still advances the counter: one workgroup
  const int grid = total < kAdamGrid ? total : kAdamGrid;
  if (a.sched) hipLaunchKernelGGL((rowwise_adagrad_kernel<true>), dim3(grid), dim3(256), 0, s, list, a);
  else hipLaunchKernelGGL((rowwise_adagrad_kernel<false>), dim3(grid), dim3(256), 0, s, list, a);
  return hipGetLastError();
}

}  // namespace dfwfm
