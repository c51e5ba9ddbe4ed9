// dfwfm_rowwise_lists.hip -- the row-wise Adagrad step of the categorical tables driven by exchanged touched-row
// lists (include_dp/dfwfm_rowwise_lists.h: the contract).
//
// Two kernels joined.  The claim is lazy_lists_kernel's (dfwfm_lazy_lists.hip): a work block is 256 entries of ONE
// list, one lane per entry; blocks behind the list's count leave at once.  The lane reads its destination and finds
// the span that holds it by a search over the launch's spans, which every workgroup stages once in LDS (the search
// index differs per lane, and the kernel arguments are indexed with workgroup-uniform indices only).  A destination in
// no span of the list's width, or between two rows, is dropped before any address is formed.  Destinations are unique
// within a list, so every lane claims for itself: a device-scope look at the row's stamp and, unless it already holds
// this step's stamp, an atomic exchange -- whoever reads back another value is the first of this step and owns the row.
// The update is rowwise_adagrad_kernel's (dfwfm_rowwise_adagrad.hip), by the very same two functions
// (dfwfm_rowwise_adagrad.h): at width 1 the owning lane does the row alone; else the wave's owned rows are compacted
// through LDS and each taken by kLazyGroup = 16 lanes, which run the row's sequential chain by in-group shuffles.  What
// the compaction carries per row is the destination, the row's parameter pointer and its accumulator's pointer: the
// gradient lives in the flat buffer at the destination, the accumulator in the span's own array at the row.
// A bounded grid walks the work blocks; every workgroup reads the step counter first and the last one to finish in the
// call's last launch advances it (the dense kernels' ticket).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_adam.h"
#include "dfwfm_internal.h"
#include "dfwfm_rowwise_adagrad.h"
#include "dfwfm_rowwise_lists.h"

namespace dfwfm {

// the step's stamp, the lazy kernels' scheme: (step - 1) mod (2^32 - 1) + 1, never 0 (stamps start zero-filled)
__device__ __forceinline__ int32_t rowwise_lists_stamp(int64_t step) {
  return (int32_t)(uint32_t)((uint64_t)(step - 1) % 0xffffffffull + 1ull);
}

// SCHED: the first wave evaluates the schedule at the step (lr_schedule_value, dfwfm_adam.h) and its lane 0 forms the
// scalars with that double in the place of a.oh.lr; nothing else differs.
template <bool SCHED>
__global__ void __launch_bounds__(256) rowwise_lists_kernel(const RowListsArgs a) {
  __shared__ OptimCoef s_oc;
  __shared__ int64_t s_step;
  __shared__ RowListsSpan s_sp[kRowListsSpans];
  __shared__ float* s_prow[4][64];   // per wave: the rows it owns, compacted (their parameters' first elements, ...
  __shared__ float* s_acc[4][64];    // ... their accumulators ...
  __shared__ int64_t s_dest[4][64];  // ... and their destinations in the flat gradient buffer)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < 64) {
    const int64_t step = a.st->step + 1;
    double lr = a.oh.lr;
    if constexpr (SCHED) lr = lr_schedule_value(a.sched, step);
    if (threadIdx.x == 0) {
      s_step = step;
      s_oc = optim_coef(step, a.oh, lr);
    }
  }
  // the spans into LDS: a wave-uniform index into the kernel arguments, one lane writes
  for (int i = wave; i < a.ns; i += 4) {
    const RowListsSpan x = a.sp[i];
    if (lane == 0) s_sp[i] = x;
  }
  __syncthreads();
  const OptimCoef c = s_oc;
  const int32_t stamp = rowwise_lists_stamp(s_step);
  for (int b = blockIdx.x; b < a.nblocks; b += gridDim.x) {
    int lo = 0, hi = a.nl - 1;
    while (lo < hi) {  // last list whose block0 <= b
      const int mid = (lo + hi + 1) >> 1;
      if (a.ls[mid].block0 <= b) lo = mid;
      else hi = mid - 1;
    }
    const ListsList T = a.ls[lo];
    int64_t n = *T.count;  // every reader stops at min(count, cap)
    n = n < 0 ? 0 : (n < T.cap ? n : T.cap);
    const int64_t e0 = (int64_t)(b - T.block0) * 256;
    if (e0 >= n) continue;  // (uniform over the workgroup)
    const int64_t e = e0 + threadIdx.x;
    bool mine = false;
    float* prow = nullptr;
    float* pacc = nullptr;
    int64_t d = 0;
    if (e < n && a.ns > 0) {
      d = T.dest[e];
      int slo = 0, shi = a.ns - 1;
      while (slo < shi) {  // last span whose off <= d
        const int mid = (slo + shi + 1) >> 1;
        if (s_sp[mid].off <= d) slo = mid;
        else shi = mid - 1;
      }
      const int64_t off = s_sp[slo].off;
      const int w = s_sp[slo].width;
      if (d >= off && d < s_sp[slo].end && w == T.width) {
        const int64_t rel = d - off;
        const int64_t row = rel <= 0xffffffffll ? (int64_t)((uint32_t)rel / (uint32_t)w) : rel / w;
        if (row * w == rel) {  // a row's first element
          int32_t* sp = s_sp[slo].stamp + row;
          // (the look is a device-scope load: a stale "not yet claimed" only costs the exchange it would have saved)
          mine = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != stamp &&
                 atomicExch(sp, stamp) != stamp;
          prow = s_sp[slo].p + rel;
          pacc = s_sp[slo].s + row;
        }
      }
    }
    if (T.width == 1) {
      if (mine) rowwise_update_one(c, prow, a.g + d, pacc);
      continue;  // (T is uniform over the workgroup)
    }
    const unsigned long long own = __ballot(mine);
    if (mine) {
      const int slot = __popcll(own & ((1ull << lane) - 1ull));
      s_prow[wave][slot] = prow;
      s_acc[wave][slot] = pacc;
      s_dest[wave][slot] = d;
    }
    __syncthreads();
    const int cnt = __popcll(own);
    // (a group's lanes share k, so they enter and leave this loop together: the group's shuffles see all 16 of them)
    for (int k = lane / kLazyGroup; k < cnt; k += 64 / kLazyGroup)
      rowwise_update_group(c, s_prow[wave][k], a.g + s_dest[wave][k], s_acc[wave][k], T.width, lane % kLazyGroup);
    __syncthreads();  // the compacted rows are rewritten by the next work block
  }
  if (a.bump && threadIdx.x == 0 && atomicAdd(&a.st->ticket, 1) == (int)gridDim.x - 1) optim_advance(a.st, c, s_step);
}

hipError_t launch_rowwise_lists(const RowListsArgs& a, hipStream_t s) {
  if (!a.st) return hipErrorInvalidValue;
  const int total = a.nblocks < 1 ? 1 : a.nblocks;  // an empty call still advances the counter: one workgroup
  const int grid = total < kAdamGrid ? total : kAdamGrid;
  if (a.sched) hipLaunchKernelGGL((rowwise_lists_kernel<true>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rowwise_lists_kernel<false>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dfwfm
