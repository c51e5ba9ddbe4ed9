// dfwfm_lazy_lists.hip -- the row-lazy Adam / SGD / Adagrad / RMSprop step of the categorical tables driven by exchanged
// touched-row lists (include/dfwfm_lazy_lists.h: the contract).
//
// The shape is the key-driven lazy kernels' (dfwfm_lazy_adam.hip, dfwfm_lazy_optim.hip) with the lists in the place of
// the keys.  A work block is 256 entries of ONE list, one lane per entry; blocks behind the list's count leave at once
// (a list's capacity is several times its count).  The lane reads its destination and finds the span that holds it by
// a search over the launch's spans, which every workgroup stages once in LDS (the search index differs per lane, and
// the kernel arguments are indexed with workgroup-uniform indices only).  A destination in no span of the list's
// width, or between two rows, is dropped before any address is formed.  Claim: destinations are unique within a list,
// so the lanes of a workgroup hold distinct rows and every lane claims for itself; the lists of other ranks sit in
// other work blocks, and a row several of them name is decided by the stamp -- a device-scope look and, unless the row
// already holds this step's stamp, an atomic exchange: whoever reads back another value is the first of this step and
// owns the row.  Update: adam_elem (dfwfm_adam.h) or optim_elem<K> (dfwfm_optim.h, contraction off inside it), the
// dense kernels' own arithmetic, on each element, then the gradient element is zeroed -- by the owning lane itself at
// width 1, else the wave's owned rows are compacted through LDS and each taken by kLazyGroup = 16 lanes.
// A bounded grid walks the work blocks; every workgroup reads the step counter first and the last one to finish in the
// call's last launch advances it (the dense kernels' ticket).  One template over the kind and the schedule: plain SGD
// never forms an address from its (null) state pointer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_adam.h"
#include "dfwfm_internal.h"
#include "dfwfm_lazy_lists.h"
#include "dfwfm_optim.h"

namespace dfwfm {

// the step's stamp, the lazy Adam's scheme: (step - 1) mod (2^32 - 1) + 1, never 0 (stamps start zero-filled)
__device__ __forceinline__ int32_t lazy_lists_stamp(int64_t step) {
  return (int32_t)(uint32_t)((uint64_t)(step - 1) % 0xffffffffull + 1ull);
}

// one element of an owned row (pe: its parameter, j: its index in the flat buffers): the dense kernels' function,
// then the gradient's zero
template <int K>
__device__ __forceinline__ void lazy_lists_update(const AdamCoef& ac, const OptimCoef& oc, const ListsArgs& a,
                                                  float* __restrict__ pe, int64_t j) {
  if constexpr (K == kListsAdam) {
    float p = *pe, m = a.m[j], v = a.v[j];
    adam_elem(ac, p, a.g[j], m, v);
    a.m[j] = m;
    a.v[j] = v;
    *pe = p;
    a.g[j] = 0.f;
  } else {
    constexpr bool kState = K != kOptSgd;
    float p = *pe, s = 0.f;
    if (kState) s = a.m[j];
    optim_elem<K>(oc, p, a.g[j], s);
    if (kState) a.m[j] = s;
    *pe = p;
    a.g[j] = 0.f;
  }
}

// SCHED: the first wave evaluates the schedule at the step (lr_schedule_value, dfwfm_adam.h) and its lane 0 forms the
// scalars with that double in the place of the hyper-parameters' lr; nothing else differs.
template <int K, bool SCHED>
__global__ void __launch_bounds__(256) lazy_lists_kernel(const ListsArgs a) {
  constexpr bool kAdam = K == kListsAdam;
  __shared__ AdamCoef s_ac;
  __shared__ OptimCoef s_oc;
  __shared__ int64_t s_step;
  __shared__ ListsSpan s_sp[kListsSpans];
  __shared__ float* s_prow[4][64];  // per wave: the rows it owns, compacted (their parameters' first elements ...
  __shared__ int64_t s_dest[4][64];  // ... and their destinations in the flat buffers)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < 64) {
    const int64_t step = a.st->step + 1;
    double lr = kAdam ? a.ah.lr : a.oh.lr;
    if constexpr (SCHED) lr = lr_schedule_value(a.sched, step);
    if (threadIdx.x == 0) {
      s_step = step;
      if constexpr (kAdam) s_ac = adam_coef(step, AdamHyper{lr, a.ah.b1, a.ah.b2, a.ah.eps, a.ah.wd});
      else s_oc = optim_coef(step, a.oh, lr);
    }
  }
  // the spans into LDS: a wave-uniform index into the kernel arguments, one lane writes
  for (int i = wave; i < a.ns; i += 4) {
    const ListsSpan x = a.sp[i];
    if (lane == 0) s_sp[i] = x;
  }
  __syncthreads();
  AdamCoef ac = {};
  OptimCoef oc = {};
  if constexpr (kAdam) ac = s_ac;
  else oc = s_oc;
  const int32_t stamp = lazy_lists_stamp(s_step);
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
        }
      }
    }
    if (T.width == 1) {
      if (mine) lazy_lists_update<K>(ac, oc, a, prow, d);
      continue;  // (T is uniform over the workgroup)
    }
    const unsigned long long own = __ballot(mine);
    if (mine) {
      const int slot = __popcll(own & ((1ull << lane) - 1ull));
      s_prow[wave][slot] = prow;
      s_dest[wave][slot] = d;
    }
    __syncthreads();
    const int cnt = __popcll(own);
    for (int k = lane / kLazyGroup; k < cnt; k += 64 / kLazyGroup) {
      float* p0 = s_prow[wave][k];
      const int64_t d0 = s_dest[wave][k];
      for (int el = lane % kLazyGroup; el < T.width; el += kLazyGroup) lazy_lists_update<K>(ac, oc, a, p0 + el, d0 + el);
    }
    __syncthreads();  // s_prow / s_dest are rewritten by the next work block
  }
  if (a.bump && threadIdx.x == 0 && atomicAdd(&a.st->ticket, 1) == (int)gridDim.x - 1) {
    if constexpr (kAdam) adam_advance(a.st, ac, s_step);
    else optim_advance(a.st, oc, s_step);
  }
}

template <int K>
static hipError_t launch_lazy_lists_k(const ListsArgs& a, hipStream_t s) {
  const int total = a.nblocks < 1 ? 1 : a.nblocks;  // an empty call still advances the counter: one workgroup
  const int grid = total < kAdamGrid ? total : kAdamGrid;
  if (a.sched) hipLaunchKernelGGL((lazy_lists_kernel<K, true>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((lazy_lists_kernel<K, false>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lazy_lists(int kind, const ListsArgs& a, hipStream_t s) {
  if (!a.st) return hipErrorInvalidValue;
  switch (kind) {
    case kListsAdam: return launch_lazy_lists_k<kListsAdam>(a, s);
    case kOptSgd: return launch_lazy_lists_k<kOptSgd>(a, s);
    case kOptSgdMom: return launch_lazy_lists_k<kOptSgdMom>(a, s);
    case kOptAdagrad: return launch_lazy_lists_k<kOptAdagrad>(a, s);
    case kOptRmsprop: return launch_lazy_lists_k<kOptRmsprop>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dfwfm
