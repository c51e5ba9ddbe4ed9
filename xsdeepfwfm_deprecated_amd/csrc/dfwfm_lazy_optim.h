// dfwfm_lazy_optim.h -- the launch arguments of the row-lazy SGD / Adagrad / RMSprop step
// (include/dfwfm_lazy_optim.h: the contract; dfwfm_lazy_optim.hip: the kernel).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_internal.h"
#include "dfwfm_optim.h"

namespace dfwfm {

// One table of a launch: LazyTable (dfwfm_internal.h) with one state array, 64 bytes.  The host has checked that every
// key of [0, key_range) maps to a row of the table, so the kernel indexes without a row count.
struct LazyOptimTable {
  float* p;
  float* g;
  float* s;  // null for kOptSgd
  int32_t* stamp;
  int64_t key_range;
  int64_t c;
  int32_t width, column, kind;
  int32_t block0;  // first work block of the table (a block = 256 samples)
};
constexpr int kLazyOptimList = 60;  // tables per launch (the list is a kernel argument, < 4 KiB with LazyOptimArgs)
struct LazyOptimList {
  LazyOptimTable t[kLazyOptimList];
  int32_t n;
  int32_t pad;
};
struct LazyOptimArgs {
  const int64_t* xi;
  int64_t xi_stride, batch;
  AdamDevState* st;
  const LrSchedule* sched;  // non-null: the rate is its value at the step, h.lr unused
  OptimHyper h;
  int32_t bump, nblocks;
};
static_assert(sizeof(LazyOptimTable) == 64, "lazy optim table entry");
static_assert(sizeof(LazyOptimList) + sizeof(LazyOptimArgs) + 64 <= 4096, "lazy optim launch arguments over 4 KiB");

// one launch of `kind` (OptimKind) over the list's nblocks work blocks of 256 samples (lazy_blocks, dfwfm_internal.h);
// with `bump` (the call's last launch) the last workgroup to finish advances the counter
hipError_t launch_lazy_optim(int kind, const LazyOptimList& list, const LazyOptimArgs& a, hipStream_t s);

}  // namespace dfwfm
