// dfwfm_lazy_lists.h -- the launch arguments of the list-driven row-lazy steps
// (include/dfwfm_lazy_lists.h: the contract; dfwfm_lazy_lists.hip: the kernel).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_internal.h"
#include "dfwfm_optim.h"

namespace dfwfm {

constexpr int kListsAdam = 4;  // the kernel's kind beside OptimKind's four

// One table of a launch, 40 bytes: its rows are the floats [off, end) of the flat buffers.  The host has sorted the
// spans of a launch by `off` and checked that they do not overlap.
struct ListsSpan {
  float* p;
  int32_t* stamp;
  int64_t off, end;  // end = off + rows * width
  int32_t width;
  int32_t pad;
};
// One exchanged list of a launch, 32 bytes
struct ListsList {
  const int64_t* dest;
  const int32_t* count;
  int64_t cap;
  int32_t width;
  int32_t block0;  // first work block of the list (a block = 256 entries)
};
constexpr int kListsSpans = 64;  // DFWFM_LAZY_LISTS_SPANS_PER_LAUNCH
constexpr int kListsLists = 32;  // DFWFM_LAZY_LISTS_LISTS_PER_LAUNCH
struct ListsArgs {
  ListsSpan sp[kListsSpans];
  ListsList ls[kListsLists];
  float* g;
  float* m;  // Adam: exp_avg; another optimizer: its state array (null for kOptSgd)
  float* v;  // Adam: exp_avg_sq; else unused
  AdamDevState* st;
  const LrSchedule* sched;  // non-null: the rate is its value at the step, the hyper-parameters' lr unused
  AdamHyper ah;             // kListsAdam
  OptimHyper oh;            // the other kinds
  int32_t ns, nl, bump, nblocks;
};
static_assert(sizeof(ListsSpan) == 40 && sizeof(ListsList) == 32, "lazy lists launch entries");
static_assert(sizeof(ListsArgs) + 64 <= 4096, "lazy lists launch arguments over 4 KiB");

// one launch of `kind` (kListsAdam or an OptimKind) over a.nblocks work blocks of 256 list entries; with a.bump (the
// call's last launch) the last workgroup to finish advances the counter
hipError_t launch_lazy_lists(int kind, const ListsArgs& a, hipStream_t s);

}  // namespace dfwfm
