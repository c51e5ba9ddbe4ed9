// dfwfm_rowwise_lists.h -- the launch arguments of the list-driven row-wise Adagrad step
// (include_dp/dfwfm_rowwise_lists.h: the contract; dfwfm_rowwise_lists.hip: the kernel).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_internal.h"
#include "dfwfm_lazy_lists.h"
#include "dfwfm_optim.h"

namespace dfwfm {

// One table of a launch, 48 bytes: ListsSpan (dfwfm_lazy_lists.h) with the table's accumulators, one float per row.
// [off, end) are floats of the flat GRADIENT buffer only.  The host has sorted the spans of a launch by `off` and
// checked that they do not overlap.
struct RowListsSpan {
  float* p;
  float* s;  // [rows]
  int32_t* stamp;
  int64_t off, end;  // end = off + rows * width
  int32_t width;
  int32_t pad;
};
constexpr int kRowListsSpans = 60;  // DFWFM_ROWWISE_LISTS_SPANS_PER_LAUNCH
constexpr int kRowListsLists = 24;  // DFWFM_ROWWISE_LISTS_LISTS_PER_LAUNCH
// ListsArgs without the Adam fields and the flat state arrays: 60 * 48 + 24 * 32 bytes of descriptors
struct RowListsArgs {
  RowListsSpan sp[kRowListsSpans];
  ListsList ls[kRowListsLists];
  float* g;
  AdamDevState* st;
  const LrSchedule* sched;  // non-null: the rate is its value at the step, oh.lr unused
  OptimHyper oh;            // lr, wd and eps are read
  int32_t ns, nl, bump, nblocks;
};
static_assert(sizeof(RowListsSpan) == 48, "row-wise lists launch entries");
static_assert(sizeof(RowListsArgs) + 64 <= 4096, "row-wise lists launch arguments over 4 KiB");

// one launch over a.nblocks work blocks of 256 list entries; with a.bump (the call's last launch) the last workgroup
// to finish advances the counter
hipError_t launch_rowwise_lists(const RowListsArgs& a, hipStream_t s);

}  // namespace dfwfm
