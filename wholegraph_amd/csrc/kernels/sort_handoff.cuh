// wholegraph_amd — all that the optimizer step (optim.hip) knows of the owner-side id sort (dedup.hip): the control words of a
// split sort that the step's kernels read, and four calls. The state behind the calls (the sort's side-stream lane, the record
// of the thread's last split sort, the pending deferred join) has one owner, dedup.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

namespace wm {
namespace split {
constexpr int kMaxDup = 8;   // runs of more ids than this send their bucket to the radix passes (split_sort.cuh)
// control words (u32), zeroed by split_hist_kernel's first workgroup
// [kCtlLongCounters, +16): the counters of the optimizer step's long-run side (optim.hip), zeroed here with the rest so that
// the step needs no fill of its own when it follows a split sort
// kCtlGenericDone: set by the generic path's closing kernel (dedup.hip: detect_runs)
// kCtlScanCount: workgroups of split_scan_kernel that have finished (the last one publishes the caller's verdict word)
// kCtlSortDone: set by split_join_kernel — the runs are final (whichever path wrote them); side-stream work that needs them
// waits for this word instead of an event on the caller's stream (optim.hip: the detached long-run side)
enum { kCtlOverflow = 0, kCtlTicket = 1, kCtlError = 2, kCtlRadixBuckets = 3, kCtlGenericDone = 4, kCtlSortDone = 5, kCtlScanCount = 6, kCtlLongCounters = 16, kCtlWords = 32 };
// a bit of the device error word beside the sort's own (split_sort.cuh: kErrLookBack ... kErrOnesweep = 1 ... 8): the tree fold's
// listing kernel met a run that did not fit the workspace it was handed (optim.hip: tree_mark_kernel)
constexpr unsigned kErrTreeBounds = 16u;
}  // namespace split

// The control words of this thread's last id sort if that was a split sort which wrote exactly these three arrays, else nullptr.
// Clears the record either way: one step per sort.
uint32_t* take_split_ctl(const int32_t* run_starts, const void* unique_ids, const int64_t* n_unique);
// A deferred join of this thread is pending and the device's sort lane is usable: the lane's mutex, locked, and its side stream
// in *side. Otherwise a lock that owns nothing, *side untouched.
std::unique_lock<std::mutex> lock_pending_join_side(hipStream_t* side);
// records the sort lane's `joined` event, the one a deferred join (hip_dedup_join) waits for, on `stream`
hipError_t record_sort_joined(hipStream_t stream);
// one wave on `stream` that waits for ctl[kCtlSortDone] == 1, "the runs are final" (split_sort.cuh: split_wait_kernel)
void enqueue_final_runs_wait(const uint32_t* ctl, hipStream_t stream);
// the device's error word as kernels address it (pinned host memory; hip_device_error reports and clears it), or nullptr
uint32_t* device_error_word();
}  // namespace wm
