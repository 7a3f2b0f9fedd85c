// refit_launch.h -- host only: the protocol of an in-place refit call, stated once for the six entry points that keep a small table on
// the device between calls (tlas_refit_, tlas_wide_refit_, tlas_motion_refit_, tlas_wide_motion_refit_, bvh_refit_batch_,
// wide_refit_batch_kernels.hip).  A unit keeps its argument checks, the construction of its table, its ScratchCarver layout, its kernels and the
// filling of its result; what is here is the held-table rule, the bracket of the blocking form and the fold of the counter slots.
//   the held table   the device keeps the table of the last uncaptured call in the unit's scratch pool, and the host keeps a copy to
//                    compare the next call's table with: a frame loop over one pool uploads once.  A copy on the host never vouches for
//                    bytes that are gone: the record is invalid as soon as the pool was released or has to grow
//   a captured call  reads nothing back, uploads nothing and allocates nothing, so it is refused unless the device holds this very table
//                    (and, for the top-level refits, was last used at this very shape: the slices behind the table move with it)
//   the bracket      no host read-back unless a result is asked for, and no memset node on the asynchronous path: a unit's first launch
//                    re-initialises the arrival counters, and the counters of the blocking form, which is never captured, are the one memset
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ntr_internal.h"
#include "device_scratch.h"

namespace ntr {

// Counters of the blocking form: a workgroup adds to the slot of its number modulo kRefitStatSlots (a unit's *Stats struct, one 64-byte
// line each) and the host folds the slots.
constexpr int kRefitStatSlots = 256;

// The table a call brings, as one or two blobs of words in the order they are uploaded, with the blobs' offsets in the unit's layout,
// and the shape that a capture must match beyond the table (0 where a unit has none).
struct RefitTable {
    int numBlobs;
    std::vector<uint32_t> words[2];
    size_t offset[2];
    int shape[2];
};

// What the device's table holds, one per device: the blobs the last call uploaded and the shape of the last uncaptured call.
struct RefitHeld {
    bool valid = false;
    int shape[2] = {0, 0};
    std::vector<uint32_t> words[2];
};

// The unit's words in the refusal of a captured call whose table the device does not hold: "this <table> table", "the same <same>",
// "none with <others>"
struct RefitWords { const char *table, *same, *others; };
constexpr RefitWords kRefitRangeWords = {"range", "ranges and instance count", "others"};
constexpr RefitWords kRefitRangeExtentWords = {"range", "ranges, instance count and extent", "others"};
constexpr RefitWords kRefitEntryWords = {"entry", "entries", "other entries"};

// Makes the device hold table `t` in `pool`, whose block of layoutEnd bytes is returned in *base.  t's blobs are swapped into the
// record when they are uploaded.
inline int refit_hold_table(const char* fn, const RefitWords& w, DeviceScratchPool& pool, RefitHeld (&held)[kMaxDevices], hipStream_t s,
                            bool wantsResult, size_t layoutEnd, RefitTable& t, void** base)
{
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
    RefitHeld& up = held[dev];
    if (pool.held() < layoutEnd) up.valid = false;   // released, never reserved, or about to be regrown
    const bool same = up.valid && up.words[0] == t.words[0] && up.words[1] == t.words[1];
    const bool capturing = stream_is_capturing(s);
    if (capturing && wantsResult) return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);
    if (capturing && !(same && up.shape[0] == t.shape[0] && up.shape[1] == t.shape[1]))
        return set_error(NTR_ERR_INVALID, "%s: a captured call uploads and allocates nothing: the device must hold this %s table already "
                         "-- make one uncaptured call with the same %s first (and none with %s, and no "
                         "ntr_lbvh_release_workspace, between it and the capture)", fn, w.table, w.same, w.others);
    if (const int rc = pool.reserve(layoutEnd, base)) return rc;
    if (!same) {
        // the host copy is what the upload reads and what the next call compares with: the upload is waited for, so the copy never
        // changes under it.  A loop of calls with one table (a frame loop) pays this once
        up.valid = false;
        for (int b = 0; b < t.numBlobs; b++) up.words[b].swap(t.words[b]);
        for (int b = 0; b < t.numBlobs; b++)
            NTR_HIP(hipMemcpyAsync((char*)*base + t.offset[b], up.words[b].data(), up.words[b].size() * 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipStreamSynchronize(s));
        up.valid = true;
    }
    if (!capturing) { up.shape[0] = t.shape[0]; up.shape[1] = t.shape[1]; }
    return NTR_OK;
}

// The launches of one call.  blocking: they lie between two events, the unit's zeroed block (zeroBytes at `zeroed`: its counters and
// whatever lies with them) is cleared before them and copied to *host after them, the copy is waited for and *seconds receives the
// events' distance.  Otherwise only the launches, and nothing is waited for.
template <class Launches>
int refit_bracket(hipStream_t s, bool blocking, void* zeroed, size_t zeroBytes, std::vector<char>* host, float* seconds, Launches&& launches)
{
    StreamEvents<2> ev(s);
    if (blocking) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
        NTR_HIP(hipMemsetAsync(zeroed, 0, zeroBytes, s));
    }
    launches();
    NTR_HIP(hipGetLastError());
    if (!blocking) return NTR_OK;

    NTR_HIP(ev.record(1));
    *host = std::vector<char>(zeroBytes);        // the copy is waited for right here
    NTR_HIP(hipMemcpyAsync(host->data(), zeroed, zeroBytes, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    *seconds = ms * 1e-3f;
    return NTR_OK;
}

// slot(const Stats&) for each of the counter slots that lie at `slots` in the block the bracket read back
template <class Stats, class Slot>
void refit_fold_slots(const char* slots, Slot&& slot)
{
    static_assert(sizeof(Stats) == 64, "a slot per 64-byte line");
    const Stats* hs = (const Stats*)slots;
    for (int k = 0; k < kRefitStatSlots; k++) slot(hs[k]);
}

}  // namespace ntr
