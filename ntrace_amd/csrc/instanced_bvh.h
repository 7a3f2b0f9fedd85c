// instanced_bvh.h -- the two-level layout, stated once, for the code that builds a top-level tree (tlas_build_kernels.hip) and the kernel
// that traverses one (trace_instanced_kernels.hip).  The rule is tests/np_instanced.py; compact_bvh.h holds the node layout both levels share.
//   pool      three buffers (nodes, triWoop, triIndex) that hold several Compact trees (BLAS), each byte for byte what a builder wrote
//             at pool + offset: a BLAS's links are relative to its own start, so no word is rewritten.  A pool buffer is at most
//             kPoolMaxBytes long: the offset kNoNode (trace_lane.h) plus a 64-byte fetch then lies beyond every extent, and a lane that
//             must read nothing is given that offset
//   top level Compact nodes whose leaf links are ~i, i an instance; rootLink is 0, or ~0 when the one instance is the whole tree
//   record i  16 words: 0..11 worldToObject (3x4 row-major), 12 nodesOffset in bytes, 13 triWoopOffset / 16 (rows; triIndex entries
//             too), 14 nodesBytes, 15 zero -- or, after ntr_tlas_motion_refit (tlas_motion_refit_kernels.hip), 1 for an
//             instance that moves within the shutter.  Only the motion kernels (trace_instanced_motion_kernels.hip) read word 15: every
//             other kernel takes words 0..14 and traces the scene at key 0
//   motion    key entry i, beside the records, 32 words: 0..11 objectToWorld at the shutter's opening (key 0), 16..27 objectToWorld at
//             its close (key 1), every other word zero.  Written for every instance, moving or not
//   marker    kExitMarker on the traversal stack, below an instance's entries: a positive word above kSentinel, so neither an inner
//             link (< kSentinel), nor a leaf link (< 0), nor the sentinel
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "compact_bvh.h"

namespace ntr {

constexpr int64_t kPoolMaxBytes = 0xFFFFFF00ll;
constexpr int kRecordWords = 16, kRecordBytes = 64;
constexpr int kRecNodesOffset = 12, kRecRowOffset = 13, kRecNodesBytes = 14, kRecMoving = 15;
constexpr int kMotionKeyBytes = 128, kMotionKey1Bytes = 64;   // a motion key entry, and where key 1 starts in it
constexpr int kExitMarker = kSentinel + 1;
static_assert(kRecordBytes == kNodeBytes, "a record is fetched like a node");
static_assert(kExitMarker > kSentinel, "the marker is neither a link nor the sentinel");

// ---- device: the batched passes over a pool (bvh_refit_batch_, pool_widen_batch_, bvh_optimize_batch_kernels.hip) -----------------------
// Such a pass indexes its per-slot state by a joint slot space: entry e owns [starts[e], starts[e + 1]), the running sum of the listed
// BLASes' slot counts.  The entry of joint slot `slot` (< starts[numEntries]) is the last e with starts[e] <= slot; every entry has a
// slot, so starts rises strictly.  At most 20 steps over a table that a wave's lanes walk together and the L2 holds.
__device__ __forceinline__ int joint_entry_of(const int* __restrict__ starts, int numEntries, int slot)
{
    int lo = 0, hi = numEntries;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= slot) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- host: the checks of the two entry points -----------------------------------------------------------------------------------------
// A pool buffer's size: a multiple of `unit` in [unit, kPoolMaxBytes]
inline int check_pool_bytes(const char* fn, const char* what, int64_t bytes, int unit)
{
    if (bytes < unit || (bytes % unit) != 0 || bytes > kPoolMaxBytes)
        return set_error(NTR_ERR_INVALID, "%s: %s must be a multiple of %d in [%d, 0x%llx]", fn, what, unit, unit, (unsigned long long)kPoolMaxBytes);
    return NTR_OK;
}

// The top-level tree's root: node 0, or the link ~i of an instance that is the whole tree
inline int check_root_link(const char* fn, int32_t rootLink, int32_t numInstances)
{
    if (!(rootLink == 0 || (rootLink < 0 && (int64_t)~rootLink < numInstances)))
        return set_error(NTR_ERR_INVALID, "%s: rootLink %d is neither 0 nor an instance's link", fn, (int)rootLink);
    return NTR_OK;
}

// BLAS k's range against the pool's node buffer and Compact's limits (the triWoop side has no buffer at build time: alignment and
// the pool limit only)
inline int check_blas_range(const char* fn, int k, const NtrBlasRange& r, int64_t poolNodesBytes)
{
    if (r.nodesOffset < 0 || (r.nodesOffset % kNodeBytes) != 0 || r.nodesBytes < kNodeBytes || (r.nodesBytes % kNodeBytes) != 0)
        return set_error(NTR_ERR_INVALID, "%s: BLAS %d: nodesOffset and nodesBytes must be multiples of 64, nodesBytes at least 64", fn, k);
    if (r.nodesBytes > kMaxNodesBytes || r.nodesOffset > poolNodesBytes - r.nodesBytes)
        return set_error(NTR_ERR_INVALID, "%s: BLAS %d: nodes [%lld, +%lld) lie outside the pool's %lld bytes or above Compact's 0x%llx", fn, k,
                         (long long)r.nodesOffset, (long long)r.nodesBytes, (long long)poolNodesBytes, (unsigned long long)kMaxNodesBytes);
    if (r.triWoopOffset < 0 || (r.triWoopOffset % kRowBytes) != 0 || r.triWoopBytes < kRowBytes || (r.triWoopBytes % kRowBytes) != 0 ||
        r.triWoopBytes > kPoolMaxBytes || r.triWoopOffset > kPoolMaxBytes - r.triWoopBytes)
        return set_error(NTR_ERR_INVALID, "%s: BLAS %d: triWoopOffset and triWoopBytes must be multiples of 16 inside a pool of at most 0x%llx bytes",
                         fn, k, (unsigned long long)kPoolMaxBytes);
    return NTR_OK;
}

// Two of n ranges [off(k), off(k) + len(k)) of one buffer overlap: the higher index of the first such pair in index order and, in
// *other, the lower; -1 if none.  Found by a sort over the indices, not a quadratic scan (a batch lists up to 2^20 BLASes).
template <class Off, class Len>
int first_range_overlap(int n, Off off, Len len, int* other)
{
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return off(a) != off(b) ? off(a) < off(b) : a < b; });
    int bad = -1;
    for (int i = 1; i < n; i++) {
        const int p = order[i - 1], q = order[i];
        if (off(q) < off(p) + len(p)) {
            const int hiE = std::max(p, q);
            if (bad < 0 || hiE < bad) { bad = hiE; *other = std::min(p, q); }
        }
    }
    return bad;
}

}  // namespace ntr
