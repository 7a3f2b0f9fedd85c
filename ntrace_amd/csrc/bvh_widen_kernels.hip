// bvh_widen_kernels.hip -- on-device widening of a BVHLayout_Compact tree into 4-wide nodes for gfx950 (ntr_bvh_widen).
//
// EXTENSION without a reference counterpart.  The rule is the numpy spec tests/np_bvh_wide.py, whose docstring is the normative text;
// wide_bvh.h states the node layout and the header comment of ntr_bvh_widen (include/ntrace_amd.h) restates the contract.  The pass is
// out of place: the binary tree is only read, and only a new node buffer is written -- leaves, Woop rows and triIndex are shared.
//
// A *kept* binary slot becomes a wide node: its two children, of which the inner one of largest area is replaced by its own two
// children until there are four entries or no inner entry is left (wd_expand; at most two steps).  The inner entries that remain are
// kept slots in turn.  A wide node's index is the rank of its slot among the kept slots, so the numbering is a property of the set of
// kept slots and the order in which the marking found them never reaches the output.
//
// Shape:
//   wd_seed        slot 0 is kept: level 1, first in the queue
//   wd_mark        a level of the top-down marking, a thread per queue entry of the level: expands its slot and marks each kept child
//                  by one compare-exchange on the child's level word (0 -> level); only the marker that found 0 appends the child to
//                  the queue, so a slot named by several links is kept once and a cycle ends.  The path sum of (count - 1) is carried
//                  down by an integer max among the markers of the same level -- exact whatever the arrival order
//   wd_close       one thread: the queue's tail is where the next level ends
//   the host reads the last two level bounds back once per four levels (the next level's extent sizes the launches: a level is at most
//   four times its parent level), until a level is empty; then the number of kept slots is known and checked against the limits
//   wd_scan_local, scan_block_sums (device_prims.h)   the exclusive scan of the kept flags: the ranks
//   wd_emit        a thread per kept slot: redoes its expansion, writes its 128 bytes and adds its part of the statistics
// Nothing loops without a bound and nobody waits for another workgroup, so the call ends on any input.  No word outside
// [0, 128 * kept slots) of the output is written, and the host has checked that extent against the capacity before wd_emit runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "wide_bvh.h"
#include "wide_expand.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {
namespace {

constexpr int WD_BLOCK = 256;
constexpr int WD_LEVELS_PER_READBACK = 4;

struct WdReport {
    unsigned int tail;                       // entries in the queue
    unsigned int err;                        // links > 0 that name no slot
    unsigned int counts[3], leafLinks, height, stackBound;
    unsigned int pad[8];
};
static_assert(sizeof(WdReport) == 64, "WdReport is one 64-byte record");

DeviceScratchPool g_wdPool;

__global__ void wd_seed(unsigned int* __restrict__ level, unsigned int* __restrict__ queue, unsigned int* __restrict__ bounds,
                        WdReport* __restrict__ report)
{
    level[0] = 1u;
    queue[0] = 0u;
    bounds[0] = 0u;
    bounds[1] = 1u;
    report->tail = 1u;
}

// level[s]: 0 for a slot nobody has marked, otherwise 1 + its distance from the root in wide nodes; pathSum[s]: the largest sum of
// (count - 1) over the ancestors of s among the markers of its level
__global__ __launch_bounds__(WD_BLOCK) void wd_mark(int L, int numSlots, const int* __restrict__ nodes, unsigned int* __restrict__ level,
                                                    unsigned int* __restrict__ pathSum, unsigned int* __restrict__ queue,
                                                    const unsigned int* __restrict__ bounds, WdReport* __restrict__ report)
{
    const unsigned int begin = bounds[L], end = bounds[L + 1];
    const unsigned long long i = (unsigned long long)begin + (unsigned long long)blockIdx.x * WD_BLOCK + threadIdx.x;
    if (i >= end) return;                        // (end <= numSlots: a slot is appended once)
    const int b = (int)queue[i];
    WdEntry E[kWideChildren];
    const int n = wd_expand(nodes, numSlots, b, E);
    const unsigned int sum = pathSum[b] + (unsigned int)(n - 1);
    const unsigned int mine = (unsigned int)L + 2u;
#pragma unroll
    for (int k = 0; k < kWideChildren; k++) {
        if (k >= n || !is_inner_link(E[k].link, numSlots)) continue;
        const int s = inner_index(E[k].link);
        const unsigned int old = atomicCAS(&level[s], 0u, mine);
        if (old == 0u) {
            const unsigned int pos = atomicAdd(&report->tail, 1u);
            if (pos < (unsigned int)numSlots) queue[pos] = (unsigned int)s;
        }
        if (old == 0u || old == mine) atomicMax(&pathSum[s], sum);
    }
}

__global__ void wd_close(int L, unsigned int* __restrict__ bounds, const WdReport* __restrict__ report) { bounds[L + 2] = report->tail; }

__global__ __launch_bounds__(WD_BLOCK) void wd_scan_local(int numSlots, const unsigned int* __restrict__ level, unsigned int* __restrict__ rank,
                                                          unsigned int* __restrict__ blockSums)
{
    const int i = blockIdx.x * WD_BLOCK + threadIdx.x;
    const bool valid = i < numSlots;
    scan_local_store<WD_BLOCK, unsigned int>(valid && level[i] != 0u ? 1u : 0u, valid, (size_t)(valid ? i : 0), rank, blockSums, (int)blockIdx.x);
}

__device__ __forceinline__ unsigned int wd_rank(const unsigned int* __restrict__ rank, const unsigned int* __restrict__ blockSums, int slot)
{
    return rank[slot] + blockSums[slot / WD_BLOCK];
}

__global__ __launch_bounds__(WD_BLOCK) void wd_emit(int numSlots, unsigned int numKept, const int* __restrict__ nodes,
                                                    const unsigned int* __restrict__ level, const unsigned int* __restrict__ pathSum,
                                                    const unsigned int* __restrict__ rank, const unsigned int* __restrict__ blockSums,
                                                    uint4* __restrict__ out, WdReport* __restrict__ report)
{
    const int b = blockIdx.x * WD_BLOCK + threadIdx.x;
    unsigned int c2 = 0u, c3 = 0u, c4 = 0u, leaves = 0u, err = 0u, height = 0u, bound = 0u;
    const unsigned int lv = b < numSlots ? level[b] : 0u;
    if (lv != 0u) {
        const unsigned int w = wd_rank(rank, blockSums, b);
        if (w < numKept) {                       // (always: numKept is the number of marked slots)
            WdEntry E[kWideChildren];
            const int n = wd_expand(nodes, numSlots, b, E);
            int word[kWideWords];
#pragma unroll
            for (int k = 0; k < kWideChildren; k++) {
                const WdEntry e = k < n ? E[k] : WdEntry{0, E[0].src};
                const int* nd = nodes + (size_t)(e.src >> 1) * kNodeWords;
                const int ck = e.src & 1;
#pragma unroll
                for (int j = 0; j < 6; j++) word[wide_box_word(k, j)] = nd[box_word(ck, j)];
                int link = 0;
                if (e.link < 0) {
                    link = e.link;
                    leaves++;
                } else if (is_inner_link(e.link, numSlots)) {
                    link = wide_link((int)wd_rank(rank, blockSums, inner_index(e.link)));
                } else if (e.link != 0) {
                    err++;                       // names no slot: an empty slot
                }
                word[kWideLinkWord + k] = link;
            }
            word[kWideCountWord] = n;
            word[29] = word[30] = word[31] = 0;
            uint4* dst = out + (size_t)w * kWideRows;
#pragma unroll
            for (int r = 0; r < kWideRows; r++)
                dst[r] = make_uint4((unsigned int)word[4 * r], (unsigned int)word[4 * r + 1], (unsigned int)word[4 * r + 2], (unsigned int)word[4 * r + 3]);
            c2 = n == 2; c3 = n == 3; c4 = n == 4;
            height = lv;
            bound = pathSum[b] + (unsigned int)(n - 1);
        }
    }
    c2 = wave_sum_u32(c2); c3 = wave_sum_u32(c3); c4 = wave_sum_u32(c4);
    leaves = wave_sum_u32(leaves); err = wave_sum_u32(err);
    height = wave_max_u32(height); bound = wave_max_u32(bound);
    if ((threadIdx.x & 63) == 0) {
        if (c2) atomicAdd(&report->counts[0], c2);
        if (c3) atomicAdd(&report->counts[1], c3);
        if (c4) atomicAdd(&report->counts[2], c4);
        if (leaves) atomicAdd(&report->leafLinks, leaves);
        if (err) atomicAdd(&report->err, err);
        if (height) atomicMax(&report->height, height);
        if (bound) atomicMax(&report->stackBound, bound);
    }
}

struct WdLayout {
    size_t report, level, pathSum, queue, bounds, rank, blockSums, end;
    explicit WdLayout(int64_t slots)
    {
        ScratchCarver c;
        report = c.take(sizeof(WdReport));
        level = c.take((size_t)slots * 4);
        pathSum = c.take((size_t)slots * 4);
        queue = c.take((size_t)slots * 4);
        bounds = c.take(((size_t)slots + 2 + WD_LEVELS_PER_READBACK) * 4);
        rank = c.take((size_t)slots * 4);
        blockSums = c.take(((size_t)slots / WD_BLOCK + 1) * 4);
        end = c.off;
    }
};

bool wd_ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bn && b0 < a0 + (uintptr_t)an;
}

}  // namespace

// instanced_wide_bvh.h: the pool and TLAS widening keep their BLAS table in this pass's pool
int widen_scratch_reserve(size_t bytes, void** out) { return g_wdPool.reserve(bytes, out); }

}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_widen_capacity(int64_t nodesBytes, int64_t* wideNodesBytes)
{
    if (!wideNodesBytes) return set_error(NTR_ERR_INVALID, "ntr_bvh_widen_capacity: null");
    *wideNodesBytes = 0;
    if (const int rc = check_nodes_bytes("ntr_bvh_widen_capacity", "nodesBytes", nodesBytes)) return rc;
    *wideNodesBytes = (int64_t)kWideBytes * (nodesBytes / kNodeBytes);
    return NTR_OK;
}

int ntr_bvh_widen(const void* d_nodes, int64_t nodesBytes, void* d_wideNodes, int64_t wideCapacity, NtrBvhWideResult* result, void* stream)
{
    const char* fn = "ntr_bvh_widen";
    if (result) memset(result, 0, sizeof(*result));
    if (!d_nodes) return set_error(NTR_ERR_INVALID, "%s: null d_nodes", fn);
    if (const int rc = check_nodes_bytes(fn, "nodesBytes", nodesBytes)) return rc;
    if (!d_wideNodes) return set_error(NTR_ERR_INVALID, "%s: null d_wideNodes", fn);
    if (wideCapacity < (int64_t)kWideBytes * (nodesBytes / kNodeBytes))
        return set_error(NTR_ERR_INVALID, "%s: wideCapacity is below ntr_bvh_widen_capacity()", fn);
    if (!result) return set_error(NTR_ERR_INVALID, "%s: null result", fn);
    if (wd_ranges_overlap(d_wideNodes, wideCapacity, d_nodes, nodesBytes))
        return set_error(NTR_ERR_INVALID, "%s: d_wideNodes overlaps d_nodes (the pass is out of place)", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its level extents back and cannot be captured", fn);

    const int numSlots = (int)(nodesBytes / kNodeBytes);
    const WdLayout lay(numSlots);
    void* base = nullptr;
    {
        const int rc = g_wdPool.reserve(lay.end, &base);
        if (rc != NTR_OK) return rc;
    }
    auto P = [&](size_t o) { return (char*)base + o; };
    WdReport* report = (WdReport*)P(lay.report);
    unsigned int* level = (unsigned int*)P(lay.level);
    unsigned int* pathSum = (unsigned int*)P(lay.pathSum);
    unsigned int* queue = (unsigned int*)P(lay.queue);
    unsigned int* bounds = (unsigned int*)P(lay.bounds);
    unsigned int* rank = (unsigned int*)P(lay.rank);
    unsigned int* blockSums = (unsigned int*)P(lay.blockSums);
    const int* nodes = (const int*)d_nodes;
    const dim3 block(WD_BLOCK);
    const int slotBlocks = (numSlots + WD_BLOCK - 1) / WD_BLOCK;

    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    NTR_HIP(hipMemsetAsync(report, 0, sizeof(WdReport), s));
    NTR_HIP(hipMemsetAsync(level, 0, (size_t)numSlots * 4, s));
    NTR_HIP(hipMemsetAsync(pathSum, 0, (size_t)numSlots * 4, s));
    hipLaunchKernelGGL(wd_seed, dim3(1), dim3(1), 0, s, level, queue, bounds, report);
    // the marking: level L's extent is bounds[L] .. bounds[L + 1]; `most` bounds it from the last extent read back
    int L = 0;
    int64_t most = 1;
    unsigned int numKept = 0;
    for (;;) {
        for (int j = 0; j < WD_LEVELS_PER_READBACK && L < numSlots; j++, L++) {
            hipLaunchKernelGGL(wd_mark, dim3((unsigned int)((most + WD_BLOCK - 1) / WD_BLOCK)), block, 0, s, L, numSlots, nodes, level, pathSum,
                               queue, (const unsigned int*)bounds, report);
            hipLaunchKernelGGL(wd_close, dim3(1), dim3(1), 0, s, L, bounds, (const WdReport*)report);
            most = std::min<int64_t>(most * kWideChildren, numSlots);
        }
        NTR_HIP(hipGetLastError());
        unsigned int h[2] = {0u, 0u};        // the extent of level L
        NTR_HIP(hipMemcpyAsync(h, bounds + L, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        numKept = h[1];
        if (h[1] <= h[0] || L >= numSlots) break;
        most = (int64_t)(h[1] - h[0]);
    }
    if (numKept < 1u || numKept > (unsigned int)numSlots)
        return set_error(NTR_ERR_LAYOUT, "%s: internal error: %u kept slots of %d; nothing was written", fn, numKept, numSlots);
    if ((int64_t)numKept > kMaxWideNodes)
        return set_error(NTR_ERR_OVERFLOW, "%s: the wide tree has %u nodes, more than the %lld that 32-bit links of 128-byte nodes address; nothing "
                         "was written", fn, numKept, (long long)kMaxWideNodes);
    hipLaunchKernelGGL(wd_scan_local, dim3(slotBlocks), block, 0, s, numSlots, (const unsigned int*)level, rank, blockSums);
    hipLaunchKernelGGL((scan_block_sums<WD_BLOCK, unsigned int>), dim3(1), block, 0, s, slotBlocks, (const unsigned int*)blockSums, blockSums,
                       (unsigned int*)nullptr);
    hipLaunchKernelGGL(wd_emit, dim3(slotBlocks), block, 0, s, numSlots, numKept, nodes, (const unsigned int*)level, (const unsigned int*)pathSum,
                       (const unsigned int*)rank, (const unsigned int*)blockSums, (uint4*)d_wideNodes, report);
    NTR_HIP(hipGetLastError());
    NTR_HIP(ev.record(1));
    WdReport h;
    NTR_HIP(hipMemcpyAsync(&h, report, sizeof(h), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->nodesBytes = (int64_t)numKept * kWideBytes;
    result->numNodes = (int32_t)numKept;
    for (int k = 0; k < 3; k++) result->counts[k] = (int32_t)h.counts[k];
    result->numLeafLinks = (int32_t)h.leafLinks;
    result->height = (int32_t)h.height;
    result->stackBound = (int32_t)h.stackBound;
    result->seconds = ms * 1e-3f;
    if (h.err)
        return set_error(NTR_ERR_LAYOUT, "%s: %u child links name no node slot; each was written as an empty slot (the wide tree is complete "
                         "otherwise, and *result describes it)", fn, h.err);
    return NTR_OK;
}

int ntr_bvh_widen_scratch_bytes(int64_t* bytes)
{
    if (!bytes) return set_error(NTR_ERR_INVALID, "ntr_bvh_widen_scratch_bytes: null");
    *bytes = (int64_t)g_wdPool.held();
    return NTR_OK;
}

}  // extern "C"
