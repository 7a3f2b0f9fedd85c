// pool_widen_batch_kernels.hip -- widening every BLAS of a pool into 4-wide nodes in one pass for gfx950 (ntr_pool_widen_batch;
// DESIGN.md 6t).
//
// EXTENSION without a reference counterpart.  The rule is the numpy spec tests/np_instanced_wide.py::widen_pool, the header comment of
// ntr_pool_widen_batch (include/ntrace_amd.h) states the contract, and ntr_pool_widen -- the host loop of ntr_bvh_widen, which stays
// as it is -- is the on-device differential partner: the two write the same bytes.  This is bvh_widen_kernels.hip's pass stated over
// all entries at once, so that the number of launches and read-backs follows the tallest BLAS and not the number of BLASes.
//
// The per-slot state (level, pathSum, queue, rank) is indexed by a *joint* slot space: entry k owns the slots
// [starts[k], starts[k + 1]) of it, starts being the running sum of the entries' own slot counts in k order.  It is not the pool's
// slot space: blasRanges may come in any order, alias or overlap each other and leave gaps, and each listed range is a tree of its
// own.  A link is judged against its entry's slot count only (wide_expand.h is handed the entry's first node and slot count), so a
// link that would land in a neighbour's nodes names no slot.  Because the joint space is in k order and every entry's slot 0 is kept,
// the rank of a kept slot among all kept joint slots is its wide node's index in the wide pool, and the rank of an entry's slot 0 is
// where its wide BLAS begins: placement in k order without gaps needs no further table.
//
// Shape:
//   wb_seed        a thread per entry: its slot 0 is kept, level 1, and is the entry's place in the queue
//   wb_mark        a level of the marking over the joint queue, a thread per queue entry (which carries its entry's index): wd_mark's
//                  rule with the entry's pointer and slot count
//   wb_close       one thread: the queue's tail is where the next level ends
//   the host reads the last two level bounds back once per four levels, until a level is empty: as often as for the tallest BLAS
//   wb_scan_local, scan_block_sums (device_prims.h)   the exclusive scan of the kept flags over the joint space
//   wb_table       a thread per entry: its first wide node and its node count (the difference of the ranks at its ends), and the largest
//                  count into the report -- read back before wb_emit only if some entry has more slots than a wide tree has nodes
//   wb_emit        a thread per joint slot: a kept one redoes its expansion and writes its 128 bytes; counts, leaf links and height are
//                  folded per wave and per workgroup into one of the report's slots, stackBound and the error count go to the slot's
//                  own entry (one atomic of the wave's fold where the wave lies in one entry, per lane where it straddles entries)
//   one read-back of the report's slots and the entry table
// Nothing loops without a bound and nobody waits for another workgroup, so the call ends on any input.  No word outside
// [0, 128 * kept slots) of the output is written; that extent is at most the capacity, which the host has checked against
// 128 * joint slots, and the limits are checked before wb_emit runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_wide_bvh.h"
#include "level_build.h"
#include "wide_expand.h"

namespace ntr {
namespace {

constexpr int WB_BLOCK = 256;
constexpr int WB_LEVELS_PER_READBACK = 4;
constexpr int WB_MAX_ENTRIES = 1 << 20;
constexpr int64_t WB_MAX_SLOTS = kPoolMaxBytes / kNodeBytes;   // what a pool without aliased ranges holds: every index below fits an int

struct WbReport {
    unsigned int tail;                       // entries in the queue
    unsigned int counts[3], leafLinks, height;
    unsigned int maxKept;                    // the largest node count of any entry (wb_table)
    unsigned int pad[9];
};
static_assert(sizeof(WbReport) == 64, "WbReport is one 64-byte record");
// tail and maxKept live in slot 0; wb_emit's workgroups add counts, leaf links and height to the slot of their number modulo
// WB_REPORT_SLOTS and the host folds the slots, as wide_refit_batch_kernels.hip's statistics
constexpr int WB_REPORT_SLOTS = 64;

struct WbIn {                                // an entry as the kernels see it
    int slotBase, numSlots;                  // its first node in the pool (nodesOffset / 64), its slots
};
struct WbOut {                               // what the pass finds out about an entry
    unsigned int firstNode, numNodes;        // its first wide node in the wide pool, its wide nodes
    unsigned int stackBound, err;            // NtrBvhWideResult's; links > 0 that name no slot of the entry
};
static_assert(sizeof(WbOut) == 16, "WbOut is 16 bytes");

DeviceScratchPool g_wbPool;

__global__ __launch_bounds__(WB_BLOCK) void wb_seed(int numEntries, const int* __restrict__ starts, unsigned int* __restrict__ level,
                                                    unsigned int* __restrict__ queue, unsigned int* __restrict__ queueEntry,
                                                    unsigned int* __restrict__ bounds, WbReport* __restrict__ report)
{
    const int e = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (e == 0) {
        bounds[0] = 0u;
        bounds[1] = (unsigned int)numEntries;
        report->tail = (unsigned int)numEntries;
    }
    if (e >= numEntries) return;
    const int s = starts[e];
    level[s] = 1u;
    queue[e] = (unsigned int)s;
    queueEntry[e] = (unsigned int)e;
}

// level[s], pathSum[s]: as bvh_widen_kernels.hip's, over the joint slots
__global__ __launch_bounds__(WB_BLOCK) void wb_mark(int L, int totalSlots, const int* __restrict__ pool, const int* __restrict__ starts,
                                                    const WbIn* __restrict__ in, unsigned int* __restrict__ level,
                                                    unsigned int* __restrict__ pathSum, unsigned int* __restrict__ queue,
                                                    unsigned int* __restrict__ queueEntry, const unsigned int* __restrict__ bounds,
                                                    WbReport* __restrict__ report)
{
    const unsigned int begin = bounds[L], end = bounds[L + 1];
    const unsigned long long i = (unsigned long long)begin + (unsigned long long)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= end) return;                        // (end <= totalSlots: a slot is appended once)
    const int s = (int)queue[i];
    const unsigned int e = queueEntry[i];
    const int first = starts[e];
    const WbIn I = in[e];
    WdEntry E[kWideChildren];
    const int n = wd_expand(pool + (size_t)I.slotBase * kNodeWords, I.numSlots, s - first, E);
    const unsigned int sum = pathSum[s] + (unsigned int)(n - 1);
    const unsigned int mine = (unsigned int)L + 2u;
#pragma unroll
    for (int k = 0; k < kWideChildren; k++) {
        if (k >= n || !is_inner_link(E[k].link, I.numSlots)) continue;
        const int c = first + inner_index(E[k].link);     // < first + numSlots: the entry's own joint slots
        const unsigned int old = atomicCAS(&level[c], 0u, mine);
        if (old == 0u) {
            const unsigned int pos = atomicAdd(&report->tail, 1u);
            if (pos < (unsigned int)totalSlots) {
                queue[pos] = (unsigned int)c;
                queueEntry[pos] = e;
            }
        }
        if (old == 0u || old == mine) atomicMax(&pathSum[c], sum);
    }
}

__global__ void wb_close(int L, unsigned int* __restrict__ bounds, const WbReport* __restrict__ report) { bounds[L + 2] = report->tail; }

__global__ __launch_bounds__(WB_BLOCK) void wb_scan_local(int totalSlots, const unsigned int* __restrict__ level, unsigned int* __restrict__ rank,
                                                          unsigned int* __restrict__ blockSums)
{
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    const bool valid = i < totalSlots;
    scan_local_store<WB_BLOCK, unsigned int>(valid && level[i] != 0u ? 1u : 0u, valid, (size_t)(valid ? i : 0), rank, blockSums, (int)blockIdx.x);
}

__device__ __forceinline__ unsigned int wb_rank(const unsigned int* __restrict__ rank, const unsigned int* __restrict__ blockSums, int slot)
{
    return rank[slot] + blockSums[slot / WB_BLOCK];
}

__global__ __launch_bounds__(WB_BLOCK) void wb_table(int numEntries, unsigned int numKept, const int* __restrict__ starts,
                                                     const unsigned int* __restrict__ rank, const unsigned int* __restrict__ blockSums,
                                                     WbOut* __restrict__ out, WbReport* __restrict__ report)
{
    const int e = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (e >= numEntries) return;
    const unsigned int r0 = wb_rank(rank, blockSums, starts[e]);
    const unsigned int r1 = e + 1 < numEntries ? wb_rank(rank, blockSums, starts[e + 1]) : numKept;
    out[e] = WbOut{r0, r1 - r0, 0u, 0u};
    atomicMax(&report->maxKept, r1 - r0);
}

__global__ __launch_bounds__(WB_BLOCK) void wb_emit(int numEntries, int totalSlots, unsigned int numKept, const int* __restrict__ pool,
                                                    const int* __restrict__ starts, const WbIn* __restrict__ in,
                                                    const unsigned int* __restrict__ level, const unsigned int* __restrict__ pathSum,
                                                    const unsigned int* __restrict__ rank, const unsigned int* __restrict__ blockSums,
                                                    uint4* __restrict__ outNodes, WbOut* __restrict__ out, WbReport* __restrict__ report)
{
    const int s = blockIdx.x * WB_BLOCK + threadIdx.x;
    unsigned int c2 = 0u, c3 = 0u, c4 = 0u, leaves = 0u, err = 0u, height = 0u, bound = 0u;
    // every lane has an entry, kept slot or not, so that a wave inside one entry is told by one comparison
    const int e = joint_entry_of(starts, numEntries, s < totalSlots ? s : totalSlots - 1);
    const unsigned int lv = s < totalSlots ? level[s] : 0u;
    if (lv != 0u) {
        const unsigned int w = wb_rank(rank, blockSums, s);
        if (w < numKept) {                       // (always: numKept is the number of marked slots)
            const int first = starts[e];
            const WbIn I = in[e];
            const int* nodes = pool + (size_t)I.slotBase * kNodeWords;
            const unsigned int base = wb_rank(rank, blockSums, first);   // the entry's slot 0 is kept: its rank is the entry's first wide node
            WdEntry E[kWideChildren];
            const int n = wd_expand(nodes, I.numSlots, s - first, E);
            int word[kWideWords];
#pragma unroll
            for (int k = 0; k < kWideChildren; k++) {
                const WdEntry en = k < n ? E[k] : WdEntry{0, E[0].src};
                const int* nd = nodes + (size_t)(en.src >> 1) * kNodeWords;
                const int ck = en.src & 1;
#pragma unroll
                for (int j = 0; j < 6; j++) word[wide_box_word(k, j)] = nd[box_word(ck, j)];
                int link = 0;
                if (en.link < 0) {
                    link = en.link;
                    leaves++;
                } else if (is_inner_link(en.link, I.numSlots)) {
                    link = wide_link((int)(wb_rank(rank, blockSums, first + inner_index(en.link)) - base));   // relative to the BLAS's own start
                } else if (en.link != 0) {
                    err++;                       // names no slot of its own BLAS: an empty slot
                }
                word[kWideLinkWord + k] = link;
            }
            word[kWideCountWord] = n;
            word[29] = word[30] = word[31] = 0;
            uint4* dst = outNodes + (size_t)w * kWideRows;
#pragma unroll
            for (int r = 0; r < kWideRows; r++)
                dst[r] = make_uint4((unsigned int)word[4 * r], (unsigned int)word[4 * r + 1], (unsigned int)word[4 * r + 2], (unsigned int)word[4 * r + 3]);
            c2 = n == 2; c3 = n == 3; c4 = n == 4;
            height = lv;
            bound = pathSum[s] + (unsigned int)(n - 1);
        }
    }
    // the pool's totals: folded per wave, then per workgroup in LDS, then one add per workgroup and counter into the workgroup's slot of
    // the report (the host sums the slots): a million slots would otherwise queue tens of thousands of adds on one line
    __shared__ unsigned int sums[5];
    if (threadIdx.x < 5) sums[threadIdx.x] = 0u;
    __syncthreads();
    c2 = wave_sum_u32(c2); c3 = wave_sum_u32(c3); c4 = wave_sum_u32(c4);
    leaves = wave_sum_u32(leaves);
    height = wave_max_u32(height);
    if ((threadIdx.x & 63) == 0) {
        if (c2) atomicAdd(&sums[0], c2);
        if (c3) atomicAdd(&sums[1], c3);
        if (c4) atomicAdd(&sums[2], c4);
        if (leaves) atomicAdd(&sums[3], leaves);
        if (height) atomicMax(&sums[4], height);
    }
    __syncthreads();
    if (threadIdx.x < 5 && sums[threadIdx.x]) {
        WbReport* mine = report + blockIdx.x % WB_REPORT_SLOTS;
        unsigned int* dst = threadIdx.x < 3 ? &mine->counts[threadIdx.x] : (threadIdx.x == 3 ? &mine->leafLinks : &mine->height);
        if (threadIdx.x == 4) atomicMax(dst, sums[4]); else atomicAdd(dst, sums[threadIdx.x]);
    }
    // the entry's own: a wave's fold is the entry's only where all 64 lanes lie in that entry
    if (wave_uniform(e)) {
        bound = wave_max_u32(bound);
        err = wave_sum_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (bound) atomicMax(&out[e].stackBound, bound);
            if (err) atomicAdd(&out[e].err, err);
        }
    } else {
        if (bound) atomicMax(&out[e].stackBound, bound);
        if (err) atomicAdd(&out[e].err, err);
    }
}

struct WbLayout {
    size_t head, starts, in, level, pathSum, queue, queueEntry, bounds, rank, blockSums, end;
    WbLayout(int64_t entries, int64_t slots, int64_t maxSlots)
    {
        ScratchCarver c;
        head = c.take(sizeof(WbReport) * WB_REPORT_SLOTS + (size_t)entries * sizeof(WbOut));   // the report's slots, then the entry table: one read-back
        starts = c.take(((size_t)entries + 1) * 4);
        in = c.take((size_t)entries * sizeof(WbIn));
        level = c.take((size_t)slots * 4);
        pathSum = c.take((size_t)slots * 4);
        queue = c.take((size_t)slots * 4);
        queueEntry = c.take((size_t)slots * 4);
        bounds = c.take(((size_t)maxSlots + 2 + WB_LEVELS_PER_READBACK) * 4);
        rank = c.take((size_t)slots * 4);
        blockSums = c.take(((size_t)slots / WB_BLOCK + 1) * 4);
        end = c.off;
    }
};

bool wb_ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bn && b0 < a0 + (uintptr_t)an;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_pool_widen_batch(int32_t numBlas, const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes, void* d_widePoolNodes,
                         int64_t capacity, NtrWideBlasRange* wideRanges, NtrBvhWideResult* result, void* stream)
{
    const char* fn = "ntr_pool_widen_batch";
    if (result) memset(result, 0, sizeof(*result));
    if (numBlas < 1 || !blasRanges || !wideRanges) return set_error(NTR_ERR_INVALID, "%s: no BLAS ranges", fn);
    if (numBlas > WB_MAX_ENTRIES) return set_error(NTR_ERR_INVALID, "%s: numBlas %d exceeds %d", fn, (int)numBlas, WB_MAX_ENTRIES);
    memset(wideRanges, 0, sizeof(NtrWideBlasRange) * (size_t)numBlas);
    if (!d_poolNodes || !d_widePoolNodes || !result) return set_error(NTR_ERR_INVALID, "%s: null buffer or result", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    std::vector<int> starts((size_t)numBlas + 1);
    std::vector<WbIn> in((size_t)numBlas);
    int64_t need = 0, total = 0, maxSlots = 0;
    for (int k = 0; k < numBlas; k++) {
        if (const int rc = check_blas_range(fn, k, blasRanges[k], poolNodesBytes)) return rc;
        const int64_t slots = blasRanges[k].nodesBytes / kNodeBytes;   // (ntr_bvh_widen_capacity: 128 bytes per slot)
        need += (int64_t)kWideBytes * slots;
        in[(size_t)k] = WbIn{(int)(blasRanges[k].nodesOffset / kNodeBytes), (int)slots};
        starts[(size_t)k] = (int)std::min<int64_t>(total, WB_MAX_SLOTS);
        total += slots;
        maxSlots = std::max(maxSlots, slots);
    }
    if (capacity < need) return set_error(NTR_ERR_INVALID, "%s: capacity is below ntr_pool_widen_capacity()", fn);
    if (wb_ranges_overlap(d_widePoolNodes, capacity, d_poolNodes, poolNodesBytes))
        return set_error(NTR_ERR_INVALID, "%s: d_widePoolNodes overlaps d_poolNodes (the pass is out of place)", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads extents back and cannot be captured", fn);
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    // ranges that alias each other can list more slots than a pool holds; well-formed trees of that many slots exceed the wide pool's limit
    if (total > WB_MAX_SLOTS)
        return set_error(NTR_ERR_OVERFLOW, "%s: the ranges list %lld node slots in all, more than the %lld of a pool of 0x%llx bytes; nothing was "
                         "written", fn, (long long)total, (long long)WB_MAX_SLOTS, (unsigned long long)kPoolMaxBytes);
    starts[(size_t)numBlas] = (int)total;

    const int totalSlots = (int)total;
    const WbLayout lay(numBlas, total, maxSlots);
    void* base = nullptr;
    if (const int rc = g_wbPool.reserve(lay.end, &base)) return rc;
    WbReport* report = at<WbReport>(base, lay.head);
    WbOut* out = at<WbOut>(base, lay.head + sizeof(WbReport) * WB_REPORT_SLOTS);
    int* d_starts = at<int>(base, lay.starts);
    WbIn* d_in = at<WbIn>(base, lay.in);
    unsigned int *level = at<unsigned int>(base, lay.level), *pathSum = at<unsigned int>(base, lay.pathSum);
    unsigned int *queue = at<unsigned int>(base, lay.queue), *queueEntry = at<unsigned int>(base, lay.queueEntry);
    unsigned int *bounds = at<unsigned int>(base, lay.bounds), *rank = at<unsigned int>(base, lay.rank);
    unsigned int* blockSums = at<unsigned int>(base, lay.blockSums);
    const int* pool = (const int*)d_poolNodes;
    const dim3 block(WB_BLOCK);
    const int slotBlocks = (totalSlots + WB_BLOCK - 1) / WB_BLOCK, entryBlocks = (numBlas + WB_BLOCK - 1) / WB_BLOCK;

    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    // (the host arrays outlive the uploads: the first read-back below waits for the stream)
    NTR_HIP(hipMemcpyAsync(d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemcpyAsync(d_in, in.data(), in.size() * sizeof(WbIn), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemsetAsync(report, 0, sizeof(WbReport) * WB_REPORT_SLOTS, s));
    NTR_HIP(hipMemsetAsync(level, 0, (size_t)totalSlots * 4, s));
    NTR_HIP(hipMemsetAsync(pathSum, 0, (size_t)totalSlots * 4, s));
    hipLaunchKernelGGL(wb_seed, dim3(entryBlocks), block, 0, s, (int)numBlas, (const int*)d_starts, level, queue, queueEntry, bounds, report);
    // the marking: level L's joint extent is bounds[L] .. bounds[L + 1]; `most` bounds it from the last extent read back.  A level
    // that has an entry in it has marked a new slot in some entry on every level before: L < the largest entry's slots
    int L = 0;
    int64_t most = numBlas;
    unsigned int numKept = 0;
    for (;;) {
        for (int j = 0; j < WB_LEVELS_PER_READBACK && L < maxSlots; j++, L++) {
            hipLaunchKernelGGL(wb_mark, dim3((unsigned int)((most + WB_BLOCK - 1) / WB_BLOCK)), block, 0, s, L, totalSlots, pool,
                               (const int*)d_starts, (const WbIn*)d_in, level, pathSum, queue, queueEntry, (const unsigned int*)bounds, report);
            hipLaunchKernelGGL(wb_close, dim3(1), dim3(1), 0, s, L, bounds, (const WbReport*)report);
            most = std::min<int64_t>(most * kWideChildren, totalSlots);
        }
        NTR_HIP(hipGetLastError());
        unsigned int h[2] = {0u, 0u};        // the extent of level L
        NTR_HIP(hipMemcpyAsync(h, bounds + L, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        numKept = h[1];
        if (h[1] <= h[0] || L >= maxSlots) break;
        most = (int64_t)(h[1] - h[0]);
    }
    if (numKept < (unsigned int)numBlas || numKept > (unsigned int)totalSlots)
        return set_error(NTR_ERR_LAYOUT, "%s: internal error: %u kept slots of %d in %d BLASes; nothing was written", fn, numKept, totalSlots,
                         (int)numBlas);
    if ((int64_t)numKept * kWideBytes > kPoolMaxBytes)
        return set_error(NTR_ERR_OVERFLOW, "%s: the wide pool has %u nodes and would exceed 0x%llx bytes; nothing was written", fn, numKept,
                         (unsigned long long)kPoolMaxBytes);
    hipLaunchKernelGGL(wb_scan_local, dim3(slotBlocks), block, 0, s, totalSlots, (const unsigned int*)level, rank, blockSums);
    hipLaunchKernelGGL((scan_block_sums<WB_BLOCK, unsigned int>), dim3(1), block, 0, s, slotBlocks, (const unsigned int*)blockSums, blockSums,
                       (unsigned int*)nullptr);
    hipLaunchKernelGGL(wb_table, dim3(entryBlocks), block, 0, s, (int)numBlas, numKept, (const int*)d_starts, (const unsigned int*)rank,
                       (const unsigned int*)blockSums, out, report);
    if (maxSlots > kMaxWideNodes) {          // only then can a BLAS exceed a wide tree's limit: the one further read-back
        NTR_HIP(hipGetLastError());
        WbReport h;
        NTR_HIP(hipMemcpyAsync(&h, report, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        if ((int64_t)h.maxKept > kMaxWideNodes)
            return set_error(NTR_ERR_OVERFLOW, "%s: a wide BLAS has %u nodes, more than the %lld that 32-bit links of 128-byte nodes address; "
                             "nothing was written", fn, h.maxKept, (long long)kMaxWideNodes);
    }
    hipLaunchKernelGGL(wb_emit, dim3(slotBlocks), block, 0, s, (int)numBlas, totalSlots, numKept, pool, (const int*)d_starts, (const WbIn*)d_in,
                       (const unsigned int*)level, (const unsigned int*)pathSum, (const unsigned int*)rank, (const unsigned int*)blockSums,
                       (uint4*)d_widePoolNodes, out, report);
    NTR_HIP(hipGetLastError());
    NTR_HIP(ev.record(1));
    static_assert(sizeof(WbReport) % sizeof(WbOut) == 0, "the report is a whole number of table records");
    constexpr size_t kHead = sizeof(WbReport) * WB_REPORT_SLOTS / sizeof(WbOut);
    std::vector<WbOut> host(kHead + (size_t)numBlas);
    NTR_HIP(hipMemcpyAsync(host.data(), report, host.size() * sizeof(WbOut), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    WbReport h;
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < WB_REPORT_SLOTS; i++) {
        WbReport one;
        memcpy(&one, (const char*)host.data() + sizeof(WbReport) * (size_t)i, sizeof(one));
        for (int k = 0; k < 3; k++) h.counts[k] += one.counts[k];
        h.leafLinks += one.leafLinks;
        h.height = std::max(h.height, one.height);
    }
    const WbOut* t = host.data() + kHead;
    int firstBad = -1;
    uint64_t errs = 0;
    unsigned int bound = 0;
    for (int k = 0; k < numBlas; k++) {
        wideRanges[k].nodesOffset = (int64_t)t[k].firstNode * kWideBytes;
        wideRanges[k].nodesBytes = (int64_t)t[k].numNodes * kWideBytes;
        wideRanges[k].numNodes = (int32_t)t[k].numNodes;
        wideRanges[k].stackBound = (int32_t)t[k].stackBound;
        bound = std::max(bound, t[k].stackBound);
        if (t[k].err && firstBad < 0) firstBad = k;
        errs += t[k].err;
    }
    result->nodesBytes = (int64_t)numKept * kWideBytes;
    result->numNodes = (int32_t)numKept;
    for (int k = 0; k < 3; k++) result->counts[k] = (int32_t)h.counts[k];
    result->numLeafLinks = (int32_t)h.leafLinks;
    result->height = (int32_t)h.height;
    result->stackBound = (int32_t)bound;
    result->seconds = ms * 1e-3f;
    if (errs)
        return set_error(NTR_ERR_LAYOUT, "%s: %llu child links name no node slot of their own BLAS, the first in BLAS %d; each was written as an "
                         "empty slot (every wide BLAS is complete otherwise, and *result and wideRanges describe them)", fn,
                         (unsigned long long)errs, firstBad);
    return NTR_OK;
}

int ntr_pool_widen_batch_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_pool_widen_batch_scratch_bytes", g_wbPool, bytes); }

}  // extern "C"
