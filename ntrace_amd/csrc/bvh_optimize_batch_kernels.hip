// bvh_optimize_batch_kernels.hip -- treelet restructuring (ntr_bvh_optimize_batch) and SAH cost (ntr_bvh_sah_cost_batch) of many BLASes
// of a pool in one pass for gfx950.
//
// EXTENSIONS without a reference counterpart.  The rule is the numpy spec tests/np_optimize_batch.py -- np_bvh_optimize.optimize and
// sah_cost over every entry's slices of the pool -- and the header comments (include/ntrace_amd.h) state the contracts.  A BLAS is byte
// for byte a Compact tree whose links are relative to its own start (instanced_bvh.h), so ntr_bvh_optimize at pool + offset already
// writes the right bytes; a pool of a thousand BLASes pays its read-back per pass and its launch per height a thousand times.  This is
// bvh_optimize_kernels.hip's pass stated over all entries at once, so that launches and read-backs follow the tallest BLAS and not the
// number of BLASes.  What the pass carries and what it does with a treelet is stated once, in bvh_optimize_payload.h and
// bvh_optimize_treelet.h; here is only how a thread finds its BLAS.
//
// The per-slot state is indexed by a *joint* slot space, as in pool_widen_batch_kernels.hip: entry k owns the joint slots
// [starts[k], starts[k + 1]), starts being the running sum of the entries' own slot counts.  A thread finds its entry by the binary
// search of bvh_refit_batch_kernels.hip in that table, and hands the shared bodies its BLAS's own pointers and slot count: a link is
// judged against its own BLAS's extent only.
//   ob_topology      a thread per joint slot: bvh_climb.h's topology step inside the slot's BLAS; clears the slot's height and the
//                    histogram; a malformed link goes into the entry's report and into the call's
//   ob_climb<false>  a thread per child word: op_climb_child with the entry's arrays; the owner of an entry's slot 0 writes that
//                    entry's report, and one atomic max keeps the tallest height
//   ob_histogram     one histogram of treelet roots over all entries, by height; an entry whose slot 0 nobody reached has no roots,
//                    so it stays as it is
//   ob_scan, ob_scatter   one scan up to the tallest height, one scatter into per-height lists of joint slots
//   ob_treelets      per height that has roots one launch, one wave64 per treelet: the wave resolves its entry and runs
//                    op_treelet_body on pool + nodeBase with that entry's slot count.  Treelets of one height are disjoint inside a
//                    BLAS, and BLASes share no byte (overlapping entries are refused)
// ntr_bvh_sah_cost_batch is ob_topology + ob_climb<true>, and one read-back of the entries' reports.
// Nothing loops without a bound and nobody waits for another workgroup, so both calls end on any input; no link is followed out of
// its BLAS, so nothing outside the listed ranges is read or written.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_optimize_payload.h"
#include "bvh_optimize_treelet.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_bvh.h"
#include "level_build.h"

namespace ntr {
namespace {

constexpr int OB_MAX_ENTRIES = 1 << 20;
constexpr int64_t OB_MAX_SLOTS = kPoolMaxBytes / kNodeBytes;   // what a pool without repeated ranges holds: every index below fits an int

struct ObEntry {                             // a listed BLAS as the kernels see it
    int nodeBase, numSlots;                  // its first node slot in the pool, its slots
    int rowBase, numRows;                    // its first Woop row, its rows (the SAH cost only)
};
static_assert(sizeof(ObEntry) == 16, "ObEntry must be 16 bytes");

struct ObRound {                             // cleared before every climb
    unsigned int tallest;                    // the greatest height any entry's slot 0 has reported
    unsigned int pad[15];
};
struct ObCall {                              // cleared once per call
    unsigned int err, bad;                   // the OR of the entries' error bits; the maximum of ~entry over the entries that have one
    unsigned int pad[14];
};
static_assert(sizeof(ObRound) == 64 && sizeof(ObCall) == 64, "one 64-byte record each");

DeviceScratchPool g_obPool;

__device__ __forceinline__ void ob_flag(ObCall* __restrict__ call, int e, unsigned int bits)
{
    atomicOr(&call->err, bits);
    atomicMax(&call->bad, ~(unsigned int)e);
}

__global__ __launch_bounds__(OP_BLOCK) void ob_topology(int numEntries, int totalSlots, int maxSlots, const int* __restrict__ starts,
                                                        const ObEntry* __restrict__ table, const int* __restrict__ pool,
                                                        unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                        int* __restrict__ height /* or null */,
                                                        unsigned int* __restrict__ hist /* maxSlots + 1 words, or null */,
                                                        OpRoot* __restrict__ reports, ObCall* __restrict__ call)
{
    const int slot = blockIdx.x * OP_BLOCK + threadIdx.x;   // the grid covers totalSlots + 1 >= maxSlots + 1 threads
    if (hist && slot <= maxSlots) hist[slot] = 0u;
    if (slot >= totalSlots) return;
    const int e = joint_entry_of(starts, numEntries, slot);
    const int first = starts[e];
    const ObEntry E = table[e];
    if (height) height[slot] = 0;
    int kind[2];
    topology_slot(slot - first, E.numSlots, pool + (size_t)E.nodeBase * kNodeWords, parent + first, arrive + first, kind);
    if (kind[0] == LINK_BAD || kind[1] == LINK_BAD) {       // a malformed tree only
        atomicOr(&reports[e].err, OP_ERR_LINK);
        ob_flag(call, e, OP_ERR_LINK);
    }
    // the optimiser only: a slot 0 without any child (a zero-filled slot) is no tree.  Nothing of such an entry is reached, so it stays
    // as it is either way; ntr_bvh_optimize does the same to it and says nothing
    if (height && slot == first && kind[0] == LINK_NONE && kind[1] == LINK_NONE) {
        atomicOr(&reports[e].err, (unsigned int)NTR_OPT_ERR_NO_TREE);
        ob_flag(call, e, (unsigned int)NTR_OPT_ERR_NO_TREE);
    }
}

template <bool SAH>
__global__ __launch_bounds__(OP_BLOCK) void ob_climb(int numEntries, int totalSlots, const int* __restrict__ starts,
                                                     const ObEntry* __restrict__ table, const int* __restrict__ pool,
                                                     const float4* __restrict__ poolWoop, const unsigned int* __restrict__ parent,
                                                     unsigned int* __restrict__ arrive, unsigned long long* __restrict__ info,
                                                     int* __restrict__ height, unsigned int* __restrict__ leafLinks,
                                                     OpRoot* __restrict__ reports, ObRound* __restrict__ round)
{
    const long long g = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (g >= 2ll * totalSlots) return;
    const int slot = (int)(g >> 1);
    const int e = joint_entry_of(starts, numEntries, slot);
    const int first = starts[e];
    const ObEntry E = table[e];
    op_climb_child<SAH>(slot - first, (int)(g & 1), E.numSlots, pool + (size_t)E.nodeBase * kNodeWords, E.numRows,
                        SAH ? poolWoop + E.rowBase : nullptr, parent + first, arrive + first, info + 2 * (size_t)first * (SAH ? 3 : 1),
                        SAH ? nullptr : height + first, SAH ? nullptr : leafLinks + first, reports + e, &round->tallest);
}

// qual[joint slot] and the joint histogram, as opt_histogram's.  The thread of an entry's slot 0 keeps the entry's height of the first
// pass (firstHeights, or null in later passes) and flags an entry whose slot 0 the climb never owned.
__global__ __launch_bounds__(OP_BLOCK) void ob_histogram(int numEntries, int totalSlots, const int* __restrict__ starts,
                                                         const ObEntry* __restrict__ table, const int* __restrict__ pool,
                                                         const unsigned int* __restrict__ parent, const int* __restrict__ height,
                                                         const unsigned int* __restrict__ leafLinks, const OpRoot* __restrict__ reports,
                                                         int* __restrict__ qual, unsigned int* __restrict__ hist,
                                                         int* __restrict__ firstHeights, ObCall* __restrict__ call)
{
    const int slot = blockIdx.x * OP_BLOCK + threadIdx.x;
    const bool live = slot < totalSlots;
    int first = 0;
    ObEntry E = {};
    bool done = false;
    if (live) {
        const int e = joint_entry_of(starts, numEntries, slot);
        first = starts[e];
        E = table[e];
        done = reports[e].done != 0u;
        if (!done) qual[slot] = 0;
        if (slot == first) {
            if (firstHeights) firstHeights[e] = done ? (int)reports[e].height : 0;
            if (!done) ob_flag(call, e, (unsigned int)NTR_OPT_ERR_NO_TREE);
        }
    }
    op_histogram_body(live && done, slot - first, E.numSlots, pool + (size_t)E.nodeBase * kNodeWords, parent + first, height + first,
                      leafLinks + first, qual + slot, hist);
}

__global__ __launch_bounds__(OP_BLOCK) void ob_scan(int maxSlots, const ObRound* __restrict__ round, const unsigned int* __restrict__ hist,
                                                    unsigned int* __restrict__ cursor)
{
    op_scan_body((int)min(round->tallest, (unsigned int)maxSlots) + 1, hist, cursor);
}

__global__ __launch_bounds__(OP_BLOCK) void ob_scatter(int totalSlots, const int* __restrict__ qual, unsigned int* __restrict__ cursor,
                                                       int* __restrict__ list)
{
    op_scatter_body(totalSlots, qual, cursor, list);
}

// One wave64 (one workgroup) per treelet; roots holds joint slots
__global__ __launch_bounds__(64) void ob_treelets(int numEntries, const int* __restrict__ starts, const ObEntry* __restrict__ table,
                                                  int* __restrict__ pool, const int* __restrict__ roots, int count,
                                                  unsigned int* __restrict__ rewritten)
{
    if ((int)blockIdx.x >= count) return;
    const int J = roots[blockIdx.x];
    if (J < 0 || J >= starts[numEntries]) return;
    const int e = joint_entry_of(starts, numEntries, J);
    const ObEntry E = table[e];
    op_treelet_body(E.numSlots, pool + (size_t)E.nodeBase * kNodeWords, J - starts[e], rewritten);
}

// One block, so that each read-back is one copy: the entries' first heights and reports (the per-entry read-back); the reports and the
// round's record (the memset of a round); the round's record, the call's, the counters and the histogram (the read-back of a pass).
struct ObLayout {
    size_t firstHeights, reports, round, call, stats, hist, starts, table, parent, arrive, info, height, leafLinks, qual, cursor, list, end;
    ObLayout(int64_t entries, int64_t slots, int64_t maxSlots, bool sah)
    {
        ScratchCarver c;
        const size_t fh = ((size_t)entries * 4 + 63) & ~(size_t)63;
        const size_t head = c.take(fh + (size_t)entries * sizeof(OpRoot) + sizeof(ObRound) + sizeof(ObCall) +
                                   sizeof(unsigned int) * OP_STAT_SLOTS * OP_MAX_PASSES + (size_t)(maxSlots + 1) * 4);
        firstHeights = head;
        reports = firstHeights + fh;
        round = reports + (size_t)entries * sizeof(OpRoot);
        call = round + sizeof(ObRound);
        stats = call + sizeof(ObCall);
        hist = stats + sizeof(unsigned int) * OP_STAT_SLOTS * OP_MAX_PASSES;
        starts = c.take((size_t)(entries + 1) * 4);
        table = c.take((size_t)entries * sizeof(ObEntry));
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        info = c.take((size_t)slots * 2 * 8 * (sah ? 3 : 1));
        height = leafLinks = qual = cursor = list = c.off;
        if (!sah) {
            height = c.take((size_t)slots * 4);
            leafLinks = c.take((size_t)slots * 4);
            qual = c.take((size_t)slots * 4);
            cursor = c.take((size_t)(maxSlots + 1) * 4);
            list = c.take((size_t)slots * 4);
        }
        end = c.off;
    }
};

// The arguments both calls share, and the entry table.  rows: the SAH call, which reads the entries' row ranges too.
int ob_check(const char* fn, int32_t numEntries, const NtrBlasRange* entries, const void* d_poolNodes, int64_t poolNodesBytes, bool rows,
             const void* d_poolTriWoop, int64_t poolTriWoopBytes, std::vector<int>& starts, std::vector<ObEntry>& table, int64_t* totalSlots,
             int64_t* maxSlots)
{
    if (numEntries < 1 || numEntries > OB_MAX_ENTRIES || !entries)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numEntries <= %d, a non-null entry array)", fn, OB_MAX_ENTRIES);
    if (!d_poolNodes || (rows && !d_poolTriWoop)) return set_error(NTR_ERR_INVALID, "%s: null pool buffer", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (rows)
        if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (((uintptr_t)d_poolNodes | (rows ? (uintptr_t)d_poolTriWoop : 0)) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the pool's buffers must be 16-byte aligned", fn);
    starts.resize((size_t)numEntries + 1);
    table.resize((size_t)numEntries);
    int64_t total = 0, most = 0;
    for (int k = 0; k < numEntries; k++) {
        const NtrBlasRange& r = entries[k];
        if (r.nodesOffset < 0 || (r.nodesOffset % kNodeBytes) != 0 || r.nodesBytes < kNodeBytes || (r.nodesBytes % kNodeBytes) != 0)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: nodesOffset and nodesBytes must be multiples of 64, nodesBytes at least 64", fn, k);
        if (r.nodesBytes > kMaxNodesBytes || r.nodesOffset > poolNodesBytes - r.nodesBytes)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: nodes [%lld, +%lld) lie outside the pool's %lld bytes or above Compact's 0x%llx", fn,
                             k, (long long)r.nodesOffset, (long long)r.nodesBytes, (long long)poolNodesBytes,
                             (unsigned long long)kMaxNodesBytes);
        ObEntry& E = table[(size_t)k];
        E.nodeBase = (int)(r.nodesOffset / kNodeBytes);
        E.numSlots = (int)(r.nodesBytes / kNodeBytes);
        E.rowBase = E.numRows = 0;
        if (rows) {
            if (r.triWoopOffset < 0 || (r.triWoopOffset % kRowBytes) != 0 || r.triWoopBytes < kRowBytes || (r.triWoopBytes % kRowBytes) != 0 ||
                r.triWoopBytes > poolTriWoopBytes || r.triWoopOffset > poolTriWoopBytes - r.triWoopBytes)
                return set_error(NTR_ERR_INVALID, "%s: entry %d: rows [%lld, +%lld) must be a positive multiple of 16 bytes inside the pool's "
                                 "%lld triWoop bytes", fn, k, (long long)r.triWoopOffset, (long long)r.triWoopBytes, (long long)poolTriWoopBytes);
            E.rowBase = (int)(r.triWoopOffset / kRowBytes);
            E.numRows = (int)(r.triWoopBytes / kRowBytes);
        }
        starts[(size_t)k] = (int)std::min<int64_t>(total, OB_MAX_SLOTS);
        total += E.numSlots;
        most = std::max<int64_t>(most, E.numSlots);
    }
    starts[(size_t)numEntries] = (int)std::min<int64_t>(total, OB_MAX_SLOTS);
    *totalSlots = total;
    *maxSlots = most;
    return NTR_OK;
}

struct ObDevice {                            // the scratch block as typed pointers
    int* firstHeights; OpRoot* reports; ObRound* round; ObCall* call; unsigned int *stats, *hist;
    int* starts; ObEntry* table;
    unsigned int *parent, *arrive; unsigned long long* info;
    int* height; unsigned int* leafLinks; int* qual; unsigned int* cursor; int* list;
    ObDevice(void* base, const ObLayout& l)
        : firstHeights(at<int>(base, l.firstHeights)), reports(at<OpRoot>(base, l.reports)), round(at<ObRound>(base, l.round)),
          call(at<ObCall>(base, l.call)), stats(at<unsigned int>(base, l.stats)), hist(at<unsigned int>(base, l.hist)),
          starts(at<int>(base, l.starts)), table(at<ObEntry>(base, l.table)), parent(at<unsigned int>(base, l.parent)),
          arrive(at<unsigned int>(base, l.arrive)), info(at<unsigned long long>(base, l.info)), height(at<int>(base, l.height)),
          leafLinks(at<unsigned int>(base, l.leafLinks)), qual(at<int>(base, l.qual)), cursor(at<unsigned int>(base, l.cursor)),
          list(at<int>(base, l.list))
    {
    }
};

// The reports and the round's record cleared, then ob_topology + ob_climb on stream s: two launches
template <bool SAH>
int ob_run_climb(hipStream_t s, int numEntries, int totalSlots, int maxSlots, const int* pool, const float4* poolWoop, const ObDevice& d)
{
    NTR_HIP(hipMemsetAsync(d.reports, 0, (size_t)numEntries * sizeof(OpRoot) + sizeof(ObRound), s));
    hipLaunchKernelGGL(ob_topology, dim3((unsigned int)(((int64_t)totalSlots + 1 + OP_BLOCK - 1) / OP_BLOCK)), dim3(OP_BLOCK), 0, s, numEntries,
                       totalSlots, maxSlots, (const int*)d.starts, (const ObEntry*)d.table, pool, d.parent, d.arrive,
                       SAH ? (int*)nullptr : d.height, SAH ? (unsigned int*)nullptr : d.hist, d.reports, d.call);
    hipLaunchKernelGGL(ob_climb<SAH>, dim3((unsigned int)((2ll * totalSlots + OP_BLOCK - 1) / OP_BLOCK)), dim3(OP_BLOCK), 0, s, numEntries,
                       totalSlots, (const int*)d.starts, (const ObEntry*)d.table, pool, poolWoop, (const unsigned int*)d.parent, d.arrive, d.info,
                       d.height, d.leafLinks, d.reports, d.round);
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_optimize_batch(int32_t numEntries, const NtrBlasRange* entries, void* d_poolNodes, int64_t poolNodesBytes, int32_t passes,
                           NtrBvhOptimizeBatchEntry* entryResults, NtrBvhOptimizeBatchResult* result, void* stream)
{
    const char* fn = "ntr_bvh_optimize_batch";
    if (result) memset(result, 0, sizeof(*result));
    std::vector<int> starts;
    std::vector<ObEntry> table;
    int64_t total = 0, maxSlots64 = 0;
    if (const int rc = ob_check(fn, numEntries, entries, d_poolNodes, poolNodesBytes, false, nullptr, 0, starts, table, &total, &maxSlots64))
        return rc;
    if (entryResults) memset(entryResults, 0, sizeof(*entryResults) * (size_t)numEntries);
    if (passes < 1 || passes > OP_MAX_PASSES) return set_error(NTR_ERR_INVALID, "%s: passes must be in 1..8", fn);
    // disjoint ranges inside a pool of at most kPoolMaxBytes keep the total below 2^26; overlapping ones are refused either way
    if (total > OB_MAX_SLOTS)
        return set_error(NTR_ERR_INVALID, "%s: the entries' node ranges are longer in all than a pool can be: some overlap", fn);
    {
        int other = -1;
        const int bad = first_range_overlap(numEntries, [&](int k) { return entries[k].nodesOffset; },
                                            [&](int k) { return entries[k].nodesBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the pool's nodes: a BLAS is restructured once per call", fn,
                             other, bad);
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads back per pass and cannot be captured", fn);

    const int totalSlots = (int)total, maxSlots = (int)maxSlots64;
    const ObLayout lay(numEntries, total, maxSlots, false);
    void* base = nullptr;
    if (const int rc = g_obPool.reserve(lay.end, &base)) return rc;
    const ObDevice d(base, lay);
    int* pool = (int*)d_poolNodes;
    const dim3 slotGrid((totalSlots + OP_BLOCK - 1) / OP_BLOCK);

    NtrBvhOptimizeBatchResult res = NtrBvhOptimizeBatchResult();
    res.numEntries = numEntries;
    res.passes = passes;
    res.firstBadEntry = -1;
    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    // (the host arrays outlive the uploads: the first read-back below waits for the stream)
    NTR_HIP(hipMemcpyAsync(d.starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemcpyAsync(d.table, table.data(), table.size() * sizeof(ObEntry), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemsetAsync(d.call, 0, sizeof(ObCall) + sizeof(unsigned int) * OP_STAT_SLOTS * OP_MAX_PASSES, s));

    // what a pass reads back in one copy: the round's record, the call's, the counters, the histogram's first words
    struct Head { ObRound round; ObCall call; unsigned int stats[OP_STAT_SLOTS * OP_MAX_PASSES]; };
    const size_t firstWords = std::min<size_t>((size_t)maxSlots + 1, OP_HIST_LDS);
    std::vector<unsigned char> headBuf(sizeof(Head) + 4 * firstWords);
    std::vector<unsigned int> hist;
    Head head;
    for (int pass = 0; pass <= passes; pass++) {   // the last round only measures the heights after the last pass
        const bool last = pass == passes;
        if (const int rc = ob_run_climb<false>(s, numEntries, totalSlots, maxSlots, pool, nullptr, d)) return rc;
        res.launches += 2;
        if (last) {
            NTR_HIP(ev.record(1));
            NTR_HIP(hipMemcpyAsync(&head, d.round, sizeof(Head), hipMemcpyDeviceToHost, s));
            NTR_HIP(hipStreamSynchronize(s));
            res.readBacks++;
            res.maxHeightAfter = (int32_t)head.round.tallest;
            break;
        }
        hipLaunchKernelGGL(ob_histogram, slotGrid, dim3(OP_BLOCK), 0, s, numEntries, totalSlots, (const int*)d.starts, (const ObEntry*)d.table,
                           (const int*)pool, (const unsigned int*)d.parent, (const int*)d.height, (const unsigned int*)d.leafLinks,
                           (const OpRoot*)d.reports, d.qual, d.hist, pass == 0 ? d.firstHeights : (int*)nullptr, d.call);
        hipLaunchKernelGGL(ob_scan, dim3(1), dim3(OP_BLOCK), 0, s, maxSlots, (const ObRound*)d.round, (const unsigned int*)d.hist, d.cursor);
        hipLaunchKernelGGL(ob_scatter, slotGrid, dim3(OP_BLOCK), 0, s, totalSlots, (const int*)d.qual, d.cursor, d.list);
        NTR_HIP(hipGetLastError());
        res.launches += 3;
        NTR_HIP(hipMemcpyAsync(headBuf.data(), d.round, headBuf.size(), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        res.readBacks++;
        memcpy(&head, headBuf.data(), sizeof(Head));
        hist.assign(firstWords, 0u);
        memcpy(hist.data(), headBuf.data() + sizeof(Head), 4 * firstWords);
        const int H = (int)head.round.tallest;   // 0: no entry has a tree under its slot 0
        if (H < 0 || H > maxSlots) return set_error(NTR_ERR_HIP, "%s: impossible tree height %d", fn, H);
        if (pass == 0) res.maxHeightBefore = H;
        if ((size_t)H + 1 > firstWords) {        // only a tree taller than OP_HIST_LDS
            hist.assign((size_t)H + 1, 0u);
            NTR_HIP(hipMemcpyAsync(hist.data(), d.hist, sizeof(unsigned int) * ((size_t)H + 1), hipMemcpyDeviceToHost, s));
            NTR_HIP(hipStreamSynchronize(s));
            res.readBacks++;
        }
        size_t off = 0;
        for (int hgt = 0; hgt <= H; hgt++) {
            const unsigned int cnt = hist[(size_t)hgt];
            if (off + cnt > (size_t)totalSlots) return set_error(NTR_ERR_HIP, "%s: inconsistent height histogram", fn);
            if (cnt && hgt > 0) {
                hipLaunchKernelGGL(ob_treelets, dim3(cnt), dim3(64), 0, s, numEntries, (const int*)d.starts, (const ObEntry*)d.table, pool,
                                   (const int*)d.list + off, (int)cnt, d.stats + (size_t)pass * OP_STAT_SLOTS);
                res.launches++;
            }
            off += cnt;
        }
        NTR_HIP(hipGetLastError());
        res.formed[pass] = (int64_t)off;
    }
    for (int pass = 0; pass < passes; pass++)
        for (int i = 0; i < OP_STAT_SLOTS; i++) res.rewritten[pass] += (int64_t)head.stats[pass * OP_STAT_SLOTS + i];
    res.errBits = (int32_t)head.call.err;
    res.firstBadEntry = head.call.err ? (int32_t)~head.call.bad : -1;
    if (entryResults) {
        const size_t bytes = (lay.round - lay.firstHeights);
        std::vector<unsigned char> buf(bytes);
        NTR_HIP(hipMemcpyAsync(buf.data(), d.firstHeights, bytes, hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        res.readBacks++;
        const int* fh = (const int*)buf.data();
        for (int k = 0; k < numEntries; k++) {
            OpRoot r;
            memcpy(&r, buf.data() + (lay.reports - lay.firstHeights) + sizeof(OpRoot) * (size_t)k, sizeof(r));
            NtrBvhOptimizeBatchEntry& o = entryResults[k];
            o.errBits = (int32_t)r.err;
            if (!r.done) {
                o.errBits |= NTR_OPT_ERR_NO_TREE;
                continue;
            }
            o.numNodes = (int32_t)(r.leafLinks - 1u);
            o.numLeafLinks = (int32_t)r.leafLinks;
            o.heightBefore = fh[k];
            o.heightAfter = (int32_t)r.height;
        }
    }
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    res.seconds = ms * 1e-3f;
    if (result) *result = res;
    if (head.call.err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed tree (error bits 0x%x over all entries: 1 a child link outside its BLAS's "
                         "extent, treated as a leaf link and never followed; 4 no tree under slot 0, the entry was left unchanged); every "
                         "other entry was optimised", fn, (int)~head.call.bad, head.call.err);
    return NTR_OK;
}

int ntr_bvh_optimize_batch_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_bvh_optimize_batch_scratch_bytes", g_obPool, bytes); }

int ntr_bvh_sah_cost_batch(int32_t numEntries, const NtrBlasRange* entries, const void* d_poolNodes, int64_t poolNodesBytes,
                           const void* d_poolTriWoop, int64_t poolTriWoopBytes, NtrBvhSahResult* entryResults, NtrBvhSahBatchResult* result,
                           void* stream)
{
    const char* fn = "ntr_bvh_sah_cost_batch";
    if (result) memset(result, 0, sizeof(*result));
    std::vector<int> starts;
    std::vector<ObEntry> table;
    int64_t total = 0, maxSlots64 = 0;
    if (const int rc = ob_check(fn, numEntries, entries, d_poolNodes, poolNodesBytes, true, d_poolTriWoop, poolTriWoopBytes, starts, table, &total,
                                &maxSlots64))
        return rc;
    if (!entryResults) return set_error(NTR_ERR_INVALID, "%s: null entryResults", fn);
    memset(entryResults, 0, sizeof(*entryResults) * (size_t)numEntries);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its results back and cannot be captured", fn);
    if (total > OB_MAX_SLOTS)
        return set_error(NTR_ERR_OVERFLOW, "%s: the entries list %lld node slots in all, more than the %lld of a pool of 0x%llx bytes", fn,
                         (long long)total, (long long)OB_MAX_SLOTS, (unsigned long long)kPoolMaxBytes);

    const int totalSlots = (int)total, maxSlots = (int)maxSlots64;
    const ObLayout lay(numEntries, total, maxSlots, true);
    void* base = nullptr;
    if (const int rc = g_obPool.reserve(lay.end, &base)) return rc;
    const ObDevice d(base, lay);
    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    NTR_HIP(hipMemcpyAsync(d.starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemcpyAsync(d.table, table.data(), table.size() * sizeof(ObEntry), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemsetAsync(d.call, 0, sizeof(ObCall), s));
    if (const int rc = ob_run_climb<true>(s, numEntries, totalSlots, maxSlots, (const int*)d_poolNodes, (const float4*)d_poolTriWoop, d)) return rc;
    NTR_HIP(ev.record(1));
    std::vector<OpRoot> reports((size_t)numEntries);
    NTR_HIP(hipMemcpyAsync(reports.data(), d.reports, reports.size() * sizeof(OpRoot), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    int firstBad = -1;
    unsigned int err = 0;
    for (int k = 0; k < numEntries; k++) {
        const OpRoot& r = reports[(size_t)k];
        const unsigned int bits = r.err | (r.done ? 0u : (unsigned int)NTR_OPT_ERR_NO_TREE);
        if (bits && firstBad < 0) firstBad = k;
        err |= bits;
        if (!r.done) continue;
        NtrBvhSahResult& o = entryResults[k];
        o.sahCost = r.sah;
        o.numNodes = (int32_t)r.slots;
        o.numLeaves = (int32_t)r.leaves;
        o.numTris = (int32_t)r.tris;
        o.height = (int32_t)r.height;
    }
    if (result) {
        result->numEntries = numEntries;
        result->firstBadEntry = firstBad;
        result->errBits = (int32_t)err;
        result->launches = 2;
        result->readBacks = 1;
        result->seconds = ms * 1e-3f;
    }
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed tree (error bits 0x%x over all entries: 1 child link, 2 leaf row outside the "
                         "entry's extents, 4 no tree under slot 0); such a child counts as 0, such an entry reads as zeros", fn, firstBad, err);
    return NTR_OK;
}

}  // extern "C"
