// wide_refit_batch_kernels.hip -- in-place refit of many 4-wide BLASes of a wide pool in one pass for gfx950 (ntr_pool_wide_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_wide_refit.py, and the header comment of ntr_pool_wide_refit (include/ntrace_amd.h)
// states the contract.  A wide BLAS (instanced_wide_bvh.h) shares its leaves -- Woop rows and triIndex -- with the binary BLAS it was
// widened from, and its links are relative to its own start.  ntr_pool_widen blocks, reads back and may give the tree another topology;
// a frame whose meshes deform only needs the boxes (and, for callers that trace wide only, the rows) again.  Two launches cover every
// listed wide BLAS and keep the topology:
//   wide_refit_prepare   one thread per wide node of all listed BLASes: the topology step of wide_climb.h inside the node's BLAS
//   wide_refit_climb     one thread, or a group of 4 or 8 lanes, per slot of all listed wide nodes: the leaf pass of bvh_refit_leaf.h
//                        (with or without the rewrite of the rows) and the climb of wide_climb.h with the BLAS's pointers
// A thread finds its entry by a binary search in the device table of running node sums, as bvh_refit_batch_kernels.hip's do.  A group
// never spans two slots, so none spans two BLASes.  The arrival protocol and its memory ordering are wide_climb.h's and are not
// restated.  A malformed tree is never followed: the thread sets an error bit and stops; entries share no node, so every other entry is
// refitted completely.
// No host read-back unless a result is asked for, and no memset node on the asynchronous path: the first launch re-initialises the
// arrival counters, and the counters of the blocking form, which is never captured, are the one memset.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "ntr_internal.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_wide_bvh.h"
#include "level_build.h"
#include "wide_climb.h"

namespace ntr {
namespace {

constexpr int WR_BLOCK = 256;
constexpr int WR_MAX_ENTRIES = 1 << 20;

// One listed wide BLAS as the kernels see it: 32 bytes.  The running node sums are a table of their own (numEntries + 1 words).
struct WrEntry {
    int nodeBase, numNodes;      // the BLAS's first wide node in the wide pool, its nodes
    int rowBase, numRows;        // its first Woop row (and triIndex entry), its rows
    int firstTri, numTris;       // its mesh
    float eps;
    int pad;
};
static_assert(sizeof(WrEntry) == 32, "WrEntry must be 32 bytes");

// Counters of the blocking form, as bvh_refit_batch_kernels.hip's: a workgroup adds to the slot of its number modulo WR_STAT_SLOTS and
// the host sums the slots.  bad is the maximum of ~entry over the entries with an error, so 0 says none and the lowest entry wins.
constexpr int WR_STAT_SLOTS = 256;
struct WrStats {
    unsigned int innerLinks, leafLinks, rows, err, bad;
    unsigned int pad[11];        // a slot per 64-byte line
};
static_assert(sizeof(WrStats) == 64, "WrStats must be 64 bytes");

DeviceScratchPool g_wrPool;

// The entry of listed node `node` (< starts[numEntries]): the last e with starts[e] <= node.  Every entry has a node, so starts rises strictly.
__device__ __forceinline__ int wr_entry_of(const int* __restrict__ starts, int numEntries, int node)
{
    int lo = 0, hi = numEntries;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= node) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(WR_BLOCK) void wide_refit_prepare(int numEntries, int totalNodes, const int* __restrict__ starts,
                                                               const WrEntry* __restrict__ table, const int* __restrict__ widePool,
                                                               unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                               WrStats* __restrict__ stats /* or null: nothing is counted */)
{
    const int idx = blockIdx.x * WR_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0;
    int e = 0;
    if (idx < totalNodes) {
        e = wr_entry_of(starts, numEntries, idx);
        const int first = starts[e];
        const WrEntry E = table[e];
        int kind[kWideChildren];
        if (!wide_topology_node(idx - first, E.numNodes, widePool + (size_t)E.nodeBase * kWideWords, parent + first, arrive + first, kind))
            err |= RF_ERR_LINK;
#pragma unroll
        for (int k = 0; k < kWideChildren; k++) {
            leaf += kind[k] == LINK_LEAF ? 1u : 0u;
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= RF_ERR_LINK;
        }
    }
    if (!stats) return;
    stats += blockIdx.x % WR_STAT_SLOTS;
    if (err) atomicMax(&stats->bad, ~(unsigned int)e);   // (rare) the entry is the lane's own: a wave covers several
    // one add per wave and counter
    inner = wave_sum_u32(inner);
    leaf = wave_sum_u32(leaf);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (inner) atomicAdd(&stats->innerLinks, inner);
        if (leaf) atomicAdd(&stats->leafLinks, leaf);
        if (err) atomicOr(&stats->err, err);
    }
}

// G lanes share a slot (bvh_refit_leaf.h); thread gid serves slot k = (gid / G) & 3 of listed node (gid / G) >> 2.
template <int G, bool REWRITE>
__global__ __launch_bounds__(WR_BLOCK) void wide_refit_climb(int numEntries, int totalNodes, const int* __restrict__ starts,
                                                             const WrEntry* __restrict__ table, int* __restrict__ widePool,
                                                             float4* __restrict__ poolWoop, const int* __restrict__ poolTriIndex,
                                                             const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                             const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                             float* __restrict__ blasBoxes /* or null */, WrStats* __restrict__ stats)
{
    const unsigned int gid = blockIdx.x * (unsigned int)WR_BLOCK + threadIdx.x;   // < 4 * totalNodes * G + WR_BLOCK <= 2^30 + 256
    const int g = (int)(gid / G), sub = (int)(gid % G);
    const int groupShift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane
    const int listed = g >> 2, k = g & 3;
    const bool live = listed < totalNodes;
    int e = 0, first = 0;
    WrEntry E = {};
    if (live) {
        e = wr_entry_of(starts, numEntries, listed);
        first = starts[e];
        E = table[e];
    }
    const int node = listed - first;
    int* nodes = widePool + (size_t)E.nodeBase * kWideWords;
    const int count = live ? nodes[(size_t)node * kWideWords + kWideCountWord] : 0;
    const bool slot = live && wide_count_ok(count) && k < count;   // a node with a bad count word has no slots (the first launch reported it)
    const int link = slot ? nodes[(size_t)node * kWideWords + kWideLinkWord + k] : 0;
    const bool leaf = link < 0;                  // uniform within a group
    unsigned int err = 0, rows = 0;
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // ord_enc words: min / max as integers
    if (leaf)
        refit_leaf_rows<G, REWRITE>(link, sub, groupShift, E.numRows, poolWoop + E.rowBase, poolTriIndex + E.rowBase, E.numTris,
                                    tri + 3 * (size_t)E.firstTri, numVerts, pos, err, rows, lo, hi);
    // a node named by two links: one namer's parent word was overwritten, and that namer says so (the first launch reported bad links)
    if (link > 0 && sub == 0 && is_wide_link(link, E.numNodes) && !wide_names_child(parent + first, node, k, link)) err |= RF_ERR_LINK;
    const unsigned int groupErr = leaf ? (unsigned int)((__ballot(err != 0) >> groupShift) & ((1ull << G) - 1ull)) : 0u;
    if (stats) {                                 // uniform; the whole wave is here: nobody has returned yet
        WrStats* mine = stats + blockIdx.x % WR_STAT_SLOTS;
        if (err) atomicMax(&mine->bad, ~(unsigned int)e);
        const unsigned int waveRows = wave_sum_u32(rows), waveErr = wave_or_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (waveRows) atomicAdd(&mine->rows, waveRows);
            if (waveErr) atomicOr(&mine->err, waveErr);
        }
    }
    // an inner slot arrives with the owner of its node; after an error the nodes above keep an arrival short and stay as they are
    if (!slot || link > 0 || sub != 0 || groupErr) return;
    if (leaf && lo[0] <= hi[0]) {                // some triangle was folded; a leaf without rows, like an empty slot, keeps its box words
        float box[6];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            box[2 * q] = ord_dec(lo[q]) - E.eps;
            box[2 * q + 1] = ord_dec(hi[q]) + E.eps;
        }
        wide_publish_box(nodes, node, k, box);
    }
    wide_climb(node, E.numNodes, nodes, parent + first, arrive + first, blasBoxes ? blasBoxes + 6 * (size_t)e : nullptr);
}

struct WrLayout {
    size_t stats, starts, table, parent, arrive, end;
    WrLayout(int64_t entries, int64_t nodes)
    {
        ScratchCarver c;
        stats = c.take(sizeof(WrStats) * WR_STAT_SLOTS);
        starts = c.take((size_t)(entries + 1) * 4);
        table = c.take((size_t)entries * sizeof(WrEntry));
        parent = c.take((size_t)nodes * 4);
        arrive = c.take((size_t)nodes * 4);
        end = c.off;
    }
};

// What the device's table holds, per device: the table the last call uploaded.  valid is cleared whenever the pool has been released
// or has to grow (the next call finds it smaller than it needs), so a table on the host never vouches for bytes that are gone.
struct WrUploaded {
    bool valid = false;
    std::vector<int> starts;
    std::vector<WrEntry> table;
};
WrUploaded g_wrUploaded[kMaxDevices];

// Two ranges [off, off + len) of the same buffer overlap: found by a sort over the entries' indices, not a quadratic scan
template <class Off, class Len>
int wr_first_overlap(int n, Off off, Len len, int* other)
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

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_pool_wide_refit(int32_t numEntries, const NtrWideRefitEntry* entries, void* d_widePoolNodes, int64_t widePoolNodesBytes,
                        void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, int32_t numTrisTotal,
                        const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos, int32_t rewriteRows, float* d_blasBoxes,
                        NtrWideRefitResult* result, void* stream)
{
    const char* fn = "ntr_pool_wide_refit";
    if (result) memset(result, 0, sizeof(*result));
    if (numEntries < 1 || numEntries > WR_MAX_ENTRIES || !entries)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numEntries <= %d, a non-null entry array)", fn, WR_MAX_ENTRIES);
    if (!d_widePoolNodes || !d_poolTriWoop || !d_poolTriIndex || !d_triVtxIndex || !d_vtxPos)
        return set_error(NTR_ERR_INVALID, "%s: null pool, mesh or vertex buffer", fn);
    if (const int rc = check_wide_pool_bytes(fn, "widePoolNodesBytes", widePoolNodesBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (numTrisTotal < 1) return set_error(NTR_ERR_INVALID, "%s: numTrisTotal < 1", fn);
    if (numVerts < 1) return set_error(NTR_ERR_INVALID, "%s: numVerts < 1", fn);
    if (rewriteRows != 0 && rewriteRows != 1) return set_error(NTR_ERR_INVALID, "%s: rewriteRows must be 0 or 1", fn);
    if (((uintptr_t)d_widePoolNodes | (uintptr_t)d_poolTriWoop) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the wide pool's nodes and the pool's triWoop must be 16-byte aligned", fn);
    if (!wide_box_granules_aligned()) return set_error(NTR_ERR_INVALID, "%s: a wide box is not three aligned 8-byte granules", fn);

    std::vector<int> starts((size_t)numEntries + 1);
    std::vector<WrEntry> table((size_t)numEntries);
    int64_t totalNodes = 0, totalTris = 0, totalLeaves = 0;
    for (int k = 0; k < numEntries; k++) {
        const NtrWideRefitEntry& en = entries[k];
        if (en.wideNodesOffset < 0 || (en.wideNodesOffset % kWideBytes) != 0 || en.wideNodesBytes < kWideBytes ||
            (en.wideNodesBytes % kWideBytes) != 0 || en.wideNodesBytes > kMaxWideBytes || en.wideNodesOffset > widePoolNodesBytes - en.wideNodesBytes)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: wide nodes [%lld, +%lld) must be multiples of 128, at most 0x%llx bytes, inside the "
                             "wide pool's %lld bytes", fn, k, (long long)en.wideNodesOffset, (long long)en.wideNodesBytes,
                             (unsigned long long)kMaxWideBytes, (long long)widePoolNodesBytes);
        if (en.triWoopOffset < 0 || (en.triWoopOffset % kRowBytes) != 0 || en.triWoopBytes < kRowBytes || (en.triWoopBytes % kRowBytes) != 0 ||
            en.triWoopOffset > poolTriWoopBytes - en.triWoopBytes)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: rows [%lld, +%lld) must be multiples of 16, at least one row, inside the pool's %lld "
                             "triWoop bytes", fn, k, (long long)en.triWoopOffset, (long long)en.triWoopBytes, (long long)poolTriWoopBytes);
        if (en.numTris < 1 || en.firstTri < 0 || (int64_t)en.firstTri + en.numTris > numTrisTotal)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: triangles [%d, +%d) must be at least one inside [0, %d)", fn, k, (int)en.firstTri,
                             (int)en.numTris, (int)numTrisTotal);
        if (!std::isfinite(en.epsilon) || en.epsilon < 0.0f)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: epsilon must be finite and >= 0", fn, k);
        WrEntry& E = table[k];
        E.nodeBase = (int)(en.wideNodesOffset / kWideBytes);
        E.numNodes = (int)(en.wideNodesBytes / kWideBytes);
        E.rowBase = (int)(en.triWoopOffset / kRowBytes);
        E.numRows = (int)(en.triWoopBytes / kRowBytes);
        E.firstTri = en.firstTri;
        E.numTris = en.numTris;
        E.eps = en.epsilon;
        E.pad = 0;
        starts[k] = (int)totalNodes;
        totalNodes += E.numNodes;
        // a leaf is a terminator row: rows = 3 * triangle references + leaves, and these builders reference a triangle once (a tree with
        // duplicated references reads as one of more, smaller leaves: a choice of speed only)
        totalTris += E.numTris;
        totalLeaves += std::max<int64_t>((int64_t)E.numRows - 3ll * E.numTris, 1);
        // disjoint ranges inside a pool of at most kPoolMaxBytes keep totalNodes below 2^25; overlapping ones are refused below, but
        // their sum must not wrap the table's words first
        if (totalNodes > kPoolMaxBytes / kWideBytes)
            return set_error(NTR_ERR_INVALID, "%s: the entries' node ranges are longer in all than a wide pool can be: some overlap", fn);
    }
    starts[numEntries] = (int)totalNodes;
    {
        int other = -1;
        int bad = wr_first_overlap(numEntries, [&](int k) { return entries[k].wideNodesOffset; },
                                   [&](int k) { return entries[k].wideNodesBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the wide pool's nodes: a BLAS is refitted once per call", fn, other, bad);
        bad = wr_first_overlap(numEntries, [&](int k) { return entries[k].triWoopOffset; },
                               [&](int k) { return entries[k].triWoopBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the pool's rows: a BLAS is refitted once per call", fn, other, bad);
    }

    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
    const WrLayout lay(numEntries, totalNodes);
    WrUploaded& up = g_wrUploaded[dev];
    if (g_wrPool.held() < lay.end) up.valid = false;   // released, never reserved, or about to be regrown
    const bool same = up.valid && up.starts == starts && up.table.size() == table.size() &&
                      memcmp(up.table.data(), table.data(), table.size() * sizeof(WrEntry)) == 0;
    const bool capturing = stream_is_capturing(s);
    if (capturing && result) return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);
    if (capturing && !same)
        return set_error(NTR_ERR_INVALID, "%s: a captured call uploads and allocates nothing: the device must hold this entry table already "
                         "-- make one uncaptured call with the same entries first (and none with other entries, and no "
                         "ntr_lbvh_release_workspace, between it and the capture)", fn);
    void* base = nullptr;
    if (const int rc = g_wrPool.reserve(lay.end, &base)) return rc;
    int* d_starts = at<int>(base, lay.starts);
    WrEntry* d_table = at<WrEntry>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    if (!same) {
        // the host copy is what the upload reads and what the next call compares with: the upload is waited for, so the copy never
        // changes under it.  A loop of calls with one table (a frame loop) pays this once
        up.valid = false;
        up.starts.swap(starts);
        up.table.swap(table);
        NTR_HIP(hipMemcpyAsync(d_starts, up.starts.data(), up.starts.size() * 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(d_table, up.table.data(), up.table.size() * sizeof(WrEntry), hipMemcpyHostToDevice, s));
        NTR_HIP(hipStreamSynchronize(s));
        up.valid = true;
    }
    WrStats* stats = result ? at<WrStats>(base, lay.stats) : nullptr;

    StreamEvents<2> ev(s);
    if (result) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
        NTR_HIP(hipMemsetAsync(stats, 0, sizeof(WrStats) * WR_STAT_SLOTS, s));
    }
    const int total = (int)totalNodes;
    hipLaunchKernelGGL(wide_refit_prepare, dim3((total + WR_BLOCK - 1) / WR_BLOCK), dim3(WR_BLOCK), 0, s, (int)numEntries, total,
                       (const int*)d_starts, (const WrEntry*)d_table, (const int*)d_widePoolNodes, parent, arrive, stats);
    // lanes per leaf from the selection's mean leaf size, by ntr_bvh_refit's thresholds -- the quantity ntr_bvh_refit_batch forms from
    // the binary extents, which a wide extent does not give: a choice of speed only
    const double meanTris = (double)totalTris / (double)totalLeaves;
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((4ll * total * group + WR_BLOCK - 1) / WR_BLOCK));
#define NTR_WR_CLIMB(G, RW)                                                                                                                 \
    hipLaunchKernelGGL((wide_refit_climb<G, RW>), grid, dim3(WR_BLOCK), 0, s, (int)numEntries, total, (const int*)d_starts,                \
                       (const WrEntry*)d_table, (int*)d_widePoolNodes, (float4*)d_poolTriWoop, d_poolTriIndex, d_triVtxIndex, numVerts,    \
                       d_vtxPos, (const unsigned int*)parent, arrive, d_blasBoxes, stats)
    if (rewriteRows) {
        if (group == 1) NTR_WR_CLIMB(1, true); else if (group == 4) NTR_WR_CLIMB(4, true); else NTR_WR_CLIMB(8, true);
    } else {
        if (group == 1) NTR_WR_CLIMB(1, false); else if (group == 4) NTR_WR_CLIMB(4, false); else NTR_WR_CLIMB(8, false);
    }
#undef NTR_WR_CLIMB
    NTR_HIP(hipGetLastError());
    if (!result) return NTR_OK;

    NTR_HIP(ev.record(1));
    std::vector<WrStats> slotsHost(WR_STAT_SLOTS);   // the copy is waited for right here
    NTR_HIP(hipMemcpyAsync(slotsHost.data(), stats, sizeof(WrStats) * WR_STAT_SLOTS, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    uint64_t inner = 0, leafLinks = 0, rows = 0;
    unsigned int err = 0, bad = 0;
    for (const WrStats& v : slotsHost) {
        inner += v.innerLinks; leafLinks += v.leafLinks; rows += v.rows; err |= v.err; bad = std::max(bad, v.bad);
    }
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->numEntries = numEntries;
    result->lanesPerLeaf = group;
    result->numNodes = (int64_t)numEntries + (int64_t)inner;
    result->numLeafLinks = (int64_t)leafLinks;
    result->numRows = (int64_t)rows;
    result->firstBadEntry = err ? (int32_t)~bad : -1;
    result->errBits = (int32_t)err;
    result->seconds = ms * 1e-3f;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed wide tree (error bits 0x%x over all entries: 1 a link that names no wide node, "
                         "a node named twice or a count word outside 2..4, 2 leaf row outside the extents, 4 triangle index, 8 vertex index "
                         "out of range); the parts above such a place were left as they were, every other entry was refitted", fn, (int)~bad,
                         err);
    return NTR_OK;
}

int ntr_pool_wide_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_pool_wide_refit_scratch_bytes", g_wrPool, bytes); }

}  // extern "C"
