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
// The held entry table, the refusals of a captured call, the bracket of the blocking form and the fold of its counter slots are
// refit_launch.h's.
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
#include "refit_launch.h"
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

// A counter slot of the blocking form (refit_launch.h).  bad is the maximum of ~entry over the entries with an error, so 0 says none and the
// lowest entry wins.
struct WrStats {
    unsigned int innerLinks, leafLinks, rows, err, bad;
    unsigned int pad[11];        // a slot per 64-byte line
};
static_assert(sizeof(WrStats) == 64, "WrStats must be 64 bytes");

DeviceScratchPool g_wrPool;
RefitHeld g_wrHeld[kMaxDevices];

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
    stats += blockIdx.x % kRefitStatSlots;
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
        WrStats* mine = stats + blockIdx.x % kRefitStatSlots;
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
        stats = c.take(sizeof(WrStats) * kRefitStatSlots);
        starts = c.take((size_t)(entries + 1) * 4);
        table = c.take((size_t)entries * sizeof(WrEntry));
        parent = c.take((size_t)nodes * 4);
        arrive = c.take((size_t)nodes * 4);
        end = c.off;
    }
};

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

    RefitTable held = {2, {}, {0, 0}, {0, 0}};   // the running sums, then the entries: 8 words each
    std::vector<uint32_t> &starts = held.words[0], &table = held.words[1];
    starts = std::vector<uint32_t>((size_t)numEntries + 1);
    table = std::vector<uint32_t>((size_t)numEntries * (sizeof(WrEntry) / 4));
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
        WrEntry E;
        E.nodeBase = (int)(en.wideNodesOffset / kWideBytes);
        E.numNodes = (int)(en.wideNodesBytes / kWideBytes);
        E.rowBase = (int)(en.triWoopOffset / kRowBytes);
        E.numRows = (int)(en.triWoopBytes / kRowBytes);
        E.firstTri = en.firstTri;
        E.numTris = en.numTris;
        E.eps = en.epsilon;
        E.pad = 0;
        memcpy(&table[(size_t)k * (sizeof(WrEntry) / 4)], &E, sizeof(E));
        starts[k] = (uint32_t)totalNodes;
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
    starts[numEntries] = (uint32_t)totalNodes;
    {
        int other = -1;
        int bad = first_range_overlap(numEntries, [&](int k) { return entries[k].wideNodesOffset; },
                                   [&](int k) { return entries[k].wideNodesBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the wide pool's nodes: a BLAS is refitted once per call", fn, other, bad);
        bad = first_range_overlap(numEntries, [&](int k) { return entries[k].triWoopOffset; },
                               [&](int k) { return entries[k].triWoopBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the pool's rows: a BLAS is refitted once per call", fn, other, bad);
    }

    hipStream_t s = (hipStream_t)stream;
    const WrLayout lay(numEntries, totalNodes);
    held.offset[0] = lay.starts;
    held.offset[1] = lay.table;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitEntryWords, g_wrPool, g_wrHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    int* d_starts = at<int>(base, lay.starts);
    WrEntry* d_table = at<WrEntry>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    WrStats* stats = result ? at<WrStats>(base, lay.stats) : nullptr;

    const int total = (int)totalNodes;
    // lanes per leaf from the selection's mean leaf size, by ntr_bvh_refit's thresholds -- the quantity ntr_bvh_refit_batch forms from
    // the binary extents, which a wide extent does not give: a choice of speed only
    const double meanTris = (double)totalTris / (double)totalLeaves;
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((4ll * total * group + WR_BLOCK - 1) / WR_BLOCK));
#define NTR_WR_CLIMB(G, RW)                                                                                                                 \
    hipLaunchKernelGGL((wide_refit_climb<G, RW>), grid, dim3(WR_BLOCK), 0, s, (int)numEntries, total, (const int*)d_starts,                \
                       (const WrEntry*)d_table, (int*)d_widePoolNodes, (float4*)d_poolTriWoop, d_poolTriIndex, d_triVtxIndex, numVerts,    \
                       d_vtxPos, (const unsigned int*)parent, arrive, d_blasBoxes, stats)
    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, stats, sizeof(WrStats) * kRefitStatSlots, &host, &seconds, [&] {
        hipLaunchKernelGGL(wide_refit_prepare, dim3((total + WR_BLOCK - 1) / WR_BLOCK), dim3(WR_BLOCK), 0, s, (int)numEntries, total,
                           (const int*)d_starts, (const WrEntry*)d_table, (const int*)d_widePoolNodes, parent, arrive, stats);
        if (rewriteRows) {
            if (group == 1) NTR_WR_CLIMB(1, true); else if (group == 4) NTR_WR_CLIMB(4, true); else NTR_WR_CLIMB(8, true);
        } else {
            if (group == 1) NTR_WR_CLIMB(1, false); else if (group == 4) NTR_WR_CLIMB(4, false); else NTR_WR_CLIMB(8, false);
        }
    });
#undef NTR_WR_CLIMB
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0, rows = 0;
    unsigned int err = 0, bad = 0;
    refit_fold_slots<WrStats>(host.data(), [&](const WrStats& v) {
        inner += v.innerLinks; leafLinks += v.leafLinks; rows += v.rows; err |= v.err; bad = std::max(bad, v.bad);
    });
    result->numEntries = numEntries;
    result->lanesPerLeaf = group;
    result->numNodes = (int64_t)numEntries + (int64_t)inner;
    result->numLeafLinks = (int64_t)leafLinks;
    result->numRows = (int64_t)rows;
    result->firstBadEntry = err ? (int32_t)~bad : -1;
    result->errBits = (int32_t)err;
    result->seconds = seconds;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed wide tree (error bits 0x%x over all entries: 1 a link that names no wide node, "
                         "a node named twice or a count word outside 2..4, 2 leaf row outside the extents, 4 triangle index, 8 vertex index "
                         "out of range); the parts above such a place were left as they were, every other entry was refitted", fn, (int)~bad,
                         err);
    return NTR_OK;
}

int ntr_pool_wide_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_pool_wide_refit_scratch_bytes", g_wrPool, bytes); }

}  // extern "C"
