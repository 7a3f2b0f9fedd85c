// bvh_refit_batch_kernels.hip -- on-device refit of many BLASes of a pool in one pass for gfx950 (ntr_bvh_refit_batch).
//
// An EXTENSION: the rule is the numpy spec tests/np_refit_batch.py -- np_bvh_refit.refit over every entry's slices of the pool -- and the
// header comment of ntr_bvh_refit_batch (include/ntrace_amd.h) states the contract.  A BLAS is byte for byte a Compact tree whose links
// are relative to its own start (instanced_bvh.h), so ntr_bvh_refit at pool + offset already writes the right bytes; a pool of a
// thousand deforming meshes pays its two launches a thousand times.  Here the two launches cover every listed BLAS:
//   refit_batch_topology   one thread per node slot of all listed BLASes: the topology step of bvh_climb.h inside the slot's BLAS
//   refit_batch_climb      one thread, or a group of 4 or 8 lanes, per child slot of all listed BLASes: the leaf pass of
//                          bvh_refit_leaf.h and the climb of bvh_climb.h with the BLAS's pointers and its own numSlots
// A thread finds its entry by a binary search in the device table of running slot sums (at most 20 steps over a table that a wave's
// lanes walk together and the L2 holds; a per-slot entry word written by the first launch would cost 4 B per slot and a dependent
// load of its own).  A group never spans two child slots, so none spans two BLASes.  The arrival protocol and its memory ordering are
// bvh_climb.h's and are not restated.  A malformed tree is never followed: the thread sets an error bit and stops; entries share no
// node, so every other entry is refitted completely.
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
#include "bvh_climb.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_bvh.h"
#include "level_build.h"
#include "refit_launch.h"

namespace ntr {
namespace {

constexpr int RB_BLOCK = 256;
constexpr int RB_MAX_ENTRIES = 1 << 20;

// One listed BLAS as the kernels see it: 32 bytes.  The running slot sums are a table of their own (numEntries + 1 words), dense for
// the search.
struct RbEntry {
    int nodeBase, numSlots;      // the BLAS's first node slot in the pool, its slots
    int rowBase, numRows;        // its first Woop row (and triIndex entry), its rows
    int firstTri, numTris;       // its mesh
    float eps;
    int pad;
};
static_assert(sizeof(RbEntry) == 32, "RbEntry must be 32 bytes");

// A counter slot of the blocking form (refit_launch.h).  bad is the maximum of ~entry over the entries with an error, so 0 says none and the
// lowest entry wins.
struct RbStats {
    unsigned int innerLinks, leafLinks, rows, err, bad;
    unsigned int pad[11];        // a slot per 64-byte line
};
static_assert(sizeof(RbStats) == 64, "RbStats must be 64 bytes");

DeviceScratchPool g_rbPool;
RefitHeld g_rbHeld[kMaxDevices];

__global__ __launch_bounds__(RB_BLOCK) void refit_batch_topology(int numEntries, int totalSlots, const int* __restrict__ starts,
                                                                 const RbEntry* __restrict__ table, const int* __restrict__ poolNodes,
                                                                 unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                                 RbStats* __restrict__ stats /* or null: nothing is counted */)
{
    const int slot = blockIdx.x * RB_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0;
    int e = 0;
    if (slot < totalSlots) {
        e = joint_entry_of(starts, numEntries, slot);
        const int first = starts[e];
        const RbEntry E = table[e];
        int kind[2];
        topology_slot(slot - first, E.numSlots, poolNodes + (size_t)E.nodeBase * kNodeWords, parent + first, arrive + first, kind);
#pragma unroll
        for (int k = 0; k < 2; k++) {
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

// G lanes share a leaf (bvh_refit_leaf.h); thread gid serves child slot gid / G of the listed slots, k = its low bit.
template <int G>
__global__ __launch_bounds__(RB_BLOCK) void refit_batch_climb(int numEntries, int totalSlots, const int* __restrict__ starts,
                                                              const RbEntry* __restrict__ table, int* __restrict__ poolNodes,
                                                              float4* __restrict__ poolWoop, const int* __restrict__ poolTriIndex,
                                                              const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                              const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                              float* __restrict__ blasBoxes /* or null */, RbStats* __restrict__ stats)
{
    const unsigned int gid = blockIdx.x * (unsigned int)RB_BLOCK + threadIdx.x;   // < 2 * totalSlots * G + RB_BLOCK <= 2^30 + 256
    const int g = (int)(gid / G), sub = (int)(gid % G);
    const int groupShift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane
    const int slot = g >> 1, k = g & 1;
    const bool live = slot < totalSlots;
    int e = 0, first = 0;
    RbEntry E = {};
    if (live) {
        e = joint_entry_of(starts, numEntries, slot);
        first = starts[e];
        E = table[e];
    }
    const int node = slot - first;
    int* nodes = poolNodes + (size_t)E.nodeBase * kNodeWords;
    const int link = live ? nodes[(size_t)node * kNodeWords + kLinkWord + k] : 0;
    const bool leaf = link < 0;                  // an inner child arrives with the owner of its node; offset 0 is no child at all
    unsigned int err = 0, rows = 0;
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // ord_enc words: min / max as integers
    if (leaf)                                    // uniform within a group
        refit_leaf_rows<G>(link, sub, groupShift, E.numRows, poolWoop + E.rowBase, poolTriIndex + E.rowBase, E.numTris,
                           tri + 3 * (size_t)E.firstTri, numVerts, pos, err, rows, lo, hi);
    const unsigned int groupErr = leaf ? (unsigned int)((__ballot(err != 0) >> groupShift) & ((1ull << G) - 1ull)) : 0u;
    if (stats) {                                 // uniform; the whole wave is here: nobody has returned yet
        RbStats* mine = stats + blockIdx.x % kRefitStatSlots;
        if (err) atomicMax(&mine->bad, ~(unsigned int)e);
        const unsigned int waveRows = wave_sum_u32(rows), waveErr = wave_or_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (waveRows) atomicAdd(&mine->rows, waveRows);
            if (waveErr) atomicOr(&mine->err, waveErr);
        }
    }
    if (!leaf || sub != 0 || groupErr) return;   // after an error the nodes above keep an arrival short and stay as they are
    refit_leaf_climb(node, k, E.numSlots, nodes, lo, hi, E.eps, parent + first, arrive + first, blasBoxes ? blasBoxes + 6 * (size_t)e : nullptr);
}

struct RbLayout {
    size_t stats, starts, table, parent, arrive, end;
    RbLayout(int64_t entries, int64_t slots)
    {
        ScratchCarver c;
        stats = c.take(sizeof(RbStats) * kRefitStatSlots);
        starts = c.take((size_t)(entries + 1) * 4);
        table = c.take((size_t)entries * sizeof(RbEntry));
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        end = c.off;
    }
};

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_refit_batch(int32_t numEntries, const NtrRefitBatchEntry* entries, void* d_poolNodes, int64_t poolNodesBytes,
                        void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, int32_t numTrisTotal,
                        const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos, float* d_blasBoxes,
                        NtrBvhRefitBatchResult* result, void* stream)
{
    const char* fn = "ntr_bvh_refit_batch";
    if (result) memset(result, 0, sizeof(*result));
    if (numEntries < 1 || numEntries > RB_MAX_ENTRIES || !entries)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numEntries <= %d, a non-null entry array)", fn, RB_MAX_ENTRIES);
    if (!d_poolNodes || !d_poolTriWoop || !d_poolTriIndex || !d_triVtxIndex || !d_vtxPos)
        return set_error(NTR_ERR_INVALID, "%s: null pool, mesh or vertex buffer", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (numTrisTotal < 1) return set_error(NTR_ERR_INVALID, "%s: numTrisTotal < 1", fn);
    if (numVerts < 1) return set_error(NTR_ERR_INVALID, "%s: numVerts < 1", fn);
    if (((uintptr_t)d_poolNodes | (uintptr_t)d_poolTriWoop) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the pool's nodes and triWoop must be 16-byte aligned", fn);

    RefitTable held = {2, {}, {0, 0}, {0, 0}};   // the running sums, then the entries: 8 words each
    std::vector<uint32_t> &starts = held.words[0], &table = held.words[1];
    starts = std::vector<uint32_t>((size_t)numEntries + 1);
    table = std::vector<uint32_t>((size_t)numEntries * (sizeof(RbEntry) / 4));
    int64_t totalSlots = 0, totalRows = 0;
    for (int k = 0; k < numEntries; k++) {
        const NtrRefitBatchEntry& en = entries[k];
        if (const int rc = check_blas_range(fn, k, en.range, poolNodesBytes)) return rc;
        if (en.range.triWoopOffset > poolTriWoopBytes - en.range.triWoopBytes)
            return set_error(NTR_ERR_INVALID, "%s: BLAS %d: rows [%lld, +%lld) lie outside the pool's %lld triWoop bytes", fn, k,
                             (long long)en.range.triWoopOffset, (long long)en.range.triWoopBytes, (long long)poolTriWoopBytes);
        if (en.numTris < 1 || en.firstTri < 0 || (int64_t)en.firstTri + en.numTris > numTrisTotal)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: triangles [%d, +%d) must be at least one inside [0, %d)", fn, k, (int)en.firstTri,
                             (int)en.numTris, (int)numTrisTotal);
        if (!std::isfinite(en.epsilon) || en.epsilon < 0.0f)
            return set_error(NTR_ERR_INVALID, "%s: entry %d: epsilon must be finite and >= 0", fn, k);
        RbEntry E;
        E.nodeBase = (int)(en.range.nodesOffset / kNodeBytes);
        E.numSlots = (int)(en.range.nodesBytes / kNodeBytes);
        E.rowBase = (int)(en.range.triWoopOffset / kRowBytes);
        E.numRows = (int)(en.range.triWoopBytes / kRowBytes);
        E.firstTri = en.firstTri;
        E.numTris = en.numTris;
        E.eps = en.epsilon;
        E.pad = 0;
        memcpy(&table[(size_t)k * (sizeof(RbEntry) / 4)], &E, sizeof(E));
        starts[k] = (uint32_t)totalSlots;
        totalSlots += E.numSlots;
        totalRows += E.numRows;
        // disjoint ranges inside a pool of at most kPoolMaxBytes keep totalSlots below 2^26; overlapping ones are refused below, but
        // their sum must not wrap the table's words first
        if (totalSlots > kPoolMaxBytes / kNodeBytes)
            return set_error(NTR_ERR_INVALID, "%s: the entries' node ranges are longer in all than a pool can be: some overlap", fn);
    }
    starts[numEntries] = (uint32_t)totalSlots;
    {
        int other = -1;
        int bad = first_range_overlap(numEntries, [&](int k) { return entries[k].range.nodesOffset; },
                                   [&](int k) { return entries[k].range.nodesBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the pool's nodes: a BLAS is refitted once per call", fn, other, bad);
        bad = first_range_overlap(numEntries, [&](int k) { return entries[k].range.triWoopOffset; },
                               [&](int k) { return entries[k].range.triWoopBytes; }, &other);
        if (bad >= 0)
            return set_error(NTR_ERR_INVALID, "%s: entries %d and %d overlap in the pool's rows: a BLAS is refitted once per call", fn, other, bad);
    }

    hipStream_t s = (hipStream_t)stream;
    const RbLayout lay(numEntries, totalSlots);
    held.offset[0] = lay.starts;
    held.offset[1] = lay.table;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitEntryWords, g_rbPool, g_rbHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    int* d_starts = at<int>(base, lay.starts);
    RbEntry* d_table = at<RbEntry>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    RbStats* stats = result ? at<RbStats>(base, lay.stats) : nullptr;

    const int slots = (int)totalSlots;
    // lanes per leaf from the mean leaf size the selection's extents imply (a tree has one leaf more than inner nodes), by
    // ntr_bvh_refit's thresholds: a choice of speed only
    const double leaves = (double)totalSlots + (double)numEntries;
    const double meanTris = ((double)totalRows - leaves) / (3.0 * leaves);
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((2ll * slots * group + RB_BLOCK - 1) / RB_BLOCK));
#define NTR_RB_CLIMB(G)                                                                                                                    \
    hipLaunchKernelGGL(refit_batch_climb<G>, grid, dim3(RB_BLOCK), 0, s, (int)numEntries, slots, (const int*)d_starts, (const RbEntry*)d_table, \
                       (int*)d_poolNodes, (float4*)d_poolTriWoop, d_poolTriIndex, d_triVtxIndex, numVerts, d_vtxPos,                        \
                       (const unsigned int*)parent, arrive, d_blasBoxes, stats)
    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, stats, sizeof(RbStats) * kRefitStatSlots, &host, &seconds, [&] {
        hipLaunchKernelGGL(refit_batch_topology, dim3((slots + RB_BLOCK - 1) / RB_BLOCK), dim3(RB_BLOCK), 0, s, (int)numEntries, slots,
                           (const int*)d_starts, (const RbEntry*)d_table, (const int*)d_poolNodes, parent, arrive, stats);
        if (group == 1) NTR_RB_CLIMB(1); else if (group == 4) NTR_RB_CLIMB(4); else NTR_RB_CLIMB(8);
    });
#undef NTR_RB_CLIMB
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0, rows = 0;
    unsigned int err = 0, bad = 0;
    refit_fold_slots<RbStats>(host.data(), [&](const RbStats& v) {
        inner += v.innerLinks; leafLinks += v.leafLinks; rows += v.rows; err |= v.err; bad = std::max(bad, v.bad);
    });
    result->numEntries = numEntries;
    result->lanesPerLeaf = group;
    result->numNodes = (int64_t)numEntries + (int64_t)inner;
    result->numLeaves = (int64_t)leafLinks;
    result->numRows = (int64_t)rows;
    result->firstBadEntry = err ? (int32_t)~bad : -1;
    result->errBits = (int32_t)err;
    result->seconds = seconds;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed tree (error bits 0x%x over all entries: 1 child link, 2 leaf row outside "
                         "the extents, 4 triangle index, 8 vertex index out of range); the parts above such a place were left as they were, "
                         "every other entry was refitted", fn, (int)~bad, err);
    return NTR_OK;
}

int ntr_bvh_refit_batch_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_bvh_refit_batch_scratch_bytes", g_rbPool, bytes); }

}  // extern "C"
