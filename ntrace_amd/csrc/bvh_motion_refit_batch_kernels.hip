// bvh_motion_refit_batch_kernels.hip -- the two-key refit of many BLASes of a pool in one pass for gfx950 (ntr_bvh_motion_refit_batch).
//
// An EXTENSION: the rule is the numpy spec tests/np_motion_refit_batch.py -- np_bvh_motion.motion_refit over every entry's slices of the
// pool's five buffers -- and the header comment of ntr_bvh_motion_refit_batch (include/ntrace_amd.h) states the contract; DESIGN.md 6ah
// the shape.  ntr_bvh_motion_refit at pool + offset already writes the right bytes (a BLAS's links are relative to its own start,
// instanced_bvh.h); a pool of deforming meshes pays its three launches per BLAS.  Here they cover every listed BLAS:
//   motion_batch_prepare      one thread per listed node slot AND per listed row.  The two index spaces have entry edges of their own, so
//                             a thread finds its entry twice, in the running slot sums and in the running row sums.  As a slot: copies
//                             the slot to nodes1, makes the topology step of bvh_climb.h inside its BLAS (the parent words serve both
//                             keys, each key has arrival counters of its own).  As a row: zeroes its row of both vertex-row pools
//   motion_batch_climb<G, 0>  key 0: refit_leaf_rows with the row rewrite over pos0, the leaf's vertex rows and terminator into
//                             vertRows0 (bvh_motion_leaf.h), refit_leaf_climb in nodes0
//   motion_batch_climb<G, 1>  key 1, a launch of its own AFTER key 0's: refit_leaf_rows without the rewrite (it reads the rows only to
//                             find the terminators, which key 0's launch has finished writing around) over pos1, vertRows1, the climb in
//                             nodes1
//   motion_batch_boxes        only when the boxes are asked for: one thread per entry unites the two keys' root boxes in the total order
// The entry search is joint_entry_of (instanced_bvh.h), as in bvh_refit_batch_kernels.hip, whose header says why.  A group never spans
// two child slots, so none spans two BLASes.  The arrival protocol and its memory ordering are bvh_climb.h's and are not restated.  A
// malformed tree is never followed: the thread sets an error bit and stops; entries share no node, so every other entry is refitted
// completely; the vertex rows of a leaf are written only after its walk came through without an error.
// The held entry table, the refusals of a captured call, the bracket of the blocking form and the fold of its counter slots are
// refit_launch.h's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_motion_leaf.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_bvh.h"
#include "level_build.h"
#include "refit_launch.h"

namespace ntr {
namespace {

constexpr int MB_BLOCK = 256;
constexpr int MB_MAX_ENTRIES = 1 << 20;

// One listed BLAS as the kernels see it: 32 bytes.  The running sums are tables of their own (numEntries + 1 words each, the slot sums
// and behind them the row sums), dense for the search.
struct MbEntry {
    int nodeBase, numSlots;      // the BLAS's first node slot in the pool, its slots
    int rowBase, numRows;        // its first row (of triWoop, triIndex and both vertex-row pools), its rows
    int firstTri, numTris;       // its mesh
    float eps;
    int pad;
};
static_assert(sizeof(MbEntry) == 32, "MbEntry must be 32 bytes");

// A counter slot of the blocking form (refit_launch.h).  bad is the maximum of ~entry over the entries with an error, so 0 says none and the
// lowest entry wins.
struct MbStats {
    unsigned int innerLinks, leafLinks, rows, err, bad;
    unsigned int pad[11];        // a slot per 64-byte line
};
static_assert(sizeof(MbStats) == 64, "MbStats must be 64 bytes");

DeviceScratchPool g_mbPool;
RefitHeld g_mbHeld[kMaxDevices];

__global__ __launch_bounds__(MB_BLOCK) void motion_batch_prepare(int numEntries, int totalSlots, int totalRows, const int* __restrict__ slotStarts,
                                                                 const int* __restrict__ rowStarts, const MbEntry* __restrict__ table,
                                                                 const int* __restrict__ poolNodes0, int* __restrict__ poolNodes1,
                                                                 unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive0,
                                                                 unsigned int* __restrict__ arrive1, uint4* __restrict__ poolVertRows0,
                                                                 uint4* __restrict__ poolVertRows1, float* __restrict__ keyBoxes /* or null */,
                                                                 MbStats* __restrict__ stats /* or null: nothing is counted */)
{
    // < max(totalSlots, totalRows) + MB_BLOCK <= 2^28 + 256: disjoint ranges inside pools of at most kPoolMaxBytes
    const int i = (int)(blockIdx.x * (unsigned int)MB_BLOCK + threadIdx.x);
    unsigned int inner = 0, leaf = 0, err = 0;
    int e = 0;
    if (i < totalSlots) {
        e = joint_entry_of(slotStarts, numEntries, i);
        const int first = slotStarts[e], node = i - first;
        const MbEntry E = table[e];
        const int* nodes0 = poolNodes0 + (size_t)E.nodeBase * kNodeWords;
        const uint4* src = reinterpret_cast<const uint4*>(nodes0 + (size_t)node * kNodeWords);
        uint4* dst = reinterpret_cast<uint4*>(poolNodes1 + ((size_t)E.nodeBase + (size_t)node) * kNodeWords);
#pragma unroll
        for (int q = 0; q < 4; q++) dst[q] = src[q];
        int kind[2];
        topology_slot(node, E.numSlots, nodes0, parent + first, arrive0 + first, kind);
        arrive1[i] = 0u;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            leaf += kind[k] == LINK_LEAF ? 1u : 0u;
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= RF_ERR_LINK;
        }
        if (keyBoxes && node == 0) {             // empty (min > max) until a key's root is reached: motion_batch_boxes skips such an entry
#pragma unroll
            for (int q = 0; q < 12; q++) keyBoxes[12 * (size_t)e + q] = (q % 6) < 3 ? INFINITY : -INFINITY;
        }
    }
    if (i < totalRows) {                         // the row space has entry edges of its own
        const int er = joint_entry_of(rowStarts, numEntries, i);
        const size_t row = (size_t)table[er].rowBase + (size_t)(i - rowStarts[er]);
        poolVertRows0[row] = make_uint4(0u, 0u, 0u, 0u);
        poolVertRows1[row] = make_uint4(0u, 0u, 0u, 0u);
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

// G lanes share a leaf (bvh_refit_leaf.h); thread gid serves child slot gid / G of the listed slots, k = its low bit.  poolNodes, pos,
// poolVertRows, arrive and the box slot are the key's.  KEY1: the second key -- the Woop rows are read only, and nothing is counted but
// errors (both keys walk the same leaves).
template <int G, bool KEY1>
__global__ __launch_bounds__(MB_BLOCK) void motion_batch_climb(int numEntries, int totalSlots, const int* __restrict__ slotStarts,
                                                               const MbEntry* __restrict__ table, int* __restrict__ poolNodes,
                                                               float4* __restrict__ poolWoop, const int* __restrict__ poolTriIndex,
                                                               const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                               uint4* __restrict__ poolVertRows, const unsigned int* __restrict__ parent,
                                                               unsigned int* __restrict__ arrive, float* __restrict__ keyBoxes /* or null */,
                                                               MbStats* __restrict__ stats)
{
    const unsigned int gid = blockIdx.x * (unsigned int)MB_BLOCK + threadIdx.x;   // < 2 * totalSlots * G + MB_BLOCK <= 2^30 + 256
    const int g = (int)(gid / G), sub = (int)(gid % G);
    const int groupShift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane
    const int slot = g >> 1, k = g & 1;
    const bool live = slot < totalSlots;
    int e = 0, first = 0;
    MbEntry E = {};
    if (live) {
        e = joint_entry_of(slotStarts, numEntries, slot);
        first = slotStarts[e];
        E = table[e];
    }
    const int node = slot - first;
    int* nodes = poolNodes + (size_t)E.nodeBase * kNodeWords;
    const int link = live ? nodes[(size_t)node * kNodeWords + kLinkWord + k] : 0;
    const bool leaf = link < 0;                  // an inner child arrives with the owner of its node; offset 0 is no child at all
    unsigned int err = 0, rows = 0;
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // ord_enc words: min / max as integers
    const int* triE = tri + 3 * (size_t)E.firstTri;
    if (leaf)                                    // uniform within a group
        refit_leaf_rows<G, !KEY1>(link, sub, groupShift, E.numRows, poolWoop + E.rowBase, poolTriIndex + E.rowBase, E.numTris, triE, numVerts,
                                  pos, err, rows, lo, hi);
    const unsigned int groupErr = leaf ? (unsigned int)((__ballot(err != 0) >> groupShift) & ((1ull << G) - 1ull)) : 0u;
    if (leaf && !groupErr)
        motion_leaf_vertex_rows<G>(link, sub, groupShift, E.numRows, poolWoop + E.rowBase, poolTriIndex + E.rowBase, triE, pos,
                                   poolVertRows + E.rowBase);
    if (stats) {                                 // uniform; the whole wave is here: nobody has returned yet
        MbStats* mine = stats + blockIdx.x % kRefitStatSlots;
        if (err) atomicMax(&mine->bad, ~(unsigned int)e);
        const unsigned int waveRows = KEY1 ? 0u : wave_sum_u32(rows), waveErr = wave_or_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (waveRows) atomicAdd(&mine->rows, waveRows);
            if (waveErr) atomicOr(&mine->err, waveErr);
        }
    }
    if (!leaf || sub != 0 || groupErr) return;   // after an error the nodes above keep an arrival short and stay as they are
    refit_leaf_climb(node, k, E.numSlots, nodes, lo, hi, E.eps, parent + first, arrive + first,
                     keyBoxes ? keyBoxes + 12 * (size_t)e + (KEY1 ? 6 : 0) : nullptr);
}

// Entry e's two root boxes (min.xyz max.xyz each, refit_leaf_climb's) -> their union in entry order.  An entry one of whose roots was
// not reached (a malformed tree) still holds motion_batch_prepare's empty box there and its six floats stay as they are.
__global__ __launch_bounds__(MB_BLOCK) void motion_batch_boxes(int numEntries, const float* __restrict__ keyBoxes, float* __restrict__ blasBoxes)
{
    const int e = (int)(blockIdx.x * (unsigned int)MB_BLOCK + threadIdx.x);   // < numEntries + MB_BLOCK <= 2^20 + 256
    if (e >= numEntries) return;
    const float *b0 = keyBoxes + 12 * (size_t)e, *b1 = b0 + 6;
    if (b0[0] > b0[3] || b1[0] > b1[3]) return;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        blasBoxes[6 * (size_t)e + q] = ord_min(b0[q], b1[q]);
        blasBoxes[6 * (size_t)e + 3 + q] = ord_max(b0[3 + q], b1[3 + q]);
    }
}

struct MbLayout {
    size_t stats, starts, table, parent, arrive0, arrive1, boxes, end;
    MbLayout(int64_t entries, int64_t slots)
    {
        ScratchCarver c;
        stats = c.take(sizeof(MbStats) * kRefitStatSlots);
        starts = c.take((size_t)(entries + 1) * 8);   // the slot sums, then the row sums: one blob (refit_launch.h takes two)
        table = c.take((size_t)entries * sizeof(MbEntry));
        parent = c.take((size_t)slots * 4);
        arrive0 = c.take((size_t)slots * 4);
        arrive1 = c.take((size_t)slots * 4);
        boxes = c.take((size_t)entries * 12 * sizeof(float));
        end = c.off;
    }
};

struct MbSpan { const char* name; uintptr_t at; uint64_t bytes; };

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_motion_refit_batch(int32_t numEntries, const NtrRefitBatchEntry* entries, void* d_poolNodes0, int64_t poolNodesBytes,
                               void* d_poolNodes1, void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                               void* d_poolVertRows0, void* d_poolVertRows1, int32_t numTrisTotal, const int32_t* d_triVtxIndex,
                               int32_t numVerts, const float* d_vtxPos0, const float* d_vtxPos1, float* d_blasBoxes,
                               NtrBvhRefitBatchResult* result, void* stream)
{
    const char* fn = "ntr_bvh_motion_refit_batch";
    if (result) memset(result, 0, sizeof(*result));
    // ntr_bvh_refit_batch's checks, in its order
    if (numEntries < 1 || numEntries > MB_MAX_ENTRIES || !entries)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numEntries <= %d, a non-null entry array)", fn, MB_MAX_ENTRIES);
    if (!d_poolNodes0 || !d_poolTriWoop || !d_poolTriIndex || !d_triVtxIndex || !d_vtxPos0)
        return set_error(NTR_ERR_INVALID, "%s: null pool, mesh or vertex buffer", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (numTrisTotal < 1) return set_error(NTR_ERR_INVALID, "%s: numTrisTotal < 1", fn);
    if (numVerts < 1) return set_error(NTR_ERR_INVALID, "%s: numVerts < 1", fn);
    if (((uintptr_t)d_poolNodes0 | (uintptr_t)d_poolTriWoop) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the pool's nodes and triWoop must be 16-byte aligned", fn);

    RefitTable held = {2, {}, {0, 0}, {0, 0}};   // the two running sums, then the entries: 8 words each
    std::vector<uint32_t> &starts = held.words[0], &table = held.words[1];
    starts = std::vector<uint32_t>(2 * ((size_t)numEntries + 1));
    table = std::vector<uint32_t>((size_t)numEntries * (sizeof(MbEntry) / 4));
    uint32_t* rowStarts = starts.data() + (size_t)numEntries + 1;
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
        MbEntry E;
        E.nodeBase = (int)(en.range.nodesOffset / kNodeBytes);
        E.numSlots = (int)(en.range.nodesBytes / kNodeBytes);
        E.rowBase = (int)(en.range.triWoopOffset / kRowBytes);
        E.numRows = (int)(en.range.triWoopBytes / kRowBytes);
        E.firstTri = en.firstTri;
        E.numTris = en.numTris;
        E.eps = en.epsilon;
        E.pad = 0;
        memcpy(&table[(size_t)k * (sizeof(MbEntry) / 4)], &E, sizeof(E));
        starts[k] = (uint32_t)totalSlots;
        rowStarts[k] = (uint32_t)totalRows;
        totalSlots += E.numSlots;
        totalRows += E.numRows;
        // disjoint ranges inside a pool of at most kPoolMaxBytes keep totalSlots below 2^26 and totalRows below 2^28; overlapping ones
        // are refused below, but their sums must not wrap the tables' words first
        if (totalSlots > kPoolMaxBytes / kNodeBytes)
            return set_error(NTR_ERR_INVALID, "%s: the entries' node ranges are longer in all than a pool can be: some overlap", fn);
        if (totalRows > kPoolMaxBytes / kRowBytes)
            return set_error(NTR_ERR_INVALID, "%s: the entries' row ranges are longer in all than a pool can be: some overlap", fn);
    }
    starts[numEntries] = (uint32_t)totalSlots;
    rowStarts[numEntries] = (uint32_t)totalRows;
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
    // the second key's buffers
    if (!d_poolNodes1) return set_error(NTR_ERR_INVALID, "%s: null d_poolNodes1", fn);
    if (!d_poolVertRows0) return set_error(NTR_ERR_INVALID, "%s: null d_poolVertRows0", fn);
    if (!d_poolVertRows1) return set_error(NTR_ERR_INVALID, "%s: null d_poolVertRows1", fn);
    if (!d_vtxPos1) return set_error(NTR_ERR_INVALID, "%s: null d_vtxPos1", fn);
    if (((uintptr_t)d_poolNodes0 | (uintptr_t)d_poolNodes1 | (uintptr_t)d_poolTriWoop | (uintptr_t)d_poolVertRows0 | (uintptr_t)d_poolVertRows1) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: d_poolNodes0, d_poolNodes1, d_poolTriWoop, d_poolVertRows0 and d_poolVertRows1 must be 16-byte "
                         "aligned", fn);
    {   // ntr_bvh_motion_refit's span check over the pools' whole extents: what the call writes fresh meets nothing else of the call
        const uint64_t nodesB = (uint64_t)poolNodesBytes, rowsB = (uint64_t)poolTriWoopBytes;
        const uint64_t meshBytes = 12ull * (uint64_t)numTrisTotal, posBytes = 12ull * (uint64_t)numVerts;
        const MbSpan fresh[4] = {{"d_poolNodes1", (uintptr_t)d_poolNodes1, nodesB}, {"d_poolVertRows0", (uintptr_t)d_poolVertRows0, rowsB},
                                 {"d_poolVertRows1", (uintptr_t)d_poolVertRows1, rowsB}, {"d_vtxPos1", (uintptr_t)d_vtxPos1, posBytes}};
        const MbSpan old[6] = {{"d_poolNodes0", (uintptr_t)d_poolNodes0, nodesB}, {"d_poolTriWoop", (uintptr_t)d_poolTriWoop, rowsB},
                               {"d_poolTriIndex", (uintptr_t)d_poolTriIndex, rowsB / 4}, {"d_triVtxIndex", (uintptr_t)d_triVtxIndex, meshBytes},
                               {"d_vtxPos0", (uintptr_t)d_vtxPos0, posBytes},
                               {"d_blasBoxes", (uintptr_t)d_blasBoxes, d_blasBoxes ? 24ull * (uint64_t)numEntries : 0ull}};
        auto meet = [](const MbSpan& a, const MbSpan& b) { return a.bytes && b.bytes && a.at < b.at + b.bytes && b.at < a.at + a.bytes; };
        for (int a = 0; a < 4; a++) {
            for (int b = 0; b < 6; b++)
                if (meet(fresh[a], old[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, old[b].name);
            for (int b = a + 1; b < 4; b++)
                if (meet(fresh[a], fresh[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, fresh[b].name);
        }
    }

    hipStream_t s = (hipStream_t)stream;
    const MbLayout lay(numEntries, totalSlots);
    held.offset[0] = lay.starts;
    held.offset[1] = lay.table;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitEntryWords, g_mbPool, g_mbHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    const int* d_slotStarts = at<int>(base, lay.starts);
    const int* d_rowStarts = d_slotStarts + (size_t)numEntries + 1;
    const MbEntry* d_table = at<MbEntry>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive0 = at<unsigned int>(base, lay.arrive0),
                 *arrive1 = at<unsigned int>(base, lay.arrive1);
    float* keyBoxes = d_blasBoxes ? at<float>(base, lay.boxes) : nullptr;
    MbStats* stats = result ? at<MbStats>(base, lay.stats) : nullptr;

    const int slots = (int)totalSlots, rows = (int)totalRows;
    // lanes per leaf from the mean leaf size the selection's extents imply (a tree has one leaf more than inner nodes), by
    // ntr_bvh_refit's thresholds, as ntr_bvh_refit_batch: a choice of speed only
    const double leaves = (double)totalSlots + (double)numEntries;
    const double meanTris = ((double)totalRows - leaves) / (3.0 * leaves);
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((2ll * slots * group + MB_BLOCK - 1) / MB_BLOCK));
    const int most = slots > rows ? slots : rows;
#define NTR_MB_CLIMB(G, KEY1, NODES, POS, VROWS, ARRIVE)                                                                                       \
    hipLaunchKernelGGL((motion_batch_climb<G, KEY1>), grid, dim3(MB_BLOCK), 0, s, (int)numEntries, slots, d_slotStarts, d_table, (int*)(NODES), \
                       (float4*)d_poolTriWoop, d_poolTriIndex, d_triVtxIndex, numVerts, POS, (uint4*)(VROWS), (const unsigned int*)parent,    \
                       ARRIVE, keyBoxes, stats)
#define NTR_MB_KEYS(G)                                                                  \
    do {                                                                                \
        NTR_MB_CLIMB(G, false, d_poolNodes0, d_vtxPos0, d_poolVertRows0, arrive0);      \
        NTR_MB_CLIMB(G, true, d_poolNodes1, d_vtxPos1, d_poolVertRows1, arrive1);       \
    } while (0)
    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, stats, sizeof(MbStats) * kRefitStatSlots, &host, &seconds, [&] {
        hipLaunchKernelGGL(motion_batch_prepare, dim3((unsigned int)(((long long)most + MB_BLOCK - 1) / MB_BLOCK)), dim3(MB_BLOCK), 0, s,
                           (int)numEntries, slots, rows, d_slotStarts, d_rowStarts, d_table, (const int*)d_poolNodes0, (int*)d_poolNodes1, parent,
                           arrive0, arrive1, (uint4*)d_poolVertRows0, (uint4*)d_poolVertRows1, keyBoxes, stats);
        if (group == 1) NTR_MB_KEYS(1); else if (group == 4) NTR_MB_KEYS(4); else NTR_MB_KEYS(8);
        if (d_blasBoxes)
            hipLaunchKernelGGL(motion_batch_boxes, dim3((unsigned int)((numEntries + MB_BLOCK - 1) / MB_BLOCK)), dim3(MB_BLOCK), 0, s,
                               (int)numEntries, (const float*)keyBoxes, d_blasBoxes);
    });
#undef NTR_MB_KEYS
#undef NTR_MB_CLIMB
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0, rowsSeen = 0;
    unsigned int err = 0, bad = 0;
    refit_fold_slots<MbStats>(host.data(), [&](const MbStats& v) {
        inner += v.innerLinks; leafLinks += v.leafLinks; rowsSeen += v.rows; err |= v.err; bad = std::max(bad, v.bad);
    });
    result->numEntries = numEntries;
    result->lanesPerLeaf = group;
    result->numNodes = (int64_t)numEntries + (int64_t)inner;
    result->numLeaves = (int64_t)leafLinks;
    result->numRows = (int64_t)rowsSeen;
    result->firstBadEntry = err ? (int32_t)~bad : -1;
    result->errBits = (int32_t)err;
    result->seconds = seconds;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: entry %d: malformed tree (error bits 0x%x over all entries: 1 child link, 2 leaf row outside "
                         "the extents, 4 triangle index, 8 vertex index out of range); the parts above such a place were left as they were, "
                         "every other entry was refitted", fn, (int)~bad, err);
    return NTR_OK;
}

int ntr_bvh_motion_refit_batch_scratch_bytes(int64_t* bytes)
{
    return pool_bytes("ntr_bvh_motion_refit_batch_scratch_bytes", g_mbPool, bytes);
}

}  // extern "C"
