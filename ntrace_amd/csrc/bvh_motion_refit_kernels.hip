// bvh_motion_refit_kernels.hip -- the two-key refit of a BVHLayout_Compact tree for deformation motion blur on gfx950
// (ntr_bvh_motion_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_bvh_motion.py (motion_refit) -- np_bvh_refit.refit over the mesh at the shutter's
// opening (pos0, in place: the caller's nodes and Woop rows) and at its close (pos1, into a second node buffer), and beside them the
// triangles' vertices under either key as rows of (x, y, z, 0) that ntr_trace_bvh_motion poses at a ray's time.  The header comment of
// ntr_bvh_motion_refit (include/ntrace_amd.h) states the contract; DESIGN.md 6ae the shape.
// Built over the leaf pass of bvh_refit_leaf.h and the climb of bvh_climb.h, as bvh_refit_batch_kernels.hip is; bvh_refit_kernels.hip
// is not touched (bvh_refit_leaf.h says why that file stands alone).  Three launches, and a fourth of one thread when the scene box is
// asked for; no host read-back and no memset or copy node, so the call is asynchronous and capturable:
//   motion_prepare     one thread per node slot and per row: copies the slot to nodes1, makes the topology step of bvh_climb.h (the
//                      parent words serve both keys, each key has arrival counters of its own), zeroes its row of both vertex-row
//                      buffers
//   motion_climb<G, 0> key 0: refit_leaf_rows with the row rewrite over pos0, the leaf's vertex rows and terminator into vertRows0
//                      (bvh_motion_leaf.h, shared with bvh_motion_refit_batch_kernels.hip),
//                      refit_leaf_climb in nodes0
//   motion_climb<G, 1> key 1, a launch of its own AFTER key 0's: refit_leaf_rows without the rewrite (it reads the rows only to find the
//                      terminators, which key 0's launch has finished writing around) over pos1, vertRows1, the climb in nodes1
//   motion_scene_box   the union of the two roots' boxes in the total order
// A malformed tree is never followed: refit_leaf_rows sets an error bit and the group stops, so nothing outside the caller's buffers
// is touched; the vertex rows of a leaf are written only after its walk came through without an error.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_motion_leaf.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "level_build.h"
#include "refit_launch.h"

namespace ntr {
namespace {

constexpr int MR_BLOCK = 256;

// A counter slot of the blocking form (refit_launch.h)
struct MrStats {
    unsigned int innerLinks, leafLinks, rows, err;
    unsigned int pad[12];        // a slot per 64-byte line
};
static_assert(sizeof(MrStats) == 64, "MrStats must be 64 bytes");

DeviceScratchPool g_mrPool;

__global__ __launch_bounds__(MR_BLOCK) void motion_prepare(int numSlots, int numRows, const int* __restrict__ nodes0, int* __restrict__ nodes1,
                                                           unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive0,
                                                           unsigned int* __restrict__ arrive1, uint4* __restrict__ vertRows0,
                                                           uint4* __restrict__ vertRows1, MrStats* __restrict__ stats /* or null */)
{
    const unsigned int i = blockIdx.x * (unsigned int)MR_BLOCK + threadIdx.x;   // < max(numSlots, numRows) + MR_BLOCK < 2^31 + 256
    unsigned int inner = 0, leaf = 0, err = 0;
    if (i < (unsigned int)numSlots) {
        const uint4* src = reinterpret_cast<const uint4*>(nodes0 + (size_t)i * kNodeWords);
        uint4* dst = reinterpret_cast<uint4*>(nodes1 + (size_t)i * kNodeWords);
#pragma unroll
        for (int q = 0; q < 4; q++) dst[q] = src[q];
        int kind[2];
        topology_slot((int)i, numSlots, nodes0, parent, arrive0, kind);
        arrive1[i] = 0u;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            leaf += kind[k] == LINK_LEAF ? 1u : 0u;
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= RF_ERR_LINK;
        }
    }
    if (i < (unsigned int)numRows) {
        vertRows0[i] = make_uint4(0u, 0u, 0u, 0u);
        vertRows1[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (!stats) return;
    stats += blockIdx.x % kRefitStatSlots;
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

// G lanes share a leaf (bvh_refit_leaf.h); thread gid serves child slot gid / G, k = its low bit.  KEY1: the second key -- the rows are
// read only, and nothing is counted but errors (both keys walk the same leaves).
template <int G, bool KEY1>
__global__ __launch_bounds__(MR_BLOCK) void motion_climb(int numSlots, int* __restrict__ nodes, int numRows, float4* __restrict__ woop,
                                                         const int* __restrict__ triIndex, int numTris, const int* __restrict__ tri,
                                                         int numVerts, const float* __restrict__ pos, uint4* __restrict__ vertRows, float eps,
                                                         const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                         float* __restrict__ keyBox, MrStats* __restrict__ stats)
{
    const unsigned int gid = blockIdx.x * (unsigned int)MR_BLOCK + threadIdx.x;   // < 2 * numSlots * G + MR_BLOCK <= 2^29 + 256
    const int g = (int)(gid / G), sub = (int)(gid % G);
    const int groupShift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane
    const int node = g >> 1, k = g & 1;
    const int link = node < numSlots ? nodes[(size_t)node * kNodeWords + kLinkWord + k] : 0;
    const bool leaf = link < 0;                  // an inner child arrives with the owner of its node; offset 0 is no child at all
    unsigned int err = 0, rows = 0;
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // ord_enc words: min / max as integers
    if (leaf)                                    // uniform within a group
        refit_leaf_rows<G, !KEY1>(link, sub, groupShift, numRows, woop, triIndex, numTris, tri, numVerts, pos, err, rows, lo, hi);
    const unsigned int groupErr = leaf ? (unsigned int)((__ballot(err != 0) >> groupShift) & ((1ull << G) - 1ull)) : 0u;
    if (leaf && !groupErr) motion_leaf_vertex_rows<G>(link, sub, groupShift, numRows, woop, triIndex, tri, pos, vertRows);
    if (stats) {                                 // uniform; the whole wave is here: nobody has returned yet
        MrStats* mine = stats + blockIdx.x % kRefitStatSlots;
        const unsigned int waveRows = KEY1 ? 0u : wave_sum_u32(rows), waveErr = wave_or_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (waveRows) atomicAdd(&mine->rows, waveRows);
            if (waveErr) atomicOr(&mine->err, waveErr);
        }
    }
    if (!leaf || sub != 0 || groupErr) return;   // after an error the nodes above keep an arrival short and stay as they are
    refit_leaf_climb(node, k, numSlots, nodes, lo, hi, eps, parent, arrive, keyBox);
}

// min.xyz max.xyz of either key's root (refit_leaf_climb) -> their union
__global__ void motion_scene_box(const float* __restrict__ box0, const float* __restrict__ box1, float* __restrict__ sceneBox)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        sceneBox[q] = ord_min(box0[q], box1[q]);
        sceneBox[3 + q] = ord_max(box0[3 + q], box1[3 + q]);
    }
}

struct MrLayout {
    size_t stats, boxes, parent, arrive0, arrive1, end;
    explicit MrLayout(int64_t slots)
    {
        ScratchCarver c;
        stats = c.take(sizeof(MrStats) * kRefitStatSlots);
        boxes = c.take(12 * sizeof(float));
        parent = c.take((size_t)slots * 4);
        arrive0 = c.take((size_t)slots * 4);
        arrive1 = c.take((size_t)slots * 4);
        end = c.off;
    }
};

struct MrSpan { const char* name; uintptr_t at; uint64_t bytes; };

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_motion_refit(void* d_nodes0, int64_t nodesBytes, void* d_nodes1, void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                         int64_t triIndexBytes, void* d_vertRows0, void* d_vertRows1, int32_t numTris, const int32_t* d_triVtxIndex,
                         int32_t numVerts, const float* d_vtxPos0, const float* d_vtxPos1, float epsilon, float* d_sceneBox,
                         NtrBvhRefitResult* result, void* stream)
{
    const char* fn = "ntr_bvh_motion_refit";
    if (result) {
        result->numNodes = result->numLeaves = result->numRows = result->pad = 0;
    }
    // ntr_bvh_refit's checks, in its order
    if (!d_nodes0) return set_error(NTR_ERR_INVALID, "%s: null d_nodes0", fn);
    if (const int rc = check_nodes_bytes(fn, "nodesBytes", nodesBytes)) return rc;
    if (!d_triWoop) return set_error(NTR_ERR_INVALID, "%s: null d_triWoop", fn);
    if (triWoopBytes < 16 || (triWoopBytes % 16) != 0 || triWoopBytes / 16 > INT_MAX)
        return set_error(NTR_ERR_INVALID, "%s: triWoopBytes must be a positive multiple of 16 (at most 2^31 - 1 rows)", fn);
    if (!d_triIndex) return set_error(NTR_ERR_INVALID, "%s: null d_triIndex", fn);
    if (triIndexBytes < 0 || triIndexBytes * 4 < triWoopBytes)
        return set_error(NTR_ERR_INVALID, "%s: triIndexBytes must cover one entry per Woop row (triIndexBytes * 4 >= triWoopBytes)", fn);
    if (numTris < 1) return set_error(NTR_ERR_INVALID, "%s: numTris < 1", fn);
    if (!d_triVtxIndex) return set_error(NTR_ERR_INVALID, "%s: null d_triVtxIndex", fn);
    if (numVerts < 1) return set_error(NTR_ERR_INVALID, "%s: numVerts < 1", fn);
    if (!d_vtxPos0) return set_error(NTR_ERR_INVALID, "%s: null d_vtxPos0", fn);
    if (!std::isfinite(epsilon) || epsilon < 0.0f) return set_error(NTR_ERR_INVALID, "%s: epsilon must be finite and >= 0", fn);
    // the second key's buffers
    if (!d_nodes1) return set_error(NTR_ERR_INVALID, "%s: null d_nodes1", fn);
    if (!d_vertRows0) return set_error(NTR_ERR_INVALID, "%s: null d_vertRows0", fn);
    if (!d_vertRows1) return set_error(NTR_ERR_INVALID, "%s: null d_vertRows1", fn);
    if (!d_vtxPos1) return set_error(NTR_ERR_INVALID, "%s: null d_vtxPos1", fn);
    if (((uintptr_t)d_nodes0 | (uintptr_t)d_nodes1 | (uintptr_t)d_triWoop | (uintptr_t)d_vertRows0 | (uintptr_t)d_vertRows1) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: d_nodes0, d_nodes1, d_triWoop, d_vertRows0 and d_vertRows1 must be 16-byte aligned", fn);
    {
        const uint64_t meshBytes = 12ull * (uint64_t)numTris, posBytes = 12ull * (uint64_t)numVerts;
        const MrSpan fresh[4] = {{"d_nodes1", (uintptr_t)d_nodes1, (uint64_t)nodesBytes}, {"d_vertRows0", (uintptr_t)d_vertRows0, (uint64_t)triWoopBytes},
                                 {"d_vertRows1", (uintptr_t)d_vertRows1, (uint64_t)triWoopBytes}, {"d_vtxPos1", (uintptr_t)d_vtxPos1, posBytes}};
        const MrSpan old[6] = {{"d_nodes0", (uintptr_t)d_nodes0, (uint64_t)nodesBytes}, {"d_triWoop", (uintptr_t)d_triWoop, (uint64_t)triWoopBytes},
                               {"d_triIndex", (uintptr_t)d_triIndex, (uint64_t)triIndexBytes}, {"d_triVtxIndex", (uintptr_t)d_triVtxIndex, meshBytes},
                               {"d_vtxPos0", (uintptr_t)d_vtxPos0, posBytes}, {"d_sceneBox", (uintptr_t)d_sceneBox, d_sceneBox ? 24ull : 0ull}};
        auto meet = [](const MrSpan& a, const MrSpan& b) { return a.bytes && b.bytes && a.at < b.at + b.bytes && b.at < a.at + a.bytes; };
        for (int a = 0; a < 4; a++) {
            for (int b = 0; b < 6; b++)
                if (meet(fresh[a], old[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, old[b].name);
            for (int b = a + 1; b < 4; b++)
                if (meet(fresh[a], fresh[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, fresh[b].name);
        }
    }

    hipStream_t s = (hipStream_t)stream;
    const int numSlots = (int)(nodesBytes / kNodeBytes), numRows = (int)(triWoopBytes / kRowBytes);
    const MrLayout lay(numSlots);
    const bool capturing = stream_is_capturing(s);
    if (capturing && result) return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);
    if (capturing && g_mrPool.held() < lay.end)
        return set_error(NTR_ERR_INVALID, "%s: the scratch pool holds %zu B and this tree needs %zu B; a captured call cannot allocate -- "
                         "refit a tree at least as large once outside the capture", fn, g_mrPool.held(), lay.end);
    void* base = nullptr;
    if (const int rc = g_mrPool.reserve(lay.end, &base)) return rc;
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive0 = at<unsigned int>(base, lay.arrive0),
                 *arrive1 = at<unsigned int>(base, lay.arrive1);
    float* boxes = at<float>(base, lay.boxes);
    MrStats* stats = result ? at<MrStats>(base, lay.stats) : nullptr;

    // lanes per leaf from the mean leaf size the extents imply, by ntr_bvh_refit's thresholds: a choice of speed only
    const double meanTris = ((double)numRows - (double)(numSlots + 1)) / (3.0 * (double)(numSlots + 1));
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((2ll * numSlots * group + MR_BLOCK - 1) / MR_BLOCK));
    const int most = numSlots > numRows ? numSlots : numRows;
#define NTR_MR_CLIMB(G, KEY1, NODES, POS, VROWS, ARRIVE, BOX)                                                                                  \
    hipLaunchKernelGGL((motion_climb<G, KEY1>), grid, dim3(MR_BLOCK), 0, s, numSlots, (int*)(NODES), numRows, (float4*)d_triWoop, d_triIndex,  \
                       numTris, d_triVtxIndex, numVerts, POS, (uint4*)(VROWS), epsilon, (const unsigned int*)parent, ARRIVE, BOX, stats)
#define NTR_MR_KEYS(G)                                                                \
    do {                                                                              \
        NTR_MR_CLIMB(G, false, d_nodes0, d_vtxPos0, d_vertRows0, arrive0, boxes);     \
        NTR_MR_CLIMB(G, true, d_nodes1, d_vtxPos1, d_vertRows1, arrive1, boxes + 6);  \
    } while (0)
    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, stats, sizeof(MrStats) * kRefitStatSlots, &host, &seconds, [&] {
        hipLaunchKernelGGL(motion_prepare, dim3((unsigned int)(((long long)most + MR_BLOCK - 1) / MR_BLOCK)), dim3(MR_BLOCK), 0, s, numSlots,
                           numRows, (const int*)d_nodes0, (int*)d_nodes1, parent, arrive0, arrive1, (uint4*)d_vertRows0, (uint4*)d_vertRows1,
                           stats);
        if (group == 1) NTR_MR_KEYS(1); else if (group == 4) NTR_MR_KEYS(4); else NTR_MR_KEYS(8);
        if (d_sceneBox)
            hipLaunchKernelGGL(motion_scene_box, dim3(1), dim3(64), 0, s, (const float*)boxes, (const float*)(boxes + 6), d_sceneBox);
    });
#undef NTR_MR_KEYS
#undef NTR_MR_CLIMB
    if (rc != NTR_OK || !result) return rc;

    MrStats h = {};
    refit_fold_slots<MrStats>(host.data(), [&](const MrStats& v) {
        h.innerLinks += v.innerLinks; h.leafLinks += v.leafLinks; h.rows += v.rows; h.err |= v.err;
    });
    if (h.err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed tree (error 0x%x: 1 child link, 2 leaf row outside the extents, 4 triangle index, "
                         "8 vertex index out of range); the parts above it were left as they were", fn, h.err);
    result->numNodes = (int32_t)(1u + h.innerLinks);
    result->numLeaves = (int32_t)h.leafLinks;
    result->numRows = (int32_t)h.rows;
    result->seconds = seconds;
    return NTR_OK;
}

int ntr_bvh_motion_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_bvh_motion_refit_scratch_bytes", g_mrPool, bytes); }

}  // extern "C"
