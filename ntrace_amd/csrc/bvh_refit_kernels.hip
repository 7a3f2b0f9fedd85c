// bvh_refit_kernels.hip -- on-device refit of a BVHLayout_Compact tree to moved vertices for gfx950 (ntr_bvh_refit).
//
// An EXTENSION: the reference has no refit (its scenes are static).  The rule is the numpy spec tests/np_bvh_refit.py, whose docstring
// is the normative text; the header comment of ntr_bvh_refit (include/ntrace_amd.h) restates the contract.  In short: the topology
// stays (child words, split word, leaf terminators, triIndex); every triangle's Woop rows are woop_rows.h over the new positions; a
// leaf child's box is the min / max over its triangles' vertices, -/+ epsilon; an inner child's box is the union of the two boxes
// stored in that child's node; min and max in the total order -0 < +0, so no result depends on the order of the operands.
//
// Shape: two launches, no host read-back, so the call is asynchronous and can be captured into a HIP graph.  All per-call state is
// re-initialised by the first launch, not by a memset node (memset nodes were observed not to re-execute on a graph replay; the
// counters of the blocking form, which is never captured, are the one exception).
//   refit_topology   one thread per node slot: the topology step of bvh_climb.h; counts the links for the result
//   refit_climb      one thread, or a group of 4 or 8 lanes, per child slot that holds a leaf: walks the leaf's row groups to the
//                    terminator, writes their Woop rows, folds the box, writes it into its slot of the parent's node and climbs
//                    (bvh_climb.h: the second arrival at a node forms the union and carries it to the grandparent's slot)
// The layout is compact_bvh.h's; the arrival protocol and its memory ordering are stated in bvh_climb.h and live only there.  The
// payload here is a child's box inside its parent's node.  Every access other than the payload's is to bytes that no other thread of
// the launch writes (link words, rows, triIndex, the mesh, the parent words of the previous launch) and is a plain access.
// A malformed tree (a link or row outside the extents, a triangle or vertex index out of range) is never followed: the thread sets an
// error bit and stops, so nothing outside the caller's buffers is touched.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <mutex>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "woop_rows.h"

namespace ntr {
namespace {

constexpr int RF_BLOCK = 256;
enum : unsigned int { RF_ERR_LINK = 1u, RF_ERR_ROW = 2u, RF_ERR_TRI = 4u, RF_ERR_VERTEX = 8u };

// Counters of the blocking form, first block of the scratch; zeroed and read back by that form only.  A workgroup adds to the slot of
// its number modulo RF_STAT_SLOTS and the host sums the slots: adds to ONE word from every wave serialise at about 10 ns each (the
// topology pass of a 520 k-node tree took 188 us that way instead of 8 us).
constexpr int RF_STAT_SLOTS = 256;
struct RfStats {
    unsigned int innerLinks, leafLinks, rows, err;
    unsigned int pad[12];    // a slot per 64-byte line
};
static_assert(sizeof(RfStats) == 64, "RfStats must be 64 bytes");

DeviceScratchPool g_rfPool;

// A child's box inside its parent's node (box_word, compact_bvh.h) is three aligned 8-byte granules: components 0-1, 2-3 and 4-5.
// Published and read at agent scope (write-through stores, loads past the L1), as agg_store_slot / agg_load_slot.
__device__ __forceinline__ void rf_publish_box(int* nodes, int node, int k, const float (&b)[6])
{
    unsigned long long* p = reinterpret_cast<unsigned long long*>(nodes + (size_t)node * kNodeWords);
    const unsigned long long w0 = (unsigned long long)__float_as_uint(b[0]) | ((unsigned long long)__float_as_uint(b[1]) << 32);
    const unsigned long long w1 = (unsigned long long)__float_as_uint(b[2]) | ((unsigned long long)__float_as_uint(b[3]) << 32);
    const unsigned long long w2 = (unsigned long long)__float_as_uint(b[4]) | ((unsigned long long)__float_as_uint(b[5]) << 32);
    __hip_atomic_store(p + box_word(k, 0) / 2, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + box_word(k, 2) / 2, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + box_word(k, 4) / 2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rf_acquire_box(const int* nodes, int node, int k, float (&b)[6])
{
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(nodes + (size_t)node * kNodeWords);
    const unsigned long long w0 = __hip_atomic_load(p + box_word(k, 0) / 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long w1 = __hip_atomic_load(p + box_word(k, 2) / 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long w2 = __hip_atomic_load(p + box_word(k, 4) / 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b[0] = __uint_as_float((unsigned int)w0); b[1] = __uint_as_float((unsigned int)(w0 >> 32));
    b[2] = __uint_as_float((unsigned int)w1); b[3] = __uint_as_float((unsigned int)(w1 >> 32));
    b[4] = __uint_as_float((unsigned int)w2); b[5] = __uint_as_float((unsigned int)(w2 >> 32));
}

__global__ __launch_bounds__(RF_BLOCK) void refit_topology(int numSlots, const int* __restrict__ nodes, unsigned int* __restrict__ parent,
                                                           unsigned int* __restrict__ arrive,
                                                           RfStats* __restrict__ stats /* or null: nothing is counted */)
{
    const int node = blockIdx.x * RF_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0;
    if (node < numSlots) {
        int kind[2];
        topology_slot(node, numSlots, nodes, parent, arrive, kind);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            leaf += kind[k] == LINK_LEAF ? 1u : 0u;
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= RF_ERR_LINK;
        }
    }
    if (!stats) return;
    stats += blockIdx.x % RF_STAT_SLOTS;
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

// G lanes share a leaf (G = 1, 4 or 8 consecutive lanes, chosen by the host from the tree's mean leaf size; the result does not depend
// on it): lane `sub` takes the row groups sub, sub + G, ... of the leaf, so that a leaf's index -> vertex gathers are in flight
// together; the lanes find the terminator by a ballot, fold their boxes by shuffles, and lane 0 of the group goes on to climb.
template <int G>
__global__ __launch_bounds__(RF_BLOCK) void refit_climb(int numSlots, int* __restrict__ nodes, int numRows, float4* __restrict__ woop,
                                                        const int* __restrict__ triIndex, int numTris, const int* __restrict__ tri,
                                                        int numVerts, const float* __restrict__ pos, float eps,
                                                        const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                        float* __restrict__ sceneBox /* or null */, RfStats* __restrict__ stats)
{
    static_assert(G == 1 || G == 2 || G == 4 || G == 8, "a group is a power of two of lanes inside a wave");
    __shared__ unsigned int sCount[3];           // the workgroup's rows, error bits and threads done (the blocking form only)
    if (stats) {                                 // uniform
        if (threadIdx.x < 3) sCount[threadIdx.x] = 0u;
        __syncthreads();
    }
    const int gid = blockIdx.x * RF_BLOCK + threadIdx.x;
    const int g = gid / G, sub = gid % G;
    const int groupShift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane
    int node = g >> 1, k = g & 1;
    const int link = g < 2 * numSlots ? nodes[(size_t)node * kNodeWords + kLinkWord + k] : 0;
    const bool leaf = link < 0;                  // an inner child arrives with the owner of its node; offset 0 is no child at all
    unsigned int err = 0;
    unsigned int rows = 0;
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};   // ord_enc words: min / max as integers
    if (leaf) {                                  // uniform within a group, and so is the trip count of this loop
        for (long long r0 = (long long)leaf_row(link);; r0 += 3 * G) {
            const long long r = r0 + 3 * sub;
            const bool inside = r < numRows;
            const bool term = !inside || __float_as_uint(woop[r].x) == kLeafTerm;
            const unsigned int terms = (unsigned int)((__ballot(term) >> groupShift) & ((1ull << G) - 1ull));
            const int first = terms ? __ffs((int)terms) - 1 : G;   // the group's lanes below `first` hold triangles
            if (sub == first) {
                if (inside) rows += 1; else err |= RF_ERR_ROW;      // the terminator, or the end of the buffer before one
            } else if (sub < first) {
                const int t = r + 2 < numRows ? triIndex[r] : -1;
                if (r + 2 >= numRows) {
                    err |= RF_ERR_ROW;
                } else if (t < 0 || t >= numTris) {
                    err |= RF_ERR_TRI;
                } else {
                    int i0, i1, i2;
                    if (!tri_indices_checked(tri, numVerts, t, i0, i1, i2)) {
                        err |= RF_ERR_VERTEX;
                    } else {
                        float v[9];
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            v[q] = pos[3 * (size_t)i0 + q];
                            v[3 + q] = pos[3 * (size_t)i1 + q];
                            v[6 + q] = pos[3 * (size_t)i2 + q];
                        }
                        float4 w0, w1, w2;
                        woop_rows_verts(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], w0, w1, w2);
                        woop[r] = w0;
                        woop[r + 1] = w1;
                        woop[r + 2] = w2;
                        rows += 3;
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            const unsigned int a = ord_enc(v[q]), b = ord_enc(v[3 + q]), c = ord_enc(v[6 + q]);
                            lo[q] = min(lo[q], min(a, min(b, c)));
                            hi[q] = max(hi[q], max(a, max(b, c)));
                        }
                    }
                }
            }
            if (terms) break;
        }
        // the group's box and error bits in every lane of the group (partners stay inside the group: they are active)
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                lo[q] = min(lo[q], (unsigned int)__shfl_xor((int)lo[q], o));
                hi[q] = max(hi[q], (unsigned int)__shfl_xor((int)hi[q], o));
            }
        }
    }
    const unsigned int groupErr = leaf ? (unsigned int)((__ballot(err != 0) >> groupShift) & ((1ull << G) - 1ull)) : 0u;
    if (stats) {                                 // one add per workgroup and counter, by the wave that finishes its leaves last:
        // no barrier, nobody's climb waits for the workgroup's longest leaf; the whole wave is here: nobody has returned yet
        const unsigned int waveRows = wave_sum_u32(rows), waveErr = wave_or_u32(err);
        if ((threadIdx.x & 63) == 0) {
            if (waveRows) atomicAdd(&sCount[0], waveRows);
            if (waveErr) atomicOr(&sCount[1], waveErr);
            if (atomicAdd(&sCount[2], 1u) == RF_BLOCK / 64 - 1) {   // a wave's LDS operations are performed in order
                const unsigned int nr = atomicAdd(&sCount[0], 0u), ne = atomicOr(&sCount[1], 0u);
                RfStats* mine = stats + blockIdx.x % RF_STAT_SLOTS;
                if (nr) atomicAdd(&mine->rows, nr);
                if (ne) atomicOr(&mine->err, ne);
            }
        }
    }
    if (!leaf || sub != 0 || groupErr) return;   // after an error the nodes above keep an arrival short and stay as they are
    float box[6];
    const bool have = lo[0] <= hi[0];            // some triangle was folded
    if (have) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            box[2 * q] = ord_dec(lo[q]) - eps;
            box[2 * q + 1] = ord_dec(hi[q]) + eps;
        }
        rf_publish_box(nodes, node, k, box);
    } else {                                     // a leaf without rows keeps its box words (nobody writes them in this launch)
        const float* nf = reinterpret_cast<const float*>(nodes + (size_t)node * kNodeWords);
#pragma unroll
        for (int j = 0; j < 6; j++) box[j] = nf[box_word(k, j)];
    }
    // the box (and the rows) have reached memory before the first arrival is announced: climb() drains them
    float sib[6];
    climb(
        node, k, numSlots, nodes, parent, arrive, [&](int pn, int pk) { rf_publish_box(nodes, pn, pk, box); },
        [&](int n, int sk) { rf_acquire_box(nodes, n, sk, sib); },
        [&](int n, int) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                box[2 * q] = ord_min(box[2 * q], sib[2 * q]);
                box[2 * q + 1] = ord_max(box[2 * q + 1], sib[2 * q + 1]);
            }
            if (n == 0 && sceneBox) {            // the root reports to no parent
                sceneBox[0] = box[0]; sceneBox[1] = box[2]; sceneBox[2] = box[4];
                sceneBox[3] = box[1]; sceneBox[4] = box[3]; sceneBox[5] = box[5];
            }
        });
}

struct RfLayout {
    size_t stats, parent, arrive, end;
    explicit RfLayout(int64_t slots)
    {
        ScratchCarver c;
        stats = c.take(sizeof(RfStats) * RF_STAT_SLOTS);
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        end = c.off;
    }
};

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_refit(void* d_nodes, int64_t nodesBytes, void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                  int64_t triIndexBytes, int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                  float epsilon, float* d_sceneBox, NtrBvhRefitResult* result, void* stream)
{
    if (result) {
        result->numNodes = result->numLeaves = result->numRows = result->pad = 0;
    }
    if (!d_nodes) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: null d_nodes");
    if (const int rc = check_nodes_bytes("ntr_bvh_refit", "nodesBytes", nodesBytes)) return rc;
    if (!d_triWoop) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: null d_triWoop");
    if (triWoopBytes < 16 || (triWoopBytes % 16) != 0 || triWoopBytes / 16 > INT_MAX)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: triWoopBytes must be a positive multiple of 16 (at most 2^31 - 1 rows)");
    if (!d_triIndex) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: null d_triIndex");
    if (triIndexBytes < 0 || triIndexBytes * 4 < triWoopBytes)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: triIndexBytes must cover one entry per Woop row (triIndexBytes * 4 >= triWoopBytes)");
    if (numTris < 1) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: numTris < 1");
    if (!d_triVtxIndex) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: null d_triVtxIndex");
    if (numVerts < 1) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: numVerts < 1");
    if (!d_vtxPos) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: null d_vtxPos");
    if (!std::isfinite(epsilon) || epsilon < 0.0f) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: epsilon must be finite and >= 0");

    hipStream_t s = (hipStream_t)stream;
    const int numSlots = (int)(nodesBytes / 64), numRows = (int)(triWoopBytes / 16);
    const RfLayout lay(numSlots);
    const bool capturing = stream_is_capturing(s);
    if (capturing && result) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: a captured call cannot read a result back (pass result = NULL)");
    if (capturing && g_rfPool.held() < lay.end)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_refit: the scratch pool holds %zu B and this tree needs %zu B; a captured call cannot "
                         "allocate -- refit a tree at least as large once outside the capture", g_rfPool.held(), lay.end);
    void* base = nullptr;
    {
        const int rc = g_rfPool.reserve(lay.end, &base);
        if (rc != NTR_OK) return rc;
    }
    auto P = [&](size_t o) { return (char*)base + o; };
    RfStats* stats = result ? (RfStats*)P(lay.stats) : nullptr;

    StreamEvents<2> ev(s);
    if (result) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
    }
    if (stats) NTR_HIP(hipMemsetAsync(stats, 0, sizeof(RfStats) * RF_STAT_SLOTS, s));
    hipLaunchKernelGGL(refit_topology, dim3((numSlots + RF_BLOCK - 1) / RF_BLOCK), dim3(RF_BLOCK), 0, s, numSlots, (const int*)d_nodes,
                       (unsigned int*)P(lay.parent), (unsigned int*)P(lay.arrive), stats);
    // lanes per leaf from the mean leaf size the extents imply (a tree has one leaf more than inner nodes): a choice of speed only
    const double meanTris = ((double)numRows - (double)(numSlots + 1)) / (3.0 * (double)(numSlots + 1));
    const int group = meanTris < 1.5 ? 1 : (meanTris < 3.0 ? 4 : 8);
    const dim3 grid((unsigned int)((2ll * numSlots * group + RF_BLOCK - 1) / RF_BLOCK));
#define NTR_RF_CLIMB(G)                                                                                                                   \
    hipLaunchKernelGGL(refit_climb<G>, grid, dim3(RF_BLOCK), 0, s, numSlots, (int*)d_nodes, numRows, (float4*)d_triWoop, d_triIndex, numTris, \
                       d_triVtxIndex, numVerts, d_vtxPos, epsilon, (const unsigned int*)P(lay.parent), (unsigned int*)P(lay.arrive),       \
                       d_sceneBox, stats)
    if (group == 1) NTR_RF_CLIMB(1); else if (group == 4) NTR_RF_CLIMB(4); else NTR_RF_CLIMB(8);
#undef NTR_RF_CLIMB
    NTR_HIP(hipGetLastError());
    if (!result) return NTR_OK;

    NTR_HIP(ev.record(1));
    static RfStats slots[RF_STAT_SLOTS];   // one caller per device at a time, and the copy is waited for right here
    static std::mutex slotsMu;
    std::lock_guard<std::mutex> lk(slotsMu);
    NTR_HIP(hipMemcpyAsync(slots, stats, sizeof(slots), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    RfStats h = {};
    for (const RfStats& v : slots) { h.innerLinks += v.innerLinks; h.leafLinks += v.leafLinks; h.rows += v.rows; h.err |= v.err; }
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    if (h.err)
        return set_error(NTR_ERR_LAYOUT, "ntr_bvh_refit: malformed tree (error 0x%x: 1 child link, 2 leaf row outside the extents, "
                         "4 triangle index, 8 vertex index out of range); the parts above it were left as they were", h.err);
    result->numNodes = (int32_t)(1u + h.innerLinks);
    result->numLeaves = (int32_t)h.leafLinks;
    result->numRows = (int32_t)h.rows;
    result->seconds = ms * 1e-3f;
    return NTR_OK;
}

int ntr_bvh_refit_scratch_bytes(int64_t* bytes)
{
    if (!bytes) return set_error(NTR_ERR_INVALID, "ntr_bvh_refit_scratch_bytes: null");
    *bytes = (int64_t)g_rfPool.held();
    return NTR_OK;
}

}  // extern "C"
