// bvh_refit_leaf.h -- the refit's leaf pass as functions of one tree's pointers: the walk over a leaf's row groups to the terminator, the
// Woop rows, the integer-order fold of the box, and epsilon, the box's publish and the climb (bvh_climb.h).  The rule is
// tests/np_bvh_refit.py.  Used by the kernels that refit many BLASes of a pool
// (bvh_refit_batch_kernels.hip) and many wide BLASes of a wide pool (wide_refit_batch_kernels.hip: refit_leaf_rows only).  refit_climb of
// bvh_refit_kernels.hip holds the same statements inline and does NOT include this header: built over these functions its three
// instances came out with other code than before (block layout and register assignment; scripts/kernel_isa_diff.sh), so that file was
// left as it was.  A change to the leaf rule is made in both places; tests/test_refit_batch_gpu.py compares the two
// kernels' bytes on every shape it runs.
// Every pointer is the TREE's: a caller whose tree lies inside a pool advances nodes, woop, triIndex, tri, parent and arrive to the
// tree's base and passes the tree's own numSlots / numRows / numTris, since a Compact tree's links are relative to its own start.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_climb.h"
#include "device_prims.h"
#include "woop_rows.h"

namespace ntr {

enum : unsigned int { RF_ERR_LINK = 1u, RF_ERR_ROW = 2u, RF_ERR_TRI = 4u, RF_ERR_VERTEX = 8u };

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

// G lanes share a leaf (G = 1, 4 or 8 consecutive lanes, chosen by the host from the mean leaf size; the result does not depend
// on it): lane `sub` takes the row groups sub, sub + G, ... of the leaf, so that a leaf's index -> vertex gathers are in flight
// together; the lanes find the terminator by a ballot and fold their boxes by shuffles.  `link` is the leaf's (< 0), uniform within
// the group, whose first lane of the wave is groupShift.  Afterwards lo / hi hold the group's box as ord_enc words in every lane of
// the group (lo > hi: no triangle was folded); err and rows are the lane's own.  REWRITE false (the wide refit that follows a binary one,
// wide_refit_batch_kernels.hip, whose rows are current already) only reads the rows, to find the terminator and triIndex: that instance
// holds no store to woop.
template <int G, bool REWRITE = true>
__device__ __forceinline__ void refit_leaf_rows(int link, int sub, int groupShift, int numRows, float4* woop,
                                                const int* triIndex, int numTris, const int* tri, int numVerts,
                                                const float* pos, unsigned int& err, unsigned int& rows,
                                                unsigned int (&lo)[3], unsigned int (&hi)[3])
{
    static_assert(G == 1 || G == 2 || G == 4 || G == 8, "a group is a power of two of lanes inside a wave");
    for (long long r0 = (long long)leaf_row(link);; r0 += 3 * G) {   // the trip count is uniform within a group
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
                    if (REWRITE) {
                        float4 w0, w1, w2;
                        woop_rows_verts(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], w0, w1, w2);
                        woop[r] = w0;
                        woop[r + 1] = w1;
                        woop[r + 2] = w2;
                    }
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
    // the group's box in every lane of the group (partners stay inside the group: they are active)
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            lo[q] = min(lo[q], (unsigned int)__shfl_xor((int)lo[q], o));
            hi[q] = max(hi[q], (unsigned int)__shfl_xor((int)hi[q], o));
        }
    }
}

// The leaf at child slot k of `node`, folded into lo / hi by refit_leaf_rows without an error: epsilon, the box into its slot of the
// node, and the climb; the root's union goes to sceneBox (min.xyz max.xyz) when given.  One lane per leaf.
__device__ __forceinline__ void refit_leaf_climb(int node, int k, int numSlots, int* nodes, const unsigned int (&lo)[3],
                                                 const unsigned int (&hi)[3], float eps, const unsigned int* parent,
                                                 unsigned int* arrive, float* sceneBox /* or null */)
{
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

}  // namespace ntr
