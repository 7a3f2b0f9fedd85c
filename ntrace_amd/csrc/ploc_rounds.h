// ploc_rounds.h -- the PLOC rounds as a service: what bvh_ploc_kernels.hip (which defines the kernels and the loop) shares with
// tlas_build_kernels.hip (which runs the same rounds over instance boxes) and with bvh_ploc_batch_kernels.hip (whose own kernels run
// the rounds of many meshes at once, segment by segment, and take the rule's pieces from here).  The rounds work on a list of
// (box, link, height) clusters and never look at a triangle: a caller fills cluster buffer 0 and the state record, then calls
// ploc_rounds and ploc_tail.
//   pl_distance, pl_nearest, pl_write_node   the rule's pieces: a union's distance, a cluster's neighbour given its position in its list
//                                   and that list's length, a merged pair's node
//   PlState / PlBuf / PlBufs / U2   the kernels' parameter types.  They sit in an unnamed namespace -- one copy per translation unit, as
//                                   level_build.h's plane table -- so that the pl_* kernels keep the names they were built under
//   PlRoundsLayout                  the rounds' slices of a scratch block
//   ploc_rounds, ploc_tail          the round loop (groups of four launches, a read-back per group) and the tail launch
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "compact_bvh.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {
namespace {

struct U2 {
    unsigned int x, y;   // survivors, merging pairs
    __device__ U2 operator+(const U2& b) const { return U2{x + b.x, y + b.y}; }
};

struct PlState {          // halves [k & 1] are read by launch group k, [(k & 1) ^ 1] written
    int n[2];             // list length
    int rounds[2];        // rounds done
    int cur[2];           // which cluster buffer holds the list
    unsigned int err;     // bit 0: vertex index out of range (ntr_tlas_build: BLAS index out of range), bit 1: a leaf row outside the buffer
                          // (emit_leaf_rows), bit 2: a node slot or a list position outside its bounds, bit 3: a round without a merge
                          // (none of the last three is expected)
    int height;           // the last cluster's height (the tail writes it)
};
static_assert(sizeof(PlState) == 32, "one 32-byte record (read_totals)");

struct PlBuf {            // a list of clusters: box component c of cluster i at box[c * cap + i] (lo.x lo.y lo.z hi.x hi.y hi.z)
    float* box;
    int* link;
    int* height;
};
struct PlBufs { PlBuf b[2]; };

}  // namespace

constexpr int kPlocMaxRadius = 64;
constexpr int kPlocMaxHeight = 100;   // the reference CPU tracer's stack (CudaBVH.cpp:701), ntr_persistent_bvh_build's bound

// ---- the rule's pieces, for every kernel that runs a round -------------------------------------------------------------------------
// d of the union of box a (registers) and the box at column j of a [6][stride] array
__device__ __forceinline__ float pl_distance(const float* a, const float* s, int stride, int j)
{
    const float ex = ord_max(a[3], s[3 * stride + j]) - ord_min(a[0], s[j]);
    const float ey = ord_max(a[4], s[4 * stride + j]) - ord_min(a[1], s[stride + j]);
    const float ez = ord_max(a[5], s[5 * stride + j]) - ord_min(a[2], s[2 * stride + j]);
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(ex, ey), __fmul_rn(ey, ez)), __fmul_rn(ez, ex));
    return d != d ? INFINITY : d;
}

// nn[i]: cluster i of a list of n sits at column li of s; its candidates i - k and i + k at li - k and li + k.  i and n may be a
// position inside a segment of a longer list and that segment's length: the result is then relative to the segment's start too
__device__ __forceinline__ int pl_nearest(const float* s, int stride, int li, int i, int n, int radius)
{
    float a[6];
#pragma unroll
    for (int c = 0; c < 6; c++) a[c] = s[c * stride + li];
    float bestD = INFINITY;
    int bestT = INT_MAX, best = -1;
    for (int k = 1; k <= radius; k++) {
        const int q = i / k;   // min(i, j) / k is q - 1 for j = i - k and q for j = i + k
        if (i - k >= 0) {
            const float d = pl_distance(a, s, stride, li - k);
            const int t = 2 * k + ((q - 1) & 1);
            if (d < bestD || (d == bestD && t < bestT)) { bestD = d; bestT = t; best = i - k; }
        }
        if (i + k < n) {
            const float d = pl_distance(a, s, stride, li + k);
            const int t = 2 * k + (q & 1);
            if (d < bestD || (d == bestD && t < bestT)) { bestD = d; bestT = t; best = i + k; }
        }
    }
    return best;
}

// the node of a merging pair: child 0 the lower-index cluster, child 1 the upper, boxes and links as they stand
__device__ __forceinline__ void pl_write_node(int* __restrict__ nodes, int slot, const float* b0, int link0, const float* b1, int link1)
{
    write_inner_node(nodes, slot, b0, b0 + 3, b1, b1 + 3, 0);
    nodes[kNodeWords * (long long)slot + kLinkWord] = link0;
    nodes[kNodeWords * (long long)slot + kLinkWord + 1] = link1;
}

// The rounds' scratch for a list of at most n clusters (cap == n in the kernels' box indexing)
struct PlRoundsLayout {
    size_t state, nn, local, blockSums, box[2], link[2], height[2];
    void carve(ScratchCarver& cv, int64_t n)
    {
        const int64_t nb = n / NTR_PLOC_TILE + 2;
        state = cv.take(sizeof(PlState));
        nn = cv.take((size_t)n * 4);
        local = cv.take((size_t)n * sizeof(U2));
        blockSums = cv.take((size_t)nb * sizeof(U2));
        for (int k = 0; k < 2; k++) {
            box[k] = cv.take((size_t)n * 24);
            link[k] = cv.take((size_t)n * 4);
            height[k] = cv.take((size_t)n * 4);
        }
    }
};

namespace {
inline PlBufs pl_bufs(void* base, const PlRoundsLayout& lay)
{
    PlBufs r;
    for (int k = 0; k < 2; k++)
        r.b[k] = PlBuf{(float*)((char*)base + lay.box[k]), (int*)((char*)base + lay.link[k]), (int*)((char*)base + lay.height[k])};
    return r;
}
}  // namespace

// The rounds before the tail over the list in cluster buffer 0 of `base` (len clusters of a buffer of cap; the state record holds
// n[0] = len and zeros): groups of four rounds, one read-back of the record per group, until the list has at most NTR_PLOC_TAIL
// clusters.  *k: launch groups so far (in: 0); *len: the list length the host knows.  Nodes go to d_nodes (nodeCap slots).
int ploc_rounds(const char* fn, void* base, const PlRoundsLayout& lay, int cap, int radius, void* d_nodes, int nodeCap, hipStream_t s,
                int* k, int* len);
// The tail launch: every remaining round in one workgroup.  The caller reads the record back (half *k & 1 after the call).
int ploc_tail(void* base, const PlRoundsLayout& lay, int cap, int radius, void* d_nodes, int nodeCap, hipStream_t s, int* k);

}  // namespace ntr
