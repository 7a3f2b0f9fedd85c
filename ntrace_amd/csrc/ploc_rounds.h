// ploc_rounds.h -- the PLOC rounds as a service: what bvh_ploc_kernels.hip (which defines the kernels and the loop) shares with
// tlas_build_kernels.hip (which runs the same rounds over instance boxes).  The rounds work on a list of (box, link, height) clusters
// and never look at a triangle: a caller fills cluster buffer 0 and the state record, then calls ploc_rounds and ploc_tail.
//   PlState / PlBuf / PlBufs / U2   the kernels' parameter types.  They sit in an unnamed namespace -- one copy per translation unit, as
//                                   level_build.h's plane table -- so that the pl_* kernels keep the names they were built under
//   PlRoundsLayout                  the rounds' slices of a scratch block
//   ploc_rounds, ploc_tail          the round loop (groups of four launches, a read-back per group) and the tail launch
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
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
