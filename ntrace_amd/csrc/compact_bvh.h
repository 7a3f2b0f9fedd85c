// compact_bvh.h -- the BVHLayout_Compact node layout, stated once, for the device code that writes, rewrites or checks such a tree
// (bvh_build_, sah_build_, bvh_refit_, bvh_optimize_, bvh_reorder_kernels.hip, bvh_utils.hip), for the kernels that traverse one (trace_kernels.hip
// and its trace_*.h) and for the C-ABI front doors that take or fill one (ntr_api.cpp, lbvh_kernels.hip, hlbvh_kernels.hip).  bvh_climb.h holds the bottom-up pass over it.
// A node is 16 words, 64 bytes (CudaBVH.hpp:42-46):
//   words 0..3    child 0: lo.x hi.x lo.y hi.y      words 4..7    child 1: lo.x hi.x lo.y hi.y
//   words 8..11   child 0: lo.z hi.z, child 1: lo.z hi.z
//   words 12, 13  the links of child 0 and child 1; word 14 the split word (no kernel reads it); word 15 is zero
// A link is a signed 32-bit word: < 0 is a leaf, ~link the leaf's first Woop row; > 0 is an inner child, the byte offset 64 * index of
// its node; 0 is the root's offset, which no link holds.  The traversal's stack sentinel is 0x76543210 (EntrypointSentinel,
// CudaTracerKernels.hpp:38), so a node at or beyond that byte offset cannot be addressed.  A leaf's rows end at a row whose x word is
// the terminator (CudaBVH.cpp:1091).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include "ntr_internal.h"

namespace ntr {

constexpr int kNodeWords = 16, kNodeBytes = 64;
constexpr int kLinkWord = 12;                                 // + k for child k
constexpr int kSentinel = 0x76543210;                         // CudaTracerKernels.hpp:38 (EntrypointSentinel)
constexpr int64_t kMaxNodesBytes = 0x76543200ll;              // largest multiple of 64 below the sentinel
constexpr int64_t kMaxNodes = kMaxNodesBytes / kNodeBytes;    // 31 019 208
static_assert(kMaxNodesBytes == kSentinel / kNodeBytes * kNodeBytes, "the node buffer ends below the sentinel");
constexpr unsigned int kLeafTerm = 0x80000000u;
// A Woop row is four words; a triangle is three rows (z, u, v: woop_rows.h), and the x word of the row after it says whether the leaf ends there
constexpr int kRowBytes = 16, kRowShift = 4;                  // byte offset = row << kRowShift
constexpr int kTriRows = 3, kTriBytes = kTriRows * kRowBytes;
static_assert(kRowBytes == 1 << kRowShift && kTriBytes + kRowBytes == kNodeBytes, "a triangle and the word after it are as long as a node");

// word (< 12) of component j (lo.x hi.x lo.y hi.y lo.z hi.z) of child k's box, and back
__host__ __device__ __forceinline__ int box_word(int k, int j) { return j < 4 ? 4 * k + j : 8 + 2 * k + (j - 4); }
__host__ __device__ __forceinline__ int box_word_child(int w) { return w < 8 ? (w >> 2) : ((w - 8) >> 1); }
__host__ __device__ __forceinline__ int box_word_comp(int w) { return w < 8 ? (w & 3) : 4 + ((w - 8) & 1); }

__host__ __device__ __forceinline__ int leaf_link(int row) { return ~row; }
__host__ __device__ __forceinline__ int leaf_row(int link) { return ~link; }
__host__ __device__ __forceinline__ int inner_link(int index) { return kNodeBytes * index; }
__host__ __device__ __forceinline__ int inner_index(int link) { return link >> 6; }
// a link that names a node slot of a buffer of numSlots slots (other than the root's: offset 0 is nobody's child)
__host__ __device__ __forceinline__ bool is_inner_link(int c, int numSlots) { return c > 0 && (c & 63) == 0 && (c >> 6) < numSlots; }

// Node idx but for its two links, which the children's tasks write when they are numbered.
__device__ __forceinline__ void write_inner_node(int* __restrict__ nodes, long long idx, const float* lo0, const float* hi0, const float* lo1,
                                                 const float* hi1, int splitWord)
{
    int* nd = nodes + kNodeWords * idx;
    const float w[12] = {lo0[0], hi0[0], lo0[1], hi0[1], lo1[0], hi1[0], lo1[1], hi1[1], lo0[2], hi0[2], lo1[2], hi1[2]};
    for (int k = 0; k < 12; k++) nd[k] = __float_as_int(w[k]);
    nd[14] = splitWord;
    nd[15] = 0;
}
__device__ __forceinline__ void write_leaf_terminator(uint4* __restrict__ woop, int* __restrict__ triIndex, long long row)
{
    woop[row] = make_uint4(kLeafTerm, kLeafTerm, kLeafTerm, kLeafTerm);
    triIndex[row] = 0;
}

// ---- host: the checks every entry point makes the same way ------------------------------------------------------------------
// The size of a node buffer an entry point is handed; `what` is the argument as that entry point's messages call it.
inline int check_nodes_bytes(const char* fn, const char* what, int64_t nodesBytes)
{
    if (nodesBytes < kNodeBytes || (nodesBytes % kNodeBytes) != 0 || nodesBytes > kMaxNodesBytes)
        return set_error(NTR_ERR_INVALID, "%s: %s must be a multiple of 64 in [64, 0x%llx]", fn, what, (unsigned long long)kMaxNodesBytes);
    return NTR_OK;
}

// The mesh a build is handed.  An entry point with further pointers passes whether they are there and how its message names them.
inline int check_build_geometry(const char* fn, int32_t numTris, int32_t numVerts, const void* d_triVtxIndex, const void* d_vtxPos,
                                bool moreThere = true, const char* more = "")
{
    if (numTris < 1 || numTris >= (1 << 28) || numVerts < 1 || !d_triVtxIndex || !d_vtxPos || !moreThere)
        return set_error(NTR_ERR_INVALID, "%s: bad geometry arguments (1 <= numTris < 2^28, numVerts >= 1, non-null buffers%s)", fn, more);
    return NTR_OK;
}

// The output buffers of a build against ntr_lbvh_capacity(numTris); *nodeCap and *rowCap (or null): what the kernels may index
inline int check_build_outputs(const char* fn, int32_t numTris, const void* d_nodes, int64_t nodesCapacity, const void* d_triWoop,
                               int64_t triWoopCapacity, const void* d_triIndex, int64_t triIndexCapacity, int64_t* nodeCap,
                               int64_t* rowCap)
{
    int64_t needN, needW, needI;
    ntr_lbvh_capacity(numTris, &needN, &needW, &needI);
    if (!d_nodes || !d_triWoop || !d_triIndex || nodesCapacity < needN || triWoopCapacity < needW || triIndexCapacity < needI)
        return set_error(NTR_ERR_INVALID, "%s: output buffers smaller than ntr_lbvh_capacity()", fn);
    if (nodeCap) *nodeCap = std::min<int64_t>(nodesCapacity / kNodeBytes, kMaxNodes);
    if (rowCap) *rowCap = std::min<int64_t>(std::min<int64_t>(triWoopCapacity / kRowBytes, triIndexCapacity / 4), INT_MAX);
    return NTR_OK;
}

// A level-synchronous build whose level brings the tree beyond kMaxNodes inner nodes
inline int node_overflow_error(const char* fn, int level, int64_t innerNodes)
{
    return set_error(NTR_ERR_OVERFLOW, "%s: level %d brings the tree to %lld inner nodes, more than the %lld that BVHLayout_Compact's "
                     "32-bit child offsets address", fn, level, (long long)innerNodes, (long long)kMaxNodes);
}

}  // namespace ntr
