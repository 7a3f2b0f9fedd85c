// wide_bvh.h -- the 4-wide node layout, stated once, for the pass that writes such a tree (bvh_widen_kernels.hip) and the kernel that
// traverses one (trace_wide_kernels.hip).  EXTENSION without a reference counterpart: the rule is the numpy spec tests/np_bvh_wide.py.
// A wide tree is a second node buffer over a BVHLayout_Compact tree (compact_bvh.h): leaves, Woop rows and triIndex are the binary
// tree's, unchanged.  A wide node is 32 words, 128 bytes, eight 16-byte rows, laid out so that ray_box2 (trace_lane.h) tests a pair of
// its boxes as it tests a Compact node's:
//   rows 0..2  words 0..11    the boxes of children 0 and 1 in Compact's box words, box_word(k, j)
//   row 3      words 12..15   the links of children 0..3
//   rows 4..6  words 16..27   the boxes of children 2 and 3: 16 + box_word(k - 2, j)
//   row 7      words 28..31   word 28 the child count (2..4), words 29..31 zero
// A link < 0 is a leaf, ~link its first Woop row, copied verbatim from the binary tree; > 0 is 128 * index of a wide node; 0 is an empty
// slot.  Slot k >= count has link 0 and a copy of slot 0's box: every box word of the wide tree is a box word of the binary tree, so
// ntr_bvh_validate's flags for the binary tree hold for the wide one -- while the binary tree is current.  A wide tree that is refitted
// on its own (ntr_pool_wide_refit with rewriteRows, ntr_tlas_wide_refit: no binary refit runs) leaves the binary boxes and their flags
// behind; the two-level trace then validates the wide buffers themselves (ntr_instanced_wide_validate).  The stack
// sentinel stays kSentinel.
#pragma once
#include "compact_bvh.h"

namespace ntr {

constexpr int kWideWords = 32, kWideBytes = 128, kWideRows = kWideBytes / kRowBytes;
constexpr int kWideChildren = 4;
constexpr int kWideLinkWord = 12;                             // + k for child k
constexpr int kWideCountWord = 28;
constexpr int64_t kMaxWideBytes = 0x76543200ll;               // largest multiple of 128 below the sentinel
constexpr int64_t kMaxWideNodes = kMaxWideBytes / kWideBytes;
static_assert(kMaxWideBytes % kWideBytes == 0 && kMaxWideBytes < kSentinel && kMaxWideBytes + kWideBytes > kSentinel,
              "the wide node buffer ends below the sentinel");

// word of component j (lo.x hi.x lo.y hi.y lo.z hi.z) of child k's box
__host__ __device__ __forceinline__ int wide_box_word(int k, int j) { return (k >= 2 ? 16 : 0) + box_word(k & 1, j); }
__host__ __device__ __forceinline__ int wide_link(int index) { return kWideBytes * index; }

// The size of a wide node buffer an entry point is handed
inline int check_wide_bytes(const char* fn, int64_t wideNodesBytes)
{
    if (wideNodesBytes < kWideBytes || (wideNodesBytes % kWideBytes) != 0 || wideNodesBytes > kMaxWideBytes)
        return set_error(NTR_ERR_INVALID, "%s: wideNodesBytes must be a multiple of 128 in [128, 0x%llx]", fn, (unsigned long long)kMaxWideBytes);
    return NTR_OK;
}

}  // namespace ntr
