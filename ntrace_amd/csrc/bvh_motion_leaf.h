// bvh_motion_leaf.h -- the vertex rows of a leaf under one key of a two-key refit, for the kernels that refit one tree
// (bvh_motion_refit_kernels.hip) and many BLASes of a pool (bvh_motion_refit_batch_kernels.hip).  The rule is tests/np_bvh_motion.py
// (motion_refit).  The walk is refit_leaf_rows' (bvh_refit_leaf.h), whose header says what a caller inside a pool passes: the TREE's
// pointers and extents.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_refit_leaf.h"

namespace ntr {

// The vertex rows of a leaf that refit_leaf_rows<G> has walked without an error in any lane of the group (so every row, triangle and
// vertex index met here is inside its extent): the same walk, lane `sub` at the row groups sub, sub + G, ...
template <int G>
__device__ __forceinline__ void motion_leaf_vertex_rows(int link, int sub, int groupShift, int numRows, const float4* woop, const int* triIndex,
                                                        const int* tri, const float* pos, uint4* vertRows)
{
    for (long long r0 = (long long)leaf_row(link);; r0 += 3 * G) {   // the trip count is uniform within a group
        const long long r = r0 + 3 * sub;
        const bool inside = r < numRows;
        const bool term = !inside || __float_as_uint(woop[r].x) == kLeafTerm;
        const unsigned int terms = (unsigned int)((__ballot(term) >> groupShift) & ((1ull << G) - 1ull));
        const int first = terms ? __ffs((int)terms) - 1 : G;
        if (sub == first) {
            if (inside) vertRows[r] = make_uint4(0u, 0u, 0u, kLeafTerm);   // in w: a vertex's x may be -0.0f, the terminator's word
        } else if (sub < first && r + 2 < numRows) {
            const int t = triIndex[r];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const size_t v = (size_t)tri[3 * (size_t)t + j];
                vertRows[r + j] = make_uint4(__float_as_uint(pos[3 * v]), __float_as_uint(pos[3 * v + 1]), __float_as_uint(pos[3 * v + 2]), 0u);
            }
        }
        if (terms) break;
    }
}

}  // namespace ntr
