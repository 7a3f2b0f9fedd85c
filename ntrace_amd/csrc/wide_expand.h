// wide_expand.h -- the expansion of a kept binary slot into the entries of a 4-wide node, stated once, for the two passes that widen a
// BVHLayout_Compact tree: bvh_widen_kernels.hip (one tree) and pool_widen_batch_kernels.hip (every BLAS of a pool).  EXTENSION without
// a reference counterpart: the rule is rules 1 and 2 of the numpy spec tests/np_bvh_wide.py.  `nodes` is the tree's own first node and
// numSlots its own slot count, so a link is judged against the tree it belongs to, wherever that tree lies in a pool.
// The area rule needs -ffp-contract=off (the Makefile's flags).
#pragma once
#include <hip/hip_runtime.h>

#include "wide_bvh.h"

namespace ntr {

struct WdEntry {
    int link;                                // the binary tree's word
    int src;                                 // 2 * slot + child: where its box is
};

// np_bvh_optimize.area of child slot src's box: fl(fl(fl(dx*dy) + fl(dy*dz)) + fl(dz*dx)) (compiled with -ffp-contract=off)
__device__ __forceinline__ float wd_area(const int* __restrict__ nodes, int src)
{
    const int* nd = nodes + (size_t)(src >> 1) * kNodeWords;
    const int k = src & 1;
    const float dx = __int_as_float(nd[box_word(k, 1)]) - __int_as_float(nd[box_word(k, 0)]);
    const float dy = __int_as_float(nd[box_word(k, 3)]) - __int_as_float(nd[box_word(k, 2)]);
    const float dz = __int_as_float(nd[box_word(k, 5)]) - __int_as_float(nd[box_word(k, 4)]);
    return (dx * dy + dy * dz) + dz * dx;
}

// Rules 1 and 2 of the spec for slot b; returns the number of entries (2..4)
__device__ __forceinline__ int wd_expand(const int* __restrict__ nodes, int numSlots, int b, WdEntry (&E)[kWideChildren])
{
    const int2 c = *reinterpret_cast<const int2*>(nodes + (size_t)b * kNodeWords + kLinkWord);
    E[0] = WdEntry{c.x, 2 * b};
    E[1] = WdEntry{c.y, 2 * b + 1};
    E[2] = E[3] = WdEntry{0, 2 * b};
    int n = 2;
#pragma unroll
    for (int step = 0; step < 2; step++) {   // n == 2 + step while the expansion goes on
        int best = -1;
        float bestA = 0.0f;
#pragma unroll
        for (int p = 0; p < 2 + step; p++) {
            if (n != 2 + step || !is_inner_link(E[p].link, numSlots)) continue;
            const float a = wd_area(nodes, E[p].src);
            if (best < 0 || a > bestA || (bestA != bestA && a == a)) {   // a NaN loses to every number; ties stay with the lowest position
                best = p;
                bestA = a;
            }
        }
        if (best < 0) break;
        const int slot = inner_index(E[best].link);
        const int2 cc = *reinterpret_cast<const int2*>(nodes + (size_t)slot * kNodeWords + kLinkWord);
#pragma unroll
        for (int p = 2 + step; p > 1; p--)
            if (p > best + 1) E[p] = E[p - 1];
#pragma unroll
        for (int p = 0; p < 2 + step; p++)
            if (p == best) {
                E[p] = WdEntry{cc.x, 2 * slot};
                E[p + 1] = WdEntry{cc.y, 2 * slot + 1};
            }
        n++;
    }
    return n;
}

}  // namespace ntr
