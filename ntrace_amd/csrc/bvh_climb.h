// bvh_climb.h -- the bottom-up pass over a BVHLayout_Compact tree (compact_bvh.h): the topology step that prepares it and the climb,
// once, for the refit (bvh_refit_kernels.hip), for the optimiser's height / SAH-cost passes (bvh_optimize_payload.h, for bvh_optimize_kernels.hip and bvh_optimize_batch_kernels.hip) and for the
// renumbering's subtree counts (bvh_reorder_kernels.hip).
//
// Two launches.  The topology step, one thread per node slot, clears the slot's arrival counter and writes
// parent[child] = 2 * node + k for every inner link.  Parent words are not cleared: one is only believed where the node it names links
// back (parent_links_back), which a stale word of an earlier call cannot.  The root is nobody's child, and a zero-filled slot no link
// reaches reads as "two links at offset 0" and so names nobody.
// The climb starts one thread at every child slot that holds a leaf.  A thread publishes what it knows about (node, k) and arrives at
// the node; the SECOND arrival owns the node: it reads the sibling's payload, forms the node's value, publishes it into the parent's
// slot and arrives there; the first arrival exits.  Nobody waits for anybody, so no forward-progress assumption is made, and a node
// reached by more than two arrivals (not a tree) is owned once (by the arrival that reads 1), so the pass ends on any input.
// The hand-off crosses workgroups and XCDs (a payload a thread reads was written by another CU), in the form lbvh_agglomerate_kernel
// uses for its meeting slots: the payload is written with agent-scope (write-through) relaxed stores, drained with s_waitcnt vmcnt(0),
// then comes the returning agent-scope atomic on the node's counter; the owner reads the sibling's payload with agent-scope relaxed
// loads, served past its L1.  The payload's stores and loads are the callers'; their place relative to the arrival is fixed here.
#pragma once
#include <hip/hip_runtime.h>
#include "compact_bvh.h"

namespace ntr {

enum : int { LINK_NONE = 0, LINK_LEAF, LINK_INNER, LINK_BAD };   // offset 0, a leaf, a node slot of the buffer, anything else

// The topology step for slot `node` (< numSlots): kind[k] classifies link k.  LINK_BAD is c > 0 && !is_inner_link(c), that is
// (c & 63) != 0 || (c >> 6) >= numSlots for c > 0: the one set both the refit and the optimiser report as a malformed child link.
__device__ __forceinline__ void topology_slot(int node, int numSlots, const int* __restrict__ nodes, unsigned int* __restrict__ parent,
                                              unsigned int* __restrict__ arrive, int (&kind)[2])
{
    arrive[node] = 0u;
    const int2 link = *reinterpret_cast<const int2*>(nodes + (size_t)node * kNodeWords + kLinkWord);
    const int c[2] = {link.x, link.y};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        kind[k] = c[k] < 0 ? LINK_LEAF : (c[k] == 0 ? LINK_NONE : (is_inner_link(c[k], numSlots) ? LINK_INNER : LINK_BAD));
        if (kind[k] == LINK_INNER) parent[inner_index(c[k])] = 2u * (unsigned int)node + (unsigned int)k;
    }
}

// The parent word p of `node` is current: the slot it names is inside the buffer and links back here.
__device__ __forceinline__ bool parent_links_back(unsigned int p, int node, int numSlots, const int* nodes)
{
    const int pn = (int)(p >> 1), pk = (int)(p & 1u);
    return pn < numSlots && nodes[(size_t)pn * kNodeWords + kLinkWord + pk] == inner_link(node);
}

// Climbs from child slot k of `node`, whose payload the caller has published (or which holds it already).
//   acquire(node, k)   load the payload of child slot (node, k), the sibling's, with agent-scope loads
//   merge(node, k)     form the node's value from mine (child k) and the sibling's; it becomes mine.  node == 0 is the root, which
//                      reports to no parent: merge does what the pass does with the root's value
//   publish(node, k)   store mine as the payload of child slot (node, k) with agent-scope stores
template <class Publish, class Acquire, class Merge>
__device__ __forceinline__ void climb(int node, int k, int numSlots, const int* nodes, const unsigned int* __restrict__ parent,
                                      unsigned int* __restrict__ arrive, Publish publish, Acquire acquire, Merge merge)
{
    for (;;) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // what the owner will read has reached memory before the arrival is announced
        const unsigned int old = __hip_atomic_fetch_add(&arrive[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != 1u) return;                   // the first to arrive exits
        asm volatile("" ::: "memory");
        acquire(node, k ^ 1);
        merge(node, k);
        if (node == 0) return;
        const unsigned int p = parent[node];
        if (!parent_links_back(p, node, numSlots, nodes)) return;   // no link leads here (a stale parent word)
        node = (int)(p >> 1);
        k = (int)(p & 1u);
        publish(node, k);
    }
}

}  // namespace ntr
