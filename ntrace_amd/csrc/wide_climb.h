// wide_climb.h -- the bottom-up pass over a 4-wide tree (wide_bvh.h), once, for the refit of a wide pool (wide_refit_batch_kernels.hip)
// and of a wide top-level tree (tlas_wide_refit_kernels.hip).  The rule is tests/np_wide_refit.py.
//
// It is bvh_climb.h's pass with one difference: a node waits for its `count` (2..4) slots, not for two.  climb() of bvh_climb.h was NOT
// given the count as a parameter: its owner is "the arrival that reads 1" and its payload "the sibling's", both in the callers' lambdas,
// so every existing instance would have changed; the wide climb is stated here instead.
// Two launches.  The topology step, one thread per wide node, clears the node's arrival counter and writes
// parent[child] = 4 * node + k for every link > 0 of a slot k < count.  Parent words are not cleared: one is only believed where the
// slot it names links back (wide_parent_links_back), which a stale word of an earlier call cannot.
// The climb starts one thread at every slot k < count whose link is <= 0: a leaf's thread publishes the leaf's box into the slot first,
// the thread of a link 0 (an empty slot, which keeps its box and takes part in the union) only arrives.  The arrival that completes the
// node's count owns it: it reads the count boxes, folds them in the integer order, writes the padding slots (slot k >= count is a copy of
// slot 0's box), publishes the union into the parent's slot and arrives there.  Nobody waits for anybody.  A node is owned at most once
// (by the arrival that reads count - 1; a counter only rises) and an owner arrives at one parent slot, so a slot receives at most one
// arrival, no counter rises above 4 and the pass ends on any input.  A node named by two links climbs to the namer whose parent word
// was written last; the other namer finds the word is not its own (wide_names_child) and reports the tree as malformed.
// The hand-off crosses workgroups and XCDs exactly as bvh_climb.h's: a box is three aligned 8-byte granules written with agent-scope
// (write-through) relaxed stores, drained with s_waitcnt vmcnt(0) before the returning agent-scope atomic on the node's counter; the
// owner reads the boxes with agent-scope relaxed loads, served past its L1.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_climb.h"
#include "device_prims.h"
#include "wide_bvh.h"

namespace ntr {

// wide_box_word(k, 0 / 2 / 4) is even for every k (the host entry points check it), so a granule is 8-byte aligned in a 128-byte node
__device__ __forceinline__ void wide_publish_box(int* nodes, int node, int k, const float (&b)[6])
{
    unsigned long long* p = reinterpret_cast<unsigned long long*>(nodes + (size_t)node * kWideWords);
#pragma unroll
    for (int j = 0; j < 6; j += 2)
        __hip_atomic_store(p + wide_box_word(k, j) / 2,
                           (unsigned long long)__float_as_uint(b[j]) | ((unsigned long long)__float_as_uint(b[j + 1]) << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wide_acquire_box(const int* nodes, int node, int k, float (&b)[6])
{
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(nodes + (size_t)node * kWideWords);
#pragma unroll
    for (int j = 0; j < 6; j += 2) {
        const unsigned long long w = __hip_atomic_load(p + wide_box_word(k, j) / 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b[j] = __uint_as_float((unsigned int)w);
        b[j + 1] = __uint_as_float((unsigned int)(w >> 32));
    }
}
inline bool wide_box_granules_aligned()
{
    for (int k = 0; k < kWideChildren; k++)
        for (int j = 0; j < 6; j += 2)
            if ((wide_box_word(k, j) & 1) || wide_box_word(k, j + 1) != wide_box_word(k, j) + 1) return false;
    return true;
}

__device__ __forceinline__ bool wide_count_ok(int count) { return count >= 2 && count <= kWideChildren; }
// a link that names a wide node of a tree of numNodes nodes (other than the root: offset 0 is nobody's child)
__device__ __forceinline__ bool is_wide_link(int c, int numNodes) { return c > 0 && (c & (kWideBytes - 1)) == 0 && c / kWideBytes < numNodes; }

// The union of slots 0..count-1 of `node` (count checked by the caller) as lo.x hi.x lo.y hi.y lo.z hi.z; first: slot 0's box
__device__ __forceinline__ void wide_node_union(const int* nodes, int node, int count, float (&box)[6], float (&first)[6])
{
    wide_acquire_box(nodes, node, 0, first);
#pragma unroll
    for (int j = 0; j < 6; j++) box[j] = first[j];
    for (int s = 1; s < count; s++) {
        float other[6];
        wide_acquire_box(nodes, node, s, other);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            box[2 * q] = ord_min(box[2 * q], other[2 * q]);
            box[2 * q + 1] = ord_max(box[2 * q + 1], other[2 * q + 1]);
        }
    }
}

// The topology step for wide node `node` (< numNodes): kind[k] classifies slot k (LINK_NONE for k >= count, whose link nobody reads).
// -> false: the count word lies outside 2..4 -- the node has no slots, nobody arrives at it and nothing above it is rewritten.
__device__ __forceinline__ bool wide_topology_node(int node, int numNodes, const int* __restrict__ nodes, unsigned int* __restrict__ parent,
                                                   unsigned int* __restrict__ arrive, int (&kind)[kWideChildren])
{
    arrive[node] = 0u;
    const int4 link = *reinterpret_cast<const int4*>(nodes + (size_t)node * kWideWords + kWideLinkWord);
    const int count = nodes[(size_t)node * kWideWords + kWideCountWord];
    const int c[kWideChildren] = {link.x, link.y, link.z, link.w};
#pragma unroll
    for (int k = 0; k < kWideChildren; k++) {
        kind[k] = !wide_count_ok(count) || k >= count ? LINK_NONE
                  : c[k] < 0                          ? LINK_LEAF
                                                      : (c[k] == 0 ? LINK_NONE : (is_wide_link(c[k], numNodes) ? LINK_INNER : LINK_BAD));
        if (kind[k] == LINK_INNER) parent[c[k] / kWideBytes] = 4u * (unsigned int)node + (unsigned int)k;
    }
    return wide_count_ok(count);
}

// The parent word of the node that slot k of `node` names (an inner link the caller has checked) is this slot's: no other link names it
__device__ __forceinline__ bool wide_names_child(const unsigned int* __restrict__ parent, int node, int k, int link)
{
    return parent[link / kWideBytes] == 4u * (unsigned int)node + (unsigned int)k;
}

// The parent word p of `node` is current: the slot it names is a slot of a node of the tree and links back here
__device__ __forceinline__ bool wide_parent_links_back(unsigned int p, int node, int numNodes, const int* nodes)
{
    const int pn = (int)(p >> 2), pk = (int)(p & 3u);
    if (pn >= numNodes) return false;
    const int count = nodes[(size_t)pn * kWideWords + kWideCountWord];
    return wide_count_ok(count) && pk < count && nodes[(size_t)pn * kWideWords + kWideLinkWord + pk] == wide_link(node);
}

// Arrives at `node`, one of whose slots the caller has published (or which holds its box already), and climbs while the arrival
// completes a node.  rootBox (or null) receives node 0's union as min.xyz max.xyz, and so does rootCopy.
__device__ __forceinline__ void wide_climb(int node, int numNodes, int* nodes, const unsigned int* __restrict__ parent,
                                           unsigned int* __restrict__ arrive, float* rootBox, float* rootCopy = nullptr)
{
    for (;;) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // what the owner will read has reached memory before the arrival is announced
        const unsigned int old = __hip_atomic_fetch_add(&arrive[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int count = nodes[(size_t)node * kWideWords + kWideCountWord];   // (topology: nobody writes it)
        if (!wide_count_ok(count) || old != (unsigned int)(count - 1)) return;
        asm volatile("" ::: "memory");
        float box[6], first[6];
        wide_node_union(nodes, node, count, box, first);
        for (int s = count; s < kWideChildren; s++) {      // the padding: nobody else reads or writes these words in this launch
            float* nf = reinterpret_cast<float*>(nodes + (size_t)node * kWideWords);
#pragma unroll
            for (int j = 0; j < 6; j++) nf[wide_box_word(s, j)] = first[j];
        }
        if (node == 0) {                         // the root reports to no parent
            if (rootBox) {
                rootBox[0] = box[0]; rootBox[1] = box[2]; rootBox[2] = box[4];
                rootBox[3] = box[1]; rootBox[4] = box[3]; rootBox[5] = box[5];
            }
            if (rootCopy) {
                rootCopy[0] = box[0]; rootCopy[1] = box[2]; rootCopy[2] = box[4];
                rootCopy[3] = box[1]; rootCopy[4] = box[3]; rootCopy[5] = box[5];
            }
            return;
        }
        const unsigned int p = parent[node];
        if (!wide_parent_links_back(p, node, numNodes, nodes)) return;   // no link leads here (a stale parent word)
        node = (int)(p >> 2);
        wide_publish_box(nodes, node, (int)(p & 3u), box);
    }
}

}  // namespace ntr
