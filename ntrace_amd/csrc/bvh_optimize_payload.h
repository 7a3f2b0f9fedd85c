// bvh_optimize_payload.h -- what the optimiser's height pass and the SAH-cost pass carry up a BVHLayout_Compact tree, stated once for
// the single-tree unit (bvh_optimize_kernels.hip) and the pool unit (bvh_optimize_batch_kernels.hip): the report of a tree's slot 0,
// the payload a child hands its node, its agent-scope stores and loads, calcSAHNode's arithmetic, and the climb of one child word
// (bvh_climb.h's climb with that payload).  The callers differ only in where a tree's arrays begin: a pool unit hands every pointer
// already moved to the thread's own BLAS.
#pragma once
#include <hip/hip_runtime.h>

#include "bvh_climb.h"
#include "device_prims.h"

namespace ntr {
namespace {   // a unit's own copy: the kernels' names keep the unit's anonymous namespace

enum : unsigned int { OP_ERR_LINK = 1u, OP_ERR_ROW = 2u };

struct OpRoot {                              // what the owner of slot 0 reports; `done` stays 0 if the climb never got there
    unsigned int done, height, leafLinks, slots, leaves, tris, err;
    float sah;
    unsigned int pad[8];
};
static_assert(sizeof(OpRoot) == 64, "OpRoot must be 64 bytes");

// What a child reports to its node.  SAH: three 8-byte words (value | height, leaves | triangles, slots); else one (height | leaf links).
template <bool SAH>
struct OpInfo {
    unsigned int height, leafLinks, slots, leaves, tris;
    float value;
};
template <bool SAH>
__device__ __forceinline__ void op_publish(unsigned long long* info, size_t child, const OpInfo<SAH>& v)
{
    if (SAH) {
        unsigned long long* p = info + 3 * child;
        __hip_atomic_store(p, (unsigned long long)__float_as_uint(v.value) | ((unsigned long long)v.height << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 1, (unsigned long long)v.leaves | ((unsigned long long)v.tris << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 2, (unsigned long long)v.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __hip_atomic_store(info + child, (unsigned long long)v.height | ((unsigned long long)v.leafLinks << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <bool SAH>
__device__ __forceinline__ void op_acquire(const unsigned long long* info, size_t child, OpInfo<SAH>& v)
{
    v = OpInfo<SAH>();
    if (SAH) {
        const unsigned long long* p = info + 3 * child;
        const unsigned long long a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.value = __uint_as_float((unsigned int)a); v.height = (unsigned int)(a >> 32);
        v.leaves = (unsigned int)b; v.tris = (unsigned int)(b >> 32);
        v.slots = (unsigned int)c;
    } else {
        const unsigned long long a = __hip_atomic_load(info + child, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.height = (unsigned int)a; v.leafLinks = (unsigned int)(a >> 32);
    }
}

// fminf / fmaxf of calcSAHNode pinned: the other operand for a NaN, else by the total order -0 < +0
__device__ __forceinline__ float op_fmin(float a, float b) { return a != a ? b : (b != b ? a : ord_min(a, b)); }
__device__ __forceinline__ float op_fmax(float a, float b) { return a != a ? b : (b != b ? a : ord_max(a, b)); }
// 2 * ((dx*dy + dy*dz) + dz*dx), left to right (emitTreeKernel.cu:1374-1376); the units that include this are compiled without contraction
__device__ __forceinline__ float op_sah_area(float xi, float xa, float yi, float ya, float zi, float za)
{
    const float dx = xa - xi, dy = ya - yi, dz = za - zi;
    return 2.0f * ((dx * dy + dy * dz) + dz * dx);
}

// The climb from child word k of `node`, which is no inner link: a leaf link, a word 0, or a link outside the extent.  Every array is
// the tree's own (numSlots slots, numRows rows; info holds 2 * numSlots payloads, 3 words each with SAH); `root` is the tree's report.
// tallest (or null): a word that keeps the greatest height any tree has reported, for a unit that climbs many trees in one launch.
template <bool SAH>
__device__ __forceinline__ void op_climb_child(int node, int k, int numSlots, const int* nodes, int numRows,
                                               const float4* woop, const unsigned int* parent,
                                               unsigned int* arrive, unsigned long long* info,
                                               int* height, unsigned int* leafLinks, OpRoot* root,
                                               unsigned int* tallest)
{
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (is_inner_link(link, numSlots)) return;   // an inner child arrives with the owner of its node
    OpInfo<SAH> mine = OpInfo<SAH>();
    mine.leafLinks = 1u;
    if (SAH && link < 0) {
        mine.leaves = 1u;
        long long r = (long long)leaf_row(link);
        while (r < numRows && __float_as_uint(woop[r].x) != kLeafTerm) {   // calcLeafs (emitTreeKernel.cu:1351-1359), inside the extent
            mine.tris++;
            r += 3;
        }
        if (r >= numRows) atomicOr(&root->err, OP_ERR_ROW);
        mine.value = (float)mine.tris;
    }
    OpInfo<SAH> sib;
    const auto publish = [&](int n, int ck) { op_publish<SAH>(info, 2 * (size_t)n + ck, mine); };
    const auto acquire = [&](int n, int ck) { op_acquire<SAH>(info, 2 * (size_t)n + ck, sib); };
    const auto merge = [&](int n, int ck) {
        OpInfo<SAH> up = OpInfo<SAH>();
        up.height = 1u + max(mine.height, sib.height);
        up.leafLinks = mine.leafLinks + sib.leafLinks;
        if (SAH) {
            up.slots = 1u + mine.slots + sib.slots;
            up.leaves = mine.leaves + sib.leaves;
            up.tris = mine.tris + sib.tris;
            const float* nf = reinterpret_cast<const float*>(nodes + (size_t)n * kNodeWords);
            const float4 n0 = *reinterpret_cast<const float4*>(nf), n1 = *reinterpret_cast<const float4*>(nf + 4),
                         n2 = *reinterpret_cast<const float4*>(nf + 8);
            const float pa = op_sah_area(op_fmin(n0.x, n1.x), op_fmax(n0.y, n1.y), op_fmin(n0.z, n1.z), op_fmax(n0.w, n1.w),
                                         op_fmin(n2.x, n2.z), op_fmax(n2.y, n2.w));
            const float pl = op_sah_area(n0.x, n0.y, n0.z, n0.w, n2.x, n2.y);
            const float pr = op_sah_area(n1.x, n1.y, n1.z, n1.w, n2.z, n2.w);
            const float l = ck == 0 ? mine.value : sib.value, r = ck == 0 ? sib.value : mine.value;
            up.value = (1.0f + (pl / pa) * l) + (pr / pa) * r;
        } else {
            height[n] = (int)up.height;
            leafLinks[n] = up.leafLinks;
        }
        if (n == 0) {                         // the root reports to no parent
            root->height = up.height; root->leafLinks = up.leafLinks; root->slots = up.slots; root->leaves = up.leaves;
            root->tris = up.tris; root->sah = up.value; root->done = 1u;
            if (tallest) atomicMax(tallest, up.height);
        }
        mine = up;
    };
    publish(node, k);
    climb(node, k, numSlots, nodes, parent, arrive, publish, acquire, merge);
}

}  // namespace
}  // namespace ntr
