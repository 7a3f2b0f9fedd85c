// bvh_build_kernels.hip -- on-device binned SAH BVH builder for gfx950, one level per round (ntr_persistent_bvh_build).
//
// Rebuilds the reference's persistent BVH builder as it is configured (CudaPersistentBVHBuilder.cpp, persistent_bvh.cu with
// SPLIT_TYPE 5, PLANE_COUNT 32, BINNING_TYPE 2, SAH_TERMINATION, COMPUTE_MEDIAN_BOUNDS) without its persistent task pool or device
// heap.  The spec is the numpy restatement tests/np_bvh_binned.py, which states the rule, its canonical choices and its deviation;
// the header comment of ntr_persistent_bvh_build (include/ntrace_amd.h) lists them too.
//   once per build  bv_prep: each triangle's box and centroid (SoA), its vertex indices checked, the root's reference list 0..n-1
//   per level       bv_bin: per reference and axis the number of the task's planes that put its centroid on side -1 (a prefix, found
//                     by comparisons against the planes, never by a division) is its bin; each (task, axis, bin) gets a count and a
//                     box, in LDS when the workgroup's references share one task, then by float-order integer atomics
//                   bv_decide: one wave per task, one lane per plane: the sweeps over the bins, cost, choice (lowest finite cost,
//                     then lowest plane), children's boxes, termination; tasks without a usable plane are flagged for the median
//                   bv_median_bounds + bv_median_finish: the median split's child boxes and termination for the flagged tasks
//                   bv_task_scan_local + scan_block_sums + bv_task_emit: node numbers, leaf rows, child tasks, child reference
//                     offsets and bin slots by an exclusive scan over the tasks; inner nodes, parent links and leaf terminators
//                   bv_ref_scan_local + scan_block_sums + bv_ref_scatter: each task's child 0 ranks by a scan over the references,
//                     then a stable scatter into the next level's list, or the leaf row of a reference whose task is a leaf
//   end             emit_leaf_rows (device_prims.h): every triangle's three Woop rows and its triIndex entries at its leaf row
// Phases hand data over only at kernel boundaries.  The host reads one 32-byte record per level (the level's totals and the error
// word) to size the next level; nothing else comes back until the build ends.  Outputs go straight into the caller's buffers.
// The plane table, that read-back (read_totals) and the level's bookkeeping (LevelState) are level_build.h's.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "ntr_internal.h"
#include "level_build.h"

namespace ntr {
namespace {

constexpr int BV_BINS = 3 * (kPlanesPerAxis + 1) - 1;  // 12 + 12 + 11
constexpr int BV_SLOT = BV_BINS * 8 + 16;              // words per splitting task: 35 bins of 8 words, then the median boxes
constexpr int BV_BLOCK = 256;
constexpr int BV_MAX_DEPTH = 100;                      // CudaBVH.cpp:701: the CPU tracer's stack; the kernels hold 16 + 88

struct BvTask {         // 40 B
    float lo[3], hi[3];
    int refStart, refCount, parentSlot, binSlot;   // parentSlot: word of the parent's child pointer (-1: root); binSlot -1: a leaf
};
enum : int { BV_LEAF = 1, BV_LEAF0 = 2, BV_LEAF1 = 4, BV_MEDIAN = 8 };
struct BvDecision {     // 64 B
    float lo0[3], hi0[3], lo1[3], hi1[3];
    float split;
    int axis, nL, flags;
};
struct BvPlace {        // a task's global offsets after the task scan
    int childTask, childRef, row, nodeIdx;
};
struct BvTotals : LevelTotals {   // t.z: next level's references, t.w: next level's splitting tasks
    unsigned int median, costLeaves, depthLeaves;
};
struct BvParams {
    int triLimit, triMaxLimit, maxDepth, level;
    float ci, ct, eps, pad;
};

__device__ __forceinline__ float sel4(const float4& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
// getPlaneCentroidPosition (rt_common.cu:449-468) == -1: planeDistance with the plane (-1, 0, 0, pos) is fl(pos - c)
__device__ __forceinline__ bool side_neg(float pos, float c) { return (pos - c) < kPlaneEps; }

// ---- once per build ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BV_BLOCK) void bv_prep(int n, const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                    float4* __restrict__ boxLo, float4* __restrict__ boxHi, float4* __restrict__ cen,
                                                    int* __restrict__ refs, int* __restrict__ taskOf, BvTotals* __restrict__ tot)
{
    const int i = blockIdx.x * BV_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo, c = lo;
    float l[3], h[3];
    if (!tri_box_checked(tri, numVerts, pos, i, l, h)) {
        atomicOr(&tot->err, 1u);
    } else {
        lo = make_float4(l[0], l[1], l[2], 0.f);
        hi = make_float4(h[0], h[1], h[2], 0.f);
        // getCentroid (rt_common.cu:440-444): (mn + mx) * 0.5f
        c = make_float4((l[0] + h[0]) * 0.5f, (l[1] + h[1]) * 0.5f, (l[2] + h[2]) * 0.5f, 0.f);
    }
    boxLo[i] = lo;
    boxHi[i] = hi;
    cen[i] = c;
    refs[i] = i;
    taskOf[i] = 0;
}

// ---- per level: bin ------------------------------------------------------------------------------------------------------
// A bin's 8 words: count, the box's six words (box_words: merged by max, so that zero is the identity of an empty bin), pad.
__device__ __forceinline__ int ref_bin(const float* lo, const float* hi, int a, float c)
{
    const int m = planes_on_axis(a);
    int b = 0;
    const float mn = sel3(lo, a), mx = sel3(hi, a);
    for (int j = 0; j < m; j++) b += side_neg(plane_pos(mn, mx, j), c) ? 1 : 0;
    return b;
}

__global__ __launch_bounds__(BV_BLOCK) void bv_bin(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                   const BvTask* __restrict__ tasks, const float4* __restrict__ boxLo,
                                                   const float4* __restrict__ boxHi, const float4* __restrict__ cen,
                                                   unsigned int* __restrict__ slots)
{
    __shared__ unsigned int sh[BV_BINS * 8];
    const int r0 = blockIdx.x * BV_BLOCK;
    const int r = r0 + threadIdx.x;
    // the references are grouped by task: the workgroup shares one task iff its first and last do
    const int tFirst = taskOf[r0], tLast = taskOf[min(R, r0 + BV_BLOCK) - 1];
    const bool shared = tFirst == tLast;
    if (shared) {
        if (tasks[tFirst].binSlot < 0) return;   // uniform: a leaf task is not binned
        for (int i = threadIdx.x; i < BV_BINS * 8; i += BV_BLOCK) sh[i] = 0u;
        __syncthreads();
    }
    if (r < R) {
        const int t = taskOf[r];
        const BvTask tk = tasks[t];
        if (tk.binSlot >= 0) {
            const int id = refs[r];
            const float4 c = cen[id], bl = boxLo[id], bh = boxHi[id];
            unsigned int w[6];
            box_words(bl, bh, w);
            unsigned int* dst = shared ? sh : slots + (size_t)tk.binSlot * BV_SLOT;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                unsigned int* bin = dst + (a * (kPlanesPerAxis + 1) + ref_bin(tk.lo, tk.hi, a, sel4(c, a))) * 8;
                atomicAdd(&bin[0], 1u);
                atomic_max_box(bin + 1, w);
            }
        }
    }
    if (shared) {
        __syncthreads();
        unsigned int* g = slots + (size_t)tasks[tFirst].binSlot * BV_SLOT;
        for (int i = threadIdx.x; i < BV_BINS * 8; i += BV_BLOCK) {
            const unsigned int v = sh[i];
            if (v == 0u || (i & 7) == 7) continue;
            if ((i & 7) == 0) atomicAdd(&g[i], v);
            else atomicMax(&g[i], v);
        }
    }
}

// ---- per level: decide (one wave per task) -------------------------------------------------------------------------------
// The areas here are box_area (device_prims.h): areaAABB without an invalid-box test.
// taskTerminationCriteria (persistent_bvh.cu:245-271) over the partition; the root is never a leaf (DEVIATION, see the header)
__device__ void finish_decision(const BvTask& tk, BvDecision& d, const BvParams& prm, BvTotals* tot)
{
    const int n = tk.refCount, nL = d.nL, nR = n - nL;
    const float areaP = box_area(tk.lo, tk.hi);
    const float leafCost = prm.ci * (float)n;
    const float leftCost = box_area(d.lo0, d.hi0) / areaP * (float)nL;
    const float rightCost = box_area(d.lo1, d.hi1) / areaP * (float)nR;
    const float subdivisionCost = prm.ct + prm.ci * (leftCost + rightCost);
    bool ended = nL + nR <= prm.triMaxLimit && leafCost < subdivisionCost;
    const bool deep = prm.level > prm.maxDepth - 2;
    bool l0 = nL <= prm.triLimit || deep, l1 = nR <= prm.triLimit || deep;
    if (prm.level == 0 && ended) {
        ended = false;
        l0 = l1 = true;
    }
    if (ended) atomicAdd(&tot->costLeaves, 1u);
    else if (deep) {
        const unsigned int k = (nL > prm.triLimit ? 1u : 0u) + (nR > prm.triLimit ? 1u : 0u);
        if (k) atomicAdd(&tot->depthLeaves, k);
    }
    d.flags = (d.flags & BV_MEDIAN) | (ended ? BV_LEAF : 0) | (l0 ? BV_LEAF0 : 0) | (l1 ? BV_LEAF1 : 0);
}

__global__ __launch_bounds__(BV_BLOCK) void bv_decide(int T, const BvTask* __restrict__ tasks, const unsigned int* __restrict__ slots,
                                                      BvDecision* __restrict__ dec, BvParams prm, BvTotals* __restrict__ tot)
{
    const int t = blockIdx.x * (BV_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;   // wave-uniform
    const BvTask tk = tasks[t];
    if (tk.binSlot < 0) {
        if (lane == 0) {
            BvDecision d;
            memset(&d, 0, sizeof(d));
            d.flags = BV_LEAF;
            dec[t] = d;
        }
        return;
    }
    unsigned long long key = ~0ull;
    float p = 0.f;
    int nL = 0, nR = 0;
    unsigned int w[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // the box words of child 0, then of child 1
    if (lane < kPlanes) {
        const int a = lane / kPlanesPerAxis, j = lane - a * kPlanesPerAxis;
        const int m = a < 2 ? kPlanesPerAxis : kPlanes - 2 * kPlanesPerAxis;
        p = plane_pos(sel3(tk.lo, a), sel3(tk.hi, a), j);
        // plane j: side -1 (child 0) = bins j+1..m, side +1 (child 1) = bins 0..j
        const unsigned int* bins = slots + (size_t)tk.binSlot * BV_SLOT + a * (kPlanesPerAxis + 1) * 8;
        for (int b = 0; b <= m; b++) {
            const uint4 w0 = *(const uint4*)(bins + 8 * b), w1 = *(const uint4*)(bins + 8 * b + 4);
            const unsigned int bw[6] = {w0.y, w0.z, w0.w, w1.x, w1.y, w1.z};
            if (b > j) {
                nL += (int)w0.x;
#pragma unroll
                for (int k = 0; k < 6; k++) w[k] = max(w[k], bw[k]);
            } else {
                nR += (int)w0.x;
#pragma unroll
                for (int k = 0; k < 6; k++) w[6 + k] = max(w[6 + k], bw[k]);
            }
        }
        float l0[3], h0[3], l1[3], h1[3];
        words_box(nL, w, 0.0f, false, l0, h0);   // the cost's boxes carry no epsilon
        words_box(nR, w + 6, 0.0f, false, l1, h1);
        const float s = box_area(l0, h0) * (float)nL + box_area(l1, h1) * (float)nR;
        if (isfinite(s)) key = ((unsigned long long)__float_as_uint(s + 0.0f) << 32) | (unsigned int)lane;   // -0 -> +0
    }
    key = wave_min_u64(key);
    const int kb = (int)(key & 63ull);
    const int nLb = __shfl(nL, kb), nRb = __shfl(nR, kb);
    const float pb = __shfl(p, kb);
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = (unsigned int)__shfl((int)w[k], kb);
    if (lane != 0) return;
    BvDecision d;
    memset(&d, 0, sizeof(d));
    if (key == ~0ull || nLb == 0 || nRb == 0) {   // no split (persistent_bvh.cu:1815-1822, 2301-2303): object median
        d.flags = BV_MEDIAN;
        d.nL = tk.refCount / 2;
        atomicAdd(&tot->median, 1u);
        dec[t] = d;
        return;
    }
    d.split = pb;
    d.axis = kb / kPlanesPerAxis;
    d.nL = nLb;
    words_box(nLb, w, prm.eps, true, d.lo0, d.hi0);   // persistent_bvh.cu:1855-1863
    words_box(nRb, w + 6, prm.eps, true, d.lo1, d.hi1);
    finish_decision(tk, d, prm, tot);
    dec[t] = d;
}

// ---- per level: the median split's boxes (COMPUTE_MEDIAN_BOUNDS) ----------------------------------------------------------
__global__ __launch_bounds__(BV_BLOCK) void bv_median_bounds(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                             const BvTask* __restrict__ tasks, const BvDecision* __restrict__ dec,
                                                             const float4* __restrict__ boxLo, const float4* __restrict__ boxHi,
                                                             unsigned int* __restrict__ slots)
{
    const int r = blockIdx.x * BV_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int t = taskOf[r];
    if (!(dec[t].flags & BV_MEDIAN)) return;
    const BvTask tk = tasks[t];
    const int side = (r - tk.refStart) < tk.refCount / 2 ? 0 : 1;
    unsigned int* m = slots + (size_t)tk.binSlot * BV_SLOT + BV_BINS * 8 + 8 * side;
    const int id = refs[r];
    unsigned int w[6];
    box_words(boxLo[id], boxHi[id], w);
    atomic_max_box(m, w);
}

__global__ __launch_bounds__(BV_BLOCK) void bv_median_finish(int T, const BvTask* __restrict__ tasks, const unsigned int* __restrict__ slots,
                                                             BvDecision* __restrict__ dec, BvParams prm, BvTotals* __restrict__ tot)
{
    const int t = blockIdx.x * BV_BLOCK + threadIdx.x;
    if (t >= T) return;
    BvDecision d = dec[t];
    if (!(d.flags & BV_MEDIAN)) return;
    const BvTask tk = tasks[t];
    const unsigned int* m = slots + (size_t)tk.binSlot * BV_SLOT + BV_BINS * 8;
    words_box(d.nL, m, prm.eps, true, d.lo0, d.hi0);
    words_box(tk.refCount - d.nL, m + 8, prm.eps, true, d.lo1, d.hi1);
    finish_decision(tk, d, prm, tot);
    dec[t] = d;
}

// ---- per level: task scan + emit -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(BV_BLOCK) void bv_task_scan_local(int T, const BvTask* __restrict__ tasks, const BvDecision* __restrict__ dec,
                                                               U4* __restrict__ local, U4* __restrict__ blockSums)
{
    const int t = blockIdx.x * BV_BLOCK + threadIdx.x;
    U4 v{0, 0, 0, 0};
    if (t < T) {
        const BvDecision d = dec[t];
        const unsigned int n = (unsigned int)tasks[t].refCount;
        if (d.flags & BV_LEAF) v = U4{0u, 3u * n + 1u, 0u, 0u};
        else v = U4{1u, 0u, n, (d.flags & BV_LEAF0 ? 0u : 1u) + (d.flags & BV_LEAF1 ? 0u : 1u)};
    }
    scan_local_store<BV_BLOCK>(v, t < T, t, local, blockSums, blockIdx.x);
}

__device__ __forceinline__ BvTask child_task(const float* lo, const float* hi, int refStart, int refCount, int parentSlot, int binSlot)
{
    BvTask c;
    for (int k = 0; k < 3; k++) { c.lo[k] = lo[k]; c.hi[k] = hi[k]; }
    c.refStart = refStart;
    c.refCount = refCount;
    c.parentSlot = parentSlot;
    c.binSlot = binSlot;
    return c;
}

__global__ __launch_bounds__(BV_BLOCK) void bv_task_emit(int T, const BvTask* __restrict__ tasks, const BvDecision* __restrict__ dec,
                                                         const U4* __restrict__ local, const U4* __restrict__ blockSums, int innerBase,
                                                         int rowBase, int nodeCap, int rowCap, int* __restrict__ nodes,
                                                         uint4* __restrict__ woop, int* __restrict__ triIndex, BvTask* __restrict__ next,
                                                         BvPlace* __restrict__ place, BvTotals* __restrict__ tot)
{
    const int t = blockIdx.x * BV_BLOCK + threadIdx.x;
    if (t >= T) return;
    const U4 g = local[t] + blockSums[blockIdx.x];
    const BvDecision d = dec[t];
    const BvTask tk = tasks[t];
    const int n = tk.refCount;
    if (d.flags & BV_LEAF) {
        const int row = rowBase + (int)g.y;
        if (row + 3 * n >= rowCap) { atomicOr(&tot->err, 4u); place[t] = BvPlace{-1, -1, -1, -1}; return; }
        if (tk.parentSlot >= 0) nodes[tk.parentSlot] = leaf_link(row);
        write_leaf_terminator(woop, triIndex, row + 3 * n);
        place[t] = BvPlace{-1, -1, row, -1};
        return;
    }
    const int nodeIdx = innerBase + (int)g.x;
    if (nodeIdx >= nodeCap) { atomicOr(&tot->err, 4u); place[t] = BvPlace{-1, -1, -1, -1}; return; }
    if (tk.parentSlot >= 0) nodes[tk.parentSlot] = inner_link(nodeIdx);
    write_inner_node(nodes, nodeIdx, d.lo0, d.hi0, d.lo1, d.hi1, (d.flags & BV_MEDIAN) ? 0 : d.axis);
    const int ct = 2 * (int)g.x, cr = (int)g.z;
    const bool leaf0 = (d.flags & BV_LEAF0) != 0, leaf1 = (d.flags & BV_LEAF1) != 0;
    next[ct] = child_task(d.lo0, d.hi0, cr, d.nL, kNodeWords * nodeIdx + kLinkWord, leaf0 ? -1 : (int)g.w);
    next[ct + 1] = child_task(d.lo1, d.hi1, cr + d.nL, n - d.nL, kNodeWords * nodeIdx + kLinkWord + 1, leaf1 ? -1 : (int)g.w + (leaf0 ? 0 : 1));
    place[t] = BvPlace{ct, cr, -1, nodeIdx};
}

// ---- per level: reference scan + scatter ---------------------------------------------------------------------------------
__device__ __forceinline__ bool ref_neg(const BvDecision& d, const BvTask& tk, int r, const float4& c)
{
    if (d.flags & BV_MEDIAN) return (r - tk.refStart) < tk.refCount / 2;
    return side_neg(d.split, sel4(c, d.axis));
}

__global__ __launch_bounds__(BV_BLOCK) void bv_ref_scan_local(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                              const BvTask* __restrict__ tasks, const BvDecision* __restrict__ dec,
                                                              const float4* __restrict__ cen, unsigned int* __restrict__ local,
                                                              unsigned int* __restrict__ blockSums)
{
    const int r = blockIdx.x * BV_BLOCK + threadIdx.x;
    unsigned int v = 0u;
    if (r < R) {
        const int t = taskOf[r];
        const BvDecision d = dec[t];
        if (!(d.flags & BV_LEAF)) v = ref_neg(d, tasks[t], r, cen[refs[r]]) ? 1u : 0u;
    }
    scan_local_store<BV_BLOCK>(v, r < R, r, local, blockSums, blockIdx.x);
}

__global__ __launch_bounds__(BV_BLOCK) void bv_ref_scatter(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                           const BvTask* __restrict__ tasks, const BvDecision* __restrict__ dec,
                                                           const BvPlace* __restrict__ place, const float4* __restrict__ cen,
                                                           const unsigned int* __restrict__ local, const unsigned int* __restrict__ blockSums,
                                                           int* __restrict__ nextRefs, int* __restrict__ nextTaskOf, int* __restrict__ leafRow,
                                                           BvTotals* __restrict__ tot)
{
    const int r = blockIdx.x * BV_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int t = taskOf[r];
    const BvDecision d = dec[t];
    const BvPlace pl = place[t];
    const BvTask tk = tasks[t];
    const int id = refs[r];
    const int p = r - tk.refStart;
    if (d.flags & BV_LEAF) {
        if (pl.row >= 0) leafRow[id] = pl.row + 3 * p;
        return;
    }
    if (pl.nodeIdx < 0) return;   // capacity error already flagged
    const int s0 = tk.refStart;
    const unsigned int rank = local[r] + blockSums[r / BV_BLOCK] - (local[s0] + blockSums[s0 / BV_BLOCK]);
    int o;
    int side;
    if (ref_neg(d, tk, r, cen[id])) {
        side = 0;
        o = (int)rank;
        if (rank >= (unsigned int)d.nL) { atomicOr(&tot->err, 2u); return; }
    } else {
        side = 1;
        o = d.nL + (p - (int)rank);
        if (o < d.nL || o >= tk.refCount) { atomicOr(&tot->err, 2u); return; }
    }
    nextRefs[pl.childRef + o] = id;
    nextTaskOf[pl.childRef + o] = pl.childTask + side;
}

// ---- scratch layout ------------------------------------------------------------------------------------------------------
// Everything but the bin slots is sized by the triangle count once: references never duplicate (R <= n) and a level has at most
// n + 1 tasks.  The bin slots come last, so that growing them keeps the rest at its offsets.
struct BvLayout {
    size_t boxLo, boxHi, cen, leafRow, tasks[2], refs[2], taskOf[2], dec, place, tLocal, tBlocks, rLocal, rBlocks, totals, slots, off;
    BvLayout(int64_t n, int64_t slotCap)
    {
        ScratchCarver cv;
        const int64_t T = n + 2, nbT = T / BV_BLOCK + 2, nbR = n / BV_BLOCK + 2;
        boxLo = cv.take((size_t)n * 16);
        boxHi = cv.take((size_t)n * 16);
        cen = cv.take((size_t)n * 16);
        leafRow = cv.take((size_t)n * 4);
        for (int k = 0; k < 2; k++) {
            tasks[k] = cv.take((size_t)T * sizeof(BvTask));
            refs[k] = cv.take((size_t)n * 4);
            taskOf[k] = cv.take((size_t)n * 4);
        }
        dec = cv.take((size_t)T * sizeof(BvDecision));
        place = cv.take((size_t)T * sizeof(BvPlace));
        tLocal = cv.take((size_t)T * sizeof(U4));
        tBlocks = cv.take((size_t)nbT * sizeof(U4));
        rLocal = cv.take((size_t)n * 4);
        rBlocks = cv.take((size_t)(nbR + 1) * 4);   // + the grand total
        totals = cv.take(sizeof(BvTotals));
        slots = cv.take((size_t)slotCap * BV_SLOT * 4);
        off = cv.off;
    }
};

DeviceScratchPool g_bvPool;

// A tree of more than kMaxNodes inner nodes (compact_bvh.h) cannot be written.  Below this bound a node's words (16 * index + 15) fit
// int32 too, and with numTris < 2^28 so do references, tasks (<= n + 1), leaf rows (< 4n + 4) and bin slots (<= n / 2 + 1): no level
// exceeds the kernels' int32 indexing.

int bv_build(int n, const int32_t* d_tri, int32_t numVerts, const float* d_pos, const float* sceneMin, const float* sceneMax,
             const NtrPersistentBvhParams& prm, void* d_nodes, int64_t nodeCap, void* d_woop, int64_t rowCap, int32_t* d_idx,
             NtrPersistentBvhResult* res, hipStream_t s)
{
    const auto wall0 = std::chrono::steady_clock::now();
    // a splitting task other than the root holds at least two references, so a level has at most n / 2 + 1 of them
    const int64_t maxSlots = (int64_t)n / 2 + 1;
    int64_t slotCap = std::max<int64_t>(64, n / 16);
    for (const size_t held = g_bvPool.held(); 2 * slotCap <= maxSlots && BvLayout((int64_t)n, 2 * slotCap).off <= held;) slotCap *= 2;
    BvLayout lay((int64_t)n, slotCap);
    void* base = nullptr;
    if (const int rc = first_block(g_bvPool, lay.off, &base)) return rc;
    StreamEvents<4> ev(s);
    (void)ev.create();
    ev.mark(0);
    NTR_HIP(hipMemsetAsync(at<BvTotals>(base, lay.totals), 0, sizeof(BvTotals), s));
    const int nbN = (n + BV_BLOCK - 1) / BV_BLOCK;
    bv_prep<<<nbN, BV_BLOCK, 0, s>>>(n, d_tri, numVerts, d_pos, at<float4>(base, lay.boxLo), at<float4>(base, lay.boxHi),
                                     at<float4>(base, lay.cen), at<int>(base, lay.refs[0]), at<int>(base, lay.taskOf[0]),
                                     at<BvTotals>(base, lay.totals));
    NTR_HIP(hipGetLastError());
    BvTotals h;
    {
        BvTask root;
        memset(&root, 0, sizeof(root));
        for (int k = 0; k < 3; k++) { root.lo[k] = sceneMin[k]; root.hi[k] = sceneMax[k]; }
        root.refStart = 0;
        root.refCount = n;
        root.parentSlot = -1;
        root.binSlot = 0;
        NTR_HIP(hipMemcpyAsync(at<BvTask>(base, lay.tasks[0]), &root, sizeof(root), hipMemcpyHostToDevice, s));
        if (const int rc = read_totals(&h, at<BvTotals>(base, lay.totals), s)) return rc;   // `root` leaves scope; the vertex check is read
        if (h.err & 1u) return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: vertex index out of range");
    }
    ev.mark(1);

    LevelState lv;
    int64_t R = n, S = 1;
    while (lv.T > 0) {
        if (S > slotCap) {   // grow the bin slots; everything before them keeps its place
            const int64_t nc = std::min<int64_t>(maxSlots, std::max<int64_t>(S, slotCap + slotCap / 2));
            const BvLayout nl((int64_t)n, nc);
            const size_t keep = lay.slots;
            const int rc = g_bvPool.regrow(nl.off, &base, [&](void* from, void* to) {
                hipError_t e = hipMemcpyAsync(to, from, keep, hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                return e == hipSuccess ? (int)NTR_OK : hip_fail(e, "BVH builder scratch move");
            });
            if (rc != NTR_OK) return rc;
            slotCap = nc;
            lay = nl;
        }
        const int Ti = (int)lv.T, Ri = (int)R;
        const int nbT = (Ti + BV_BLOCK - 1) / BV_BLOCK, nbR = (Ri + BV_BLOCK - 1) / BV_BLOCK;
        BvParams kp{prm.triLimit, prm.triMaxLimit, prm.maxDepth, lv.level, prm.ci, prm.ct, prm.epsilon, 0.f};
        // resolved per level: growing the slots moves the block
        BvTask *tasks = at<BvTask>(base, lay.tasks[lv.cur]), *next = at<BvTask>(base, lay.tasks[lv.nxt()]);
        int *refs = at<int>(base, lay.refs[lv.cur]), *nextRefs = at<int>(base, lay.refs[lv.nxt()]);
        int *taskOf = at<int>(base, lay.taskOf[lv.cur]), *nextTaskOf = at<int>(base, lay.taskOf[lv.nxt()]);
        float4 *boxLo = at<float4>(base, lay.boxLo), *boxHi = at<float4>(base, lay.boxHi), *cen = at<float4>(base, lay.cen);
        BvDecision* dec = at<BvDecision>(base, lay.dec);
        BvPlace* place = at<BvPlace>(base, lay.place);
        U4 *tLocal = at<U4>(base, lay.tLocal), *tBlocks = at<U4>(base, lay.tBlocks);
        unsigned int *rLocal = at<unsigned int>(base, lay.rLocal), *rBlocks = at<unsigned int>(base, lay.rBlocks);
        unsigned int* slots = at<unsigned int>(base, lay.slots);
        BvTotals* tot = at<BvTotals>(base, lay.totals);
        if (S > 0) NTR_HIP(hipMemsetAsync(slots, 0, (size_t)S * BV_SLOT * 4, s));
        NTR_HIP(hipMemsetAsync(&tot->t, 0, sizeof(U4), s));
        if (S > 0 && Ri > 0) bv_bin<<<nbR, BV_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, boxLo, boxHi, cen, slots);
        bv_decide<<<(Ti + 3) / 4, BV_BLOCK, 0, s>>>(Ti, tasks, slots, dec, kp, tot);
        if (S > 0 && Ri > 0) {
            bv_median_bounds<<<nbR, BV_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, dec, boxLo, boxHi, slots);
            bv_median_finish<<<nbT, BV_BLOCK, 0, s>>>(Ti, tasks, slots, dec, kp, tot);
        }
        bv_task_scan_local<<<nbT, BV_BLOCK, 0, s>>>(Ti, tasks, dec, tLocal, tBlocks);
        scan_block_sums<BV_BLOCK, U4><<<1, BV_BLOCK, 0, s>>>(nbT, tBlocks, tBlocks, &tot->t);
        bv_task_emit<<<nbT, BV_BLOCK, 0, s>>>(Ti, tasks, dec, tLocal, tBlocks, (int)lv.innerBase, (int)lv.rowBase, (int)nodeCap, (int)rowCap,
                                              (int*)d_nodes, (uint4*)d_woop, d_idx, next, place, tot);
        if (Ri > 0) {
            bv_ref_scan_local<<<nbR, BV_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, dec, cen, rLocal, rBlocks);
            scan_block_sums<BV_BLOCK, unsigned int><<<1, BV_BLOCK, 0, s>>>(nbR, rBlocks, rBlocks, rBlocks + nbR);
            bv_ref_scatter<<<nbR, BV_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, dec, place, cen, rLocal, rBlocks, nextRefs, nextTaskOf,
                                                    at<int>(base, lay.leafRow), tot);
        }
        NTR_HIP(hipGetLastError());
        if (const int rc = read_totals(&h, tot, s)) return rc;
        if (const int rc = lv.check_nodes("ntr_persistent_bvh_build", h.t.x)) return rc;
        if (h.err)
            return set_error(NTR_ERR_LAYOUT, "ntr_persistent_bvh_build: internal check failed: error 0x%x at level %d", h.err, lv.level);
        lv.advance(h.t.x, h.t.y);
        R = h.t.z;
        S = h.t.w;
    }
    ev.mark(2);
    BvTotals* tot = at<BvTotals>(base, lay.totals);
    emit_leaf_rows<BV_BLOCK><<<nbN, BV_BLOCK, 0, s>>>(n, d_tri, d_pos, (const unsigned char*)nullptr, at<int>(base, lay.leafRow), (int)rowCap,
                                                      (float4*)d_woop, d_idx, &tot->err, 4u);
    NTR_HIP(hipGetLastError());
    ev.mark(3);
    if (const int rc = read_totals(&h, tot, s)) return rc;
    if (h.err) return set_error(NTR_ERR_LAYOUT, "ntr_persistent_bvh_build: internal check failed: error 0x%x in the leaf emit", h.err);

    fill_bvh_result(res, lv);
    res->medianFallbacks = (int32_t)h.median;   // counted over the whole build
    res->costLeaves = (int32_t)h.costLeaves;
    res->depthLeaves = (int32_t)h.depthLeaves;
    res->prepMs = ev.ms(0, 1);
    res->levelsMs = ev.ms(1, 2);
    res->emitMs = ev.ms(2, 3);
    res->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_persistent_bvh_params_default(NtrPersistentBvhParams* p)
{
    if (!p) return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_params_default: null");
    memset(p, 0, sizeof(*p));
    p->triLimit = 16;      // config.conf, block PersistentBVH
    p->triMaxLimit = 16;
    p->maxDepth = 50;
    p->ci = 1.0f;
    p->ct = 1.0f;
    p->epsilon = FLT_EPSILON;   // Renderer.cpp:264
    return NTR_OK;
}

int ntr_persistent_bvh_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                             const float sceneMin[3], const float sceneMax[3], const NtrPersistentBvhParams* params,
                             void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                             int32_t* d_triIndex, int64_t triIndexCapacity, NtrPersistentBvhResult* result, void* stream)
{
    if (!result) return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: null result");
    memset(result, 0, sizeof(*result));
    if (const int rc = check_build_geometry("ntr_persistent_bvh_build", numTris, numVerts, d_triVtxIndex, d_vtxPos, sceneMin && sceneMax,
                                            " and scene box"))
        return rc;
    NtrPersistentBvhParams p;
    ntr_persistent_bvh_params_default(&p);
    if (params) p = *params;
    if (p.triLimit < 1 || p.triMaxLimit < 0)
        return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: triLimit < 1 or triMaxLimit < 0");
    if (p.maxDepth < 1 || p.maxDepth > BV_MAX_DEPTH)
        return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: maxDepth %d outside 1..%d (the tracers' stacks)", (int)p.maxDepth,
                         BV_MAX_DEPTH);
    if (!std::isfinite(p.ci) || !std::isfinite(p.ct) || !std::isfinite(p.epsilon) || p.epsilon < 0.0f)
        return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: ci, ct and epsilon must be finite, epsilon >= 0");
    // the bins need plane positions that do not decrease along an axis: a finite box with min <= max (children's boxes then have it
    // too, as epsilon >= 0 only grows them)
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(sceneMin[k]) || !std::isfinite(sceneMax[k]) || !(sceneMin[k] <= sceneMax[k]))
            return set_error(NTR_ERR_INVALID, "ntr_persistent_bvh_build: scene box axis %d is [%g, %g]; it must be finite with min <= max", k,
                             (double)sceneMin[k], (double)sceneMax[k]);
    int64_t nodeCap, rowCap;
    if (const int rc = check_build_outputs("ntr_persistent_bvh_build", numTris, d_nodes, nodesCapacity, d_triWoop, triWoopCapacity, d_triIndex,
                                           triIndexCapacity, &nodeCap, &rowCap))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    return finish_build(bv_build(numTris, d_triVtxIndex, numVerts, d_vtxPos, sceneMin, sceneMax, p, d_nodes, nodeCap, d_triWoop, rowCap,
                                 d_triIndex, result, s), result, s);
}

int ntr_persistent_bvh_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_persistent_bvh_scratch_bytes", g_bvPool, bytes); }

}  // extern "C"
