// sah_build_kernels.hip -- on-device full-sweep SAH BVH builder for gfx950, one level per round (ntr_sah_device_build).
//
// Builds the tree of the host SAH builder (host/bvh/SAHBVHBuilder.cpp; the reference's src/rt/bvh/SAHBVHBuilder.cpp:51-254 with
// Platform("GPU")) node for node and triangle for triangle.  The spec is the numpy restatement tests/np_sah_sweep.py; the header
// comment of ntr_sah_device_build (include/ntrace_amd.h) lists the rule too.  The host builder's formulation is level-synchronous
// already: the three axis orders are sorted once, every node owns the same range [begin, end) of all three, and a split
// stable-partitions the two other orders inside that range.  Ranges never move, so a position of the arrays belongs to one task of
// the level (taskOf) or to a leaf that is done (-1).
//   once per build  sw_prep: each triangle's box, the drop test, its vertex indices checked, the root's box (ord_enc words, integer max)
//                   sw_live_scan_local + scan_block_sums + sw_live_scatter: the live triangles in ascending id with their three keys
//                   sw_hist + 3 x 4 one-sweep passes (radix_sort.h) on ord_enc(key + 0.0f): stable from ascending ids, the host's order
//   per level       sw_task_begin: leaf tests before the search, nodeSAH / leafSAH, the search's accumulators cleared
//                   sw_seg_local + sw_seg_sums: per axis a segmented prefix and a segmented suffix union of the boxes (segments =
//                     tasks), workgroup aggregates first, one workgroup carries them across
//                   sw_sah: the scans again with the carries; sah per position and axis, the task's lowest sah by integer min
//                   sw_pick: among the positions that hold that sah the lowest (balance, axis, i), one 64-bit integer min
//                   sw_decide_scan_local + scan_block_sums: the winner, the leaf test after the search; node numbers and leaf rows
//                   sw_mark: the side of every triangle of a split task; the children's boxes by integer max
//                   sw_task_emit: inner nodes, parent links, leaf terminators, the next level's tasks
//                   sw_ref_scan_local + scan_block_sums + sw_ref_scatter: per axis each task's child 0 ranks, then the stable
//                     partition into the other buffer; the leaf row of every triangle of a task that became a leaf
//   end             emit_leaf_rows (device_prims.h): every live triangle's three Woop rows and its triIndex entries at its leaf row
// Box unions are exact, so any grouping of the scans gives the host's areas; every cost expression keeps the spec's order of
// operations (the library is compiled without contraction).  The host reads one 32-byte record per level (read_totals, LevelState: level_build.h).
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "ntr_internal.h"
#include "level_build.h"
#include "radix_sort.h"

namespace ntr {
namespace {

constexpr int SW_BLOCK = 256;                 // per-task and per-triangle kernels
constexpr int SW_PB = 512;                    // per-position kernels: fewer workgroup aggregates for the one workgroup that carries them
constexpr int SW_SUMS = 1024;
constexpr int SW_MAX_DEPTH = 64;              // SAHBVHBuilder.hpp MaxDepth
constexpr int SW_SORT_ITEMS = 8;
constexpr int SW_HIST_BLOCKS = 512;
constexpr int SW_SEARCH = -2, SW_INNER = -1;  // task states; >= 0: a leaf listed by that axis' sequence

struct SwTask {         // 40 B
    float lo[3], hi[3];
    int begin, end, parentSlot, arranged;   // parentSlot: word of the parent's child link (-1: root); arranged: axis of the last partition
};
struct SwDecision { int state, axis, numLeft, pad; };
struct SwPlace { int childTask, row, nodeIdx, pad; };
struct SwCost { float leafSah, nodeSah; };
struct SwTotals : LevelTotals {   // err bit 1 also: a leaf row outside the buffers at the leaf emit
    unsigned int live, pad[2];
};
// w: a box as six words merged by integer max (box_words, device_prims.h).  flag: a segment starts here.
struct SwSeg {
    unsigned int w[6], flag, pad;
};
__device__ __forceinline__ SwSeg seg_join(const SwSeg& a /* earlier */, const SwSeg& b /* later */)
{
    if (b.flag) return b;
    SwSeg r;
#pragma unroll
    for (int k = 0; k < 6; k++) r.w[k] = max(a.w[k], b.w[k]);
    r.flag = a.flag;
    r.pad = 0u;
    return r;
}
__device__ __forceinline__ SwSeg seg_zero() { return SwSeg{}; }

// Exclusive segmented scan over a workgroup: lane shuffles inside a wave, the waves' joins through LDS (sh[THREADS / 64]); *total is
// the join of all values.  Every thread of the workgroup calls it.
__device__ __forceinline__ SwSeg seg_shfl_up(const SwSeg& v, int off)
{
    SwSeg o;
#pragma unroll
    for (int k = 0; k < 6; k++) o.w[k] = (unsigned int)__shfl_up((int)v.w[k], off);
    o.flag = (unsigned int)__shfl_up((int)v.flag, off);
    o.pad = 0u;
    return o;
}
template <int THREADS>
__device__ SwSeg seg_block_exclusive(const SwSeg& v, SwSeg* total, SwSeg* sh)
{
    constexpr int WAVES = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SwSeg inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const SwSeg o = seg_shfl_up(inc, off);
        if (lane >= off) inc = seg_join(o, inc);
    }
    if (lane == 63) sh[wave] = inc;
    SwSeg ex = seg_shfl_up(inc, 1);
    if (lane == 0) ex = seg_zero();
    __syncthreads();
    SwSeg before = seg_zero(), all = seg_zero();
#pragma unroll 1
    for (int w = 0; w < WAVES; w++) {
        const SwSeg t = sh[w];
        if (w < wave) before = seg_join(before, t);
        all = seg_join(all, t);
    }
    *total = all;
    __syncthreads();   // sh is reused by the next call
    return seg_join(before, ex);
}

__device__ __forceinline__ float fw_min(float a, float b) { return a < b ? a : b; }   // FW::min
__device__ __forceinline__ float fw_max(float a, float b) { return a > b ? a : b; }
// The areas here are box_area_valid / words_area (device_prims.h): AABB::area, 0 for an invalid box.

// ---- once per build ---------------------------------------------------------------------------------------------------
// rootWords[6]: the union of every triangle's box, the dropped ones too (SAHBVHBuilder.cpp run(), reference :70-84)
__global__ __launch_bounds__(SW_BLOCK) void sw_prep(int n, const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                    float4* __restrict__ boxLo, float4* __restrict__ boxHi,
                                                    unsigned char* __restrict__ liveFlag, unsigned int* __restrict__ rootWords,
                                                    SwTotals* __restrict__ tot)
{
    const int i = blockIdx.x * SW_BLOCK + threadIdx.x;
    unsigned int w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (i < n) {
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        bool live = false;
        float l[3], h[3];
        if (!tri_box_checked(tri, numVerts, pos, i, l, h)) {
            atomicOr(&tot->err, 1u);
        } else {
            const float sz[3] = {h[0] - l[0], h[1] - l[1], h[2] - l[2]};
            lo = make_float4(l[0], l[1], l[2], 0.f);
            hi = make_float4(h[0], h[1], h[2], 0.f);
            // reference :141-151: a negative extent, or at most one non-zero extent
            const float smin = fw_min(fw_min(sz[0], sz[1]), sz[2]), smax = fw_max(fw_max(sz[0], sz[1]), sz[2]);
            const float ssum = sz[0] + sz[1] + sz[2];
            live = !(smin < 0.0f || ssum == smax);
            box_words(lo, hi, w);
        }
        boxLo[i] = lo;
        boxHi[i] = hi;
        liveFlag[i] = live ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const unsigned int m = wave_max_u32(w[k]);
        if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(&rootWords[k], m);
    }
}

__global__ __launch_bounds__(SW_BLOCK) void sw_live_scan_local(int n, const unsigned char* __restrict__ liveFlag,
                                                               unsigned int* __restrict__ local, unsigned int* __restrict__ blockSums)
{
    const int i = blockIdx.x * SW_BLOCK + threadIdx.x;
    const unsigned int v = i < n ? (unsigned int)liveFlag[i] : 0u;
    scan_local_store<SW_BLOCK>(v, i < n, i, local, blockSums, blockIdx.x);
}

// the live triangles in ascending id; key on axis d = fl(min[d] + max[d]), as ord_enc(key + 0.0f): -0 and +0 sort as equal
__global__ __launch_bounds__(SW_BLOCK) void sw_live_scatter(int n, int cap, const unsigned char* __restrict__ liveFlag,
                                                            const unsigned int* __restrict__ local, const unsigned int* __restrict__ blockSums,
                                                            const float4* __restrict__ boxLo, const float4* __restrict__ boxHi,
                                                            int* __restrict__ liveIds, unsigned int* __restrict__ keys /* [3][cap] */)
{
    const int i = blockIdx.x * SW_BLOCK + threadIdx.x;
    if (i >= n || !liveFlag[i]) return;
    const unsigned int j = local[i] + blockSums[blockIdx.x];
    if (j >= (unsigned int)n) return;
    const float4 lo = boxLo[i], hi = boxHi[i];
    liveIds[j] = i;
    keys[j] = ord_enc((lo.x + hi.x) + 0.0f);
    keys[(size_t)cap + j] = ord_enc((lo.y + hi.y) + 0.0f);
    keys[2 * (size_t)cap + j] = ord_enc((lo.z + hi.z) + 0.0f);
}

// digit histograms of the three sorts' four passes: hist[axis][pass][256]; the one-sweep tile state is cleared on the way
__global__ __launch_bounds__(SW_BLOCK) void sw_hist(int m, int cap, const unsigned int* __restrict__ keys, unsigned int* __restrict__ hist,
                                                    unsigned long long* __restrict__ tileState, int tileStateWords)
{
    __shared__ unsigned int s_hist[12 * 256];
    for (int i = threadIdx.x; i < 12 * 256; i += SW_BLOCK) s_hist[i] = 0u;
    const int gtid = blockIdx.x * SW_BLOCK + threadIdx.x, gstride = gridDim.x * SW_BLOCK;
    for (int i = gtid; i < tileStateWords; i += gstride) tileState[i] = 0ull;
    __syncthreads();
    for (int j = gtid; j < m; j += gstride) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const unsigned int k = keys[(size_t)d * cap + j];
#pragma unroll
            for (int p = 0; p < 4; p++) atomicAdd(&s_hist[(d * 4 + p) * 256 + ((k >> (8 * p)) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 12 * 256; i += SW_BLOCK)
        if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

__global__ void sw_root(const unsigned int* __restrict__ rootWords, const SwTotals* __restrict__ tot, SwTask* __restrict__ tasks)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SwTask r;
    words_box(1, rootWords, 0.0f, false, r.lo, r.hi);
    r.begin = 0;
    r.end = (int)tot->live;
    r.parentSlot = -1;
    r.arranged = 2;
    tasks[0] = r;
}

// ---- per level: before the search ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SW_BLOCK) void sw_task_begin(int T, const SwTask* __restrict__ tasks, int level, int minLeaf,
                                                          SwDecision* __restrict__ dec, SwCost* __restrict__ cost,
                                                          unsigned int* __restrict__ minSah, unsigned long long* __restrict__ minKey,
                                                          unsigned int* __restrict__ childBox)
{
    const int t = blockIdx.x * SW_BLOCK + threadIdx.x;
    if (t >= T) return;
    const SwTask tk = tasks[t];
    const int m = tk.end - tk.begin;
    // reference :155-156: small enough or too deep; the root is never a leaf
    const bool leaf = (level != 0 && m <= minLeaf) || level >= SW_MAX_DEPTH;
    dec[t] = SwDecision{leaf ? tk.arranged : SW_SEARCH, 0, 0, 0};
    const float a = box_area_valid(tk.lo, tk.hi);
    cost[t] = SwCost{a * (float)m, a * 2.0f};   // area * triCost(m), area * nodeCost(2) with Platform("GPU")
    minSah[t] = 0xFFFFFFFFu;
    minKey[t] = ~0ull;
    for (int k = 0; k < 12; k++) childBox[(size_t)t * 12 + k] = 0u;
}

// ---- per level: the sweeps -----------------------------------------------------------------------------------------------
// A position's value and flag for the forward (prefix) or backward (suffix) scan of axis d.
__device__ __forceinline__ SwSeg seg_value(int p, int P, bool backward, const int* __restrict__ ord, const int* __restrict__ taskOf,
                                           const SwDecision* __restrict__ dec, const float4* __restrict__ boxLo,
                                           const float4* __restrict__ boxHi)
{
    SwSeg v = seg_zero();
    if (p < 0 || p >= P) return v;
    const int t = taskOf[p];
    const int q = backward ? p + 1 : p - 1;
    v.flag = (q < 0 || q >= P || taskOf[q] != t) ? 1u : 0u;
    if (t >= 0 && dec[t].state == SW_SEARCH) {
        const int id = ord[p];
        box_words(boxLo[id], boxHi[id], v.w);
    }
    return v;
}

// grid (nb, 3): the workgroup's joins, forward at agg[d * nb + b], backward at agg[3 * nb + d * nb + (nb - 1 - b)]
__global__ __launch_bounds__(SW_PB) void sw_seg_local(int P, int cap, const int* __restrict__ order, const int* __restrict__ taskOf,
                                                      const SwDecision* __restrict__ dec, const float4* __restrict__ boxLo,
                                                      const float4* __restrict__ boxHi, SwSeg* __restrict__ agg)
{
    __shared__ SwSeg sh[SW_PB / 64];
    const int d = blockIdx.y, nb = gridDim.x, base = blockIdx.x * SW_PB;
    const int* ord = order + (size_t)d * cap;
    SwSeg total;
    const SwSeg mine = seg_value(base + threadIdx.x, P, false, ord, taskOf, dec, boxLo, boxHi);
    // No position of the workgroup is being searched (its tasks are leaves or done): its joins are empty.  Their flags are not needed:
    // a carry that crosses this workgroup reaches positions of the task of its last position, which is not searched either.
    if (!__syncthreads_or(mine.w[3] != 0u)) {
        if (threadIdx.x == 0) {
            agg[d * nb + blockIdx.x] = seg_zero();
            agg[3 * nb + d * nb + (nb - 1 - blockIdx.x)] = seg_zero();
        }
        return;
    }
    (void)seg_block_exclusive<SW_PB>(mine, &total, sh);
    if (threadIdx.x == 0) agg[d * nb + blockIdx.x] = total;
    (void)seg_block_exclusive<SW_PB>(seg_value(base + SW_PB - 1 - threadIdx.x, P, true, ord, taskOf, dec, boxLo, boxHi), &total, sh);
    if (threadIdx.x == 0) agg[3 * nb + d * nb + (nb - 1 - blockIdx.x)] = total;
}

// grid 2: workgroup 0 carries the forward aggregates, workgroup 1 the backward ones: in[i] -> exclusive join of in[0 .. i)
__global__ __launch_bounds__(SW_SUMS) void sw_seg_sums(int count, SwSeg* __restrict__ agg)
{
    __shared__ SwSeg sh[SW_SUMS / 64];
    SwSeg* a = agg + (size_t)blockIdx.x * count;
    SwSeg carry = seg_zero();
    for (int base = 0; base < count; base += SW_SUMS) {
        const int i = base + threadIdx.x;
        const SwSeg v = i < count ? a[i] : seg_zero();
        SwSeg chunk;
        const SwSeg ex = seg_block_exclusive<SW_SUMS>(v, &chunk, sh);
        if (i < count) a[i] = seg_join(carry, ex);
        carry = seg_join(carry, chunk);
    }
}

// grid (nb, 3): sah of the split after position p (i = p - begin + 1 references left), and the task's lowest
__global__ __launch_bounds__(SW_PB) void sw_sah(int P, int cap, const int* __restrict__ order, const int* __restrict__ taskOf,
                                                const SwTask* __restrict__ tasks, const SwDecision* __restrict__ dec,
                                                const SwCost* __restrict__ cost, const float4* __restrict__ boxLo,
                                                const float4* __restrict__ boxHi, const SwSeg* __restrict__ agg,
                                                float* __restrict__ sahOut /* [3][cap] */, unsigned int* __restrict__ minSah)
{
    __shared__ SwSeg sh[SW_PB / 64];
    __shared__ SwSeg back[SW_PB];
    const int d = blockIdx.y, nb = gridDim.x, base = blockIdx.x * SW_PB;
    const int p = base + threadIdx.x;
    const int* ord = order + (size_t)d * cap;
    SwSeg total;
    const SwSeg mine = seg_value(p, P, false, ord, taskOf, dec, boxLo, boxHi);
    if (!__syncthreads_or(mine.w[3] != 0u)) return;   // no position of the workgroup is being searched
    const SwSeg exF = seg_block_exclusive<SW_PB>(mine, &total, sh);
    const SwSeg left = seg_join(seg_join(agg[d * nb + blockIdx.x], exF), mine);                 // the first i boxes
    const SwSeg exB = seg_block_exclusive<SW_PB>(seg_value(base + SW_PB - 1 - threadIdx.x, P, true, ord, taskOf, dec, boxLo, boxHi), &total, sh);
    back[SW_PB - 1 - threadIdx.x] = seg_join(agg[3 * nb + d * nb + (nb - 1 - blockIdx.x)], exB);   // everything after that position
    __syncthreads();
    const SwSeg right = back[threadIdx.x];

    int g = -1;
    unsigned int enc = 0xFFFFFFFFu;
    if (p < P) {
        const int t = taskOf[p];
        float sah = INFINITY;
        if (t >= 0 && dec[t].state == SW_SEARCH) {
            const SwTask tk = tasks[t];
            if (p < tk.end - 1) {
                const int i = p - tk.begin + 1, m = tk.end - tk.begin;
                // reference :221-232: nodeSAH + area(left) * triCost(i) + area(right) * triCost(m - i)
                const float s = cost[t].nodeSah + words_area(left.w) * (float)i + words_area(right.w) * (float)(m - i);
                if (s <= FLT_MAX) {   // takes part (never a NaN or an infinity)
                    sah = s + 0.0f;
                    enc = ord_enc(sah);
                    g = t;
                }
            }
        }
        sahOut[(size_t)d * cap + p] = sah;
    }
    wave_grouped_atomic(g, enc, wave_min_u32, [&](int t, unsigned int v) { atomicMin(&minSah[t], v); });
}

// grid (nb, 3): the lowest (balance, axis, i) among the positions that hold the task's lowest sah
__global__ __launch_bounds__(SW_PB) void sw_pick(int P, int cap, const int* __restrict__ taskOf, const SwTask* __restrict__ tasks,
                                                 const SwDecision* __restrict__ dec, const float* __restrict__ sahIn,
                                                 const unsigned int* __restrict__ minSah, unsigned long long* __restrict__ minKey)
{
    const int d = blockIdx.y;
    const int p = blockIdx.x * SW_PB + threadIdx.x;
    int g = -1;
    unsigned long long key = ~0ull;
    if (p < P) {
        const int t = taskOf[p];
        if (t >= 0 && dec[t].state == SW_SEARCH) {
            const float sah = sahIn[(size_t)d * cap + p];
            if (sah <= FLT_MAX && ord_enc(sah) == minSah[t]) {
                const SwTask tk = tasks[t];
                const int i = p - tk.begin + 1, m = tk.end - tk.begin;
                const float fl = (float)i, fr = (float)(m - i);
                const float balance = fl * fl + fr * fr;   // positive: its bits order as the floats do
                key = ((unsigned long long)__float_as_uint(balance) << 32) | ((unsigned long long)d << 28) | (unsigned long long)i;
                g = t;
            }
        }
    }
    wave_grouped_atomic(g, key, wave_min_u64, [&](int t, unsigned long long v) { atomicMin(&minKey[t], v); });
}

// ---- per level: decisions, task scan, emit --------------------------------------------------------------------------------
__global__ __launch_bounds__(SW_BLOCK) void sw_decide_scan_local(int T, const SwTask* __restrict__ tasks, int level, int maxLeaf,
                                                                 const SwCost* __restrict__ cost, const unsigned int* __restrict__ minSah,
                                                                 const unsigned long long* __restrict__ minKey, SwDecision* __restrict__ dec,
                                                                 U4* __restrict__ local, U4* __restrict__ blockSums)
{
    const int t = blockIdx.x * SW_BLOCK + threadIdx.x;
    U4 v{0, 0, 0, 0};
    if (t < T) {
        SwDecision d = dec[t];
        const int m = tasks[t].end - tasks[t].begin;
        if (d.state == SW_SEARCH) {
            const unsigned long long key = minKey[t];
            const bool win = key != ~0ull;
            // without a winner the host's default split stands: sah FLT_MAX, axis 0, nothing left (SAHBVHBuilder.hpp Split)
            const float sah = win ? ord_dec(minSah[t]) : FLT_MAX;
            d.axis = win ? (int)((key >> 28) & 3ull) : 0;
            d.numLeft = win ? (int)(key & 0x0FFFFFFFull) : 0;
            const float leafSah = cost[t].leafSah;
            // reference :163-165
            d.state = (level != 0 && fw_min(leafSah, sah) == leafSah && m <= maxLeaf) ? 2 : SW_INNER;
            dec[t] = d;
        }
        v = d.state >= 0 ? U4{0u, 3u * (unsigned int)m + 1u, 0u, 0u} : U4{1u, 0u, 0u, 0u};
    }
    scan_local_store<SW_BLOCK>(v, t < T, t, local, blockSums, blockIdx.x);
}

// the side of every triangle of a split task (1: child 0) and the children's boxes: childBox[t][child][6]
__global__ __launch_bounds__(SW_PB) void sw_mark(int P, int cap, const int* __restrict__ order, const int* __restrict__ taskOf,
                                                 const SwTask* __restrict__ tasks, const SwDecision* __restrict__ dec,
                                                 const float4* __restrict__ boxLo, const float4* __restrict__ boxHi,
                                                 unsigned char* __restrict__ side, unsigned int* __restrict__ childBox)
{
    const int p = blockIdx.x * SW_PB + threadIdx.x;
    int g = -1;
    unsigned int w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (p < P) {
        const int t = taskOf[p];
        if (t >= 0) {
            const SwDecision d = dec[t];
            if (d.state == SW_INNER) {
                const int id = order[(size_t)d.axis * cap + p];
                const bool left = p - tasks[t].begin < d.numLeft;
                side[id] = left ? 1 : 0;
                box_words(boxLo[id], boxHi[id], w);
                g = 2 * t + (left ? 0 : 1);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
        wave_grouped_atomic(g, w[k], wave_max_u32, [&](int c, unsigned int v) { atomicMax(&childBox[(size_t)c * 6 + k], v); });
}

__device__ __forceinline__ SwTask child_task(const unsigned int* w, int begin, int end, int parentSlot, int arranged)
{
    SwTask c;
    words_box(end - begin, w, 0.0f, false, c.lo, c.hi);   // an empty child keeps AABB's initial box
    c.begin = begin;
    c.end = end;
    c.parentSlot = parentSlot;
    c.arranged = arranged;
    return c;
}

__global__ __launch_bounds__(SW_BLOCK) void sw_task_emit(int T, const SwTask* __restrict__ tasks, const SwDecision* __restrict__ dec,
                                                         const unsigned int* __restrict__ childBox, const U4* __restrict__ local,
                                                         const U4* __restrict__ blockSums, int innerBase, int rowBase, int nodeCap,
                                                         int rowCap, int* __restrict__ nodes, uint4* __restrict__ woop,
                                                         int* __restrict__ triIndex, SwTask* __restrict__ next, SwPlace* __restrict__ place,
                                                         SwTotals* __restrict__ tot)
{
    const int t = blockIdx.x * SW_BLOCK + threadIdx.x;
    if (t >= T) return;
    const U4 g = local[t] + blockSums[blockIdx.x];
    const SwDecision d = dec[t];
    const SwTask tk = tasks[t];
    const int m = tk.end - tk.begin;
    if (d.state >= 0) {
        const long long row = (long long)rowBase + g.y;
        if (row + 3ll * m >= (long long)rowCap) { atomicOr(&tot->err, 4u); place[t] = SwPlace{-1, -1, -1, 0}; return; }
        if (tk.parentSlot >= 0) nodes[tk.parentSlot] = leaf_link((int)row);
        write_leaf_terminator(woop, triIndex, row + 3 * m);
        place[t] = SwPlace{-1, (int)row, -1, 0};
        return;
    }
    const long long nodeIdx = (long long)innerBase + g.x;
    if (nodeIdx >= (long long)nodeCap) { atomicOr(&tot->err, 4u); place[t] = SwPlace{-1, -1, -1, 0}; return; }
    if (tk.parentSlot >= 0) nodes[tk.parentSlot] = inner_link((int)nodeIdx);
    const int ct = 2 * (int)g.x;
    const int mid = tk.begin + d.numLeft;
    const SwTask c0 = child_task(childBox + (size_t)t * 12, tk.begin, mid, kNodeWords * (int)nodeIdx + kLinkWord, d.axis);
    const SwTask c1 = child_task(childBox + (size_t)t * 12 + 6, mid, tk.end, kNodeWords * (int)nodeIdx + kLinkWord + 1, d.axis);
    // the split word: SplitInfo(axis, SAH, false).getBitCode(); the default split's axis 0 without a winner
    write_inner_node(nodes, nodeIdx, c0.lo, c0.hi, c1.lo, c1.hi, d.axis);
    next[ct] = c0;
    next[ct + 1] = c1;
    place[t] = SwPlace{ct, -1, (int)nodeIdx, 0};
}

// ---- per level: partition ------------------------------------------------------------------------------------------------
// grid (nb, 3)
__global__ __launch_bounds__(SW_PB) void sw_ref_scan_local(int P, int cap, const int* __restrict__ order, const int* __restrict__ taskOf,
                                                           const SwDecision* __restrict__ dec, const unsigned char* __restrict__ side,
                                                           unsigned int* __restrict__ local /* [3][cap] */,
                                                           unsigned int* __restrict__ blockSums /* [3][nb] */)
{
    const int d = blockIdx.y;
    const int p = blockIdx.x * SW_PB + threadIdx.x;
    unsigned int v = 0u;
    if (p < P) {
        const int t = taskOf[p];
        if (t >= 0 && dec[t].state == SW_INNER) v = side[order[(size_t)d * cap + p]];
    }
    scan_local_store<SW_PB>(v, p < P, (size_t)d * cap + p, local, blockSums, d * gridDim.x + blockIdx.x);
}

// grid (nb, 3): stable partition of every split task's range on every axis (the identity on the winning axis); a leaf's triangles get
// their rows, back to front of the sequence the leaf is listed by (reference :193-203)
__global__ __launch_bounds__(SW_PB) void sw_ref_scatter(int P, int cap, const int* __restrict__ order, const int* __restrict__ taskOf,
                                                        const SwTask* __restrict__ tasks, const SwDecision* __restrict__ dec,
                                                        const SwPlace* __restrict__ place, const unsigned char* __restrict__ side,
                                                        const unsigned int* __restrict__ local, const unsigned int* __restrict__ blockSums,
                                                        int* __restrict__ nextOrder, int* __restrict__ nextTaskOf, int* __restrict__ leafRow,
                                                        SwTotals* __restrict__ tot)
{
    const int d = blockIdx.y, nb = gridDim.x;
    const int p = blockIdx.x * SW_PB + threadIdx.x;
    if (p >= P) return;
    const int t = taskOf[p];
    if (t < 0) {
        if (d == 0) nextTaskOf[p] = -1;
        return;
    }
    const SwDecision dc = dec[t];
    const SwPlace pl = place[t];
    const SwTask tk = tasks[t];
    const int id = order[(size_t)d * cap + p];
    if (dc.state >= 0) {
        if (d == 0) nextTaskOf[p] = -1;
        if (d == dc.state && pl.row >= 0) leafRow[id] = pl.row + 3 * (tk.end - 1 - p);
        return;
    }
    if (pl.nodeIdx < 0) return;   // capacity error already flagged
    const int q = p - tk.begin, m = tk.end - tk.begin;
    if (d == 0) nextTaskOf[p] = pl.childTask + (q < dc.numLeft ? 0 : 1);
    const unsigned int* loc = local + (size_t)d * cap;
    const unsigned int* bs = blockSums + d * nb;
    const unsigned int rank = (loc[p] + bs[p / SW_PB]) - (loc[tk.begin] + bs[tk.begin / SW_PB]);
    int o;
    if (side[id]) {
        o = (int)rank;
        if (rank >= (unsigned int)dc.numLeft) { atomicOr(&tot->err, 2u); return; }
    } else {
        o = dc.numLeft + (q - (int)rank);
        if (o < dc.numLeft || o >= m) { atomicOr(&tot->err, 2u); return; }
    }
    nextOrder[(size_t)d * cap + tk.begin + o] = id;
}

// ---- scratch layout ------------------------------------------------------------------------------------------------------
// References never duplicate, so everything is sized by the triangle count once.  A level has at most max(n, 2) tasks: two per inner
// node of the level above, and every inner node but the root holds at least two references (more than minLeafSize).
struct SwLayout {
    size_t boxLo, boxHi, liveFlag, side, leafRow, liveIds, keys, keysTmp, hist, misc, tileState, order[2], taskOf[2], tasks[2], dec, cost, minSah,
        minKey, childBox, place, tLocal, tBlocks, sah, rLocal, rBlocks, agg, rootWords, totals, off;
    int tiles;
    explicit SwLayout(int64_t n)
    {
        ScratchCarver cv;
        const int64_t T = n + 2, nbT = T / SW_BLOCK + 2, nbN = n / SW_BLOCK + 2, nbP = n / SW_PB + 2;
        tiles = (int)((n + OS_THREADS * SW_SORT_ITEMS - 1) / (OS_THREADS * SW_SORT_ITEMS));
        boxLo = cv.take((size_t)n * 16);
        boxHi = cv.take((size_t)n * 16);
        liveFlag = cv.take((size_t)n);
        side = cv.take((size_t)n);
        leafRow = cv.take((size_t)n * 4);
        liveIds = cv.take((size_t)n * 4);
        keys = cv.take((size_t)n * 12);
        keysTmp = cv.take((size_t)n * 4);
        hist = cv.take(12 * 256 * 4);
        misc = cv.take(64);
        tileState = cv.take((size_t)tiles * 256 * 8);
        for (int k = 0; k < 2; k++) {
            order[k] = cv.take((size_t)n * 12);
            taskOf[k] = cv.take((size_t)n * 4);
            tasks[k] = cv.take((size_t)T * sizeof(SwTask));
        }
        dec = cv.take((size_t)T * sizeof(SwDecision));
        cost = cv.take((size_t)T * sizeof(SwCost));
        minSah = cv.take((size_t)T * 4);
        minKey = cv.take((size_t)T * 8);
        childBox = cv.take((size_t)T * 48);
        place = cv.take((size_t)T * sizeof(SwPlace));
        tLocal = cv.take((size_t)T * sizeof(U4));
        tBlocks = cv.take((size_t)nbT * sizeof(U4));
        sah = cv.take((size_t)n * 12);
        rLocal = cv.take((size_t)n * 12);       // also the live scan's local ranks
        rBlocks = cv.take((size_t)(3 * nbP + nbN) * 4);
        agg = cv.take((size_t)6 * nbP * sizeof(SwSeg));
        rootWords = cv.take(32);
        totals = cv.take(sizeof(SwTotals));
        off = cv.off;
    }
};

DeviceScratchPool g_swPool;

int sw_build(int n, const int32_t* d_tri, int32_t numVerts, const float* d_pos, int minLeaf, int maxLeaf, void* d_nodes, int64_t nodeCap,
             void* d_woop, int64_t rowCap, int32_t* d_idx, NtrSahDeviceResult* res, hipStream_t s)
{
    const auto wall0 = std::chrono::steady_clock::now();
    const SwLayout lay((int64_t)n);
    void* base = nullptr;
    if (const int rc = first_block(g_swPool, lay.off, &base)) return rc;
    // the layout never changes, so every pointer is resolved once
    const int cap = n;
    float4 *boxLo = at<float4>(base, lay.boxLo), *boxHi = at<float4>(base, lay.boxHi);
    unsigned char *liveFlag = at<unsigned char>(base, lay.liveFlag), *side = at<unsigned char>(base, lay.side);
    int *leafRow = at<int>(base, lay.leafRow), *liveIds = at<int>(base, lay.liveIds);
    unsigned int *keys = at<unsigned int>(base, lay.keys), *hist = at<unsigned int>(base, lay.hist), *misc = at<unsigned int>(base, lay.misc);
    unsigned int *rLocal = at<unsigned int>(base, lay.rLocal), *rBlocks = at<unsigned int>(base, lay.rBlocks);   // the live scan's too
    unsigned int *rootWords = at<unsigned int>(base, lay.rootWords), *minSah = at<unsigned int>(base, lay.minSah);
    unsigned int* childBox = at<unsigned int>(base, lay.childBox);
    unsigned long long* minKey = at<unsigned long long>(base, lay.minKey);
    SwDecision* dec = at<SwDecision>(base, lay.dec);
    SwCost* cost = at<SwCost>(base, lay.cost);
    SwPlace* place = at<SwPlace>(base, lay.place);
    U4 *tLocal = at<U4>(base, lay.tLocal), *tBlocks = at<U4>(base, lay.tBlocks);
    SwSeg* agg = at<SwSeg>(base, lay.agg);
    float* sah = at<float>(base, lay.sah);
    SwTotals* tot = at<SwTotals>(base, lay.totals);

    StreamEvents<5> ev(s);
    (void)ev.create();
    ev.mark(0);
    NTR_HIP(hipMemsetAsync(tot, 0, sizeof(SwTotals), s));
    NTR_HIP(hipMemsetAsync(rootWords, 0, 32, s));
    NTR_HIP(hipMemsetAsync(hist, 0, 12 * 256 * 4, s));
    NTR_HIP(hipMemsetAsync(misc, 0, 64, s));
    NTR_HIP(hipMemsetAsync(leafRow, 0xFF, (size_t)n * 4, s));
    const int nbN = (n + SW_BLOCK - 1) / SW_BLOCK;
    sw_prep<<<nbN, SW_BLOCK, 0, s>>>(n, d_tri, numVerts, d_pos, boxLo, boxHi, liveFlag, rootWords, tot);
    sw_live_scan_local<<<nbN, SW_BLOCK, 0, s>>>(n, liveFlag, rLocal, rBlocks);
    scan_block_sums<SW_BLOCK, unsigned int><<<1, SW_BLOCK, 0, s>>>(nbN, rBlocks, rBlocks, &tot->live);
    sw_live_scatter<<<nbN, SW_BLOCK, 0, s>>>(n, cap, liveFlag, rLocal, rBlocks, boxLo, boxHi, liveIds, keys);
    sw_root<<<1, 64, 0, s>>>(rootWords, tot, at<SwTask>(base, lay.tasks[0]));
    NTR_HIP(hipGetLastError());
    SwTotals h;
    if (const int rc = read_totals(&h, tot, s)) return rc;
    if (h.err & 1u) return set_error(NTR_ERR_INVALID, "ntr_sah_device_build: vertex index out of range");
    const int P = (int)h.live;
    if (P < 0 || P > n) return set_error(NTR_ERR_LAYOUT, "ntr_sah_device_build: internal check failed: %d live triangles of %d", P, n);
    ev.mark(1);

    // ---- the three orders: stable from ascending ids, so ties go by triangle id -------------------------------------------------
    if (P > 0) {
        const int tiles = (P + OS_THREADS * SW_SORT_ITEMS - 1) / (OS_THREADS * SW_SORT_ITEMS);
        unsigned long long* tileState = at<unsigned long long>(base, lay.tileState);
        sw_hist<<<std::min(SW_HIST_BLOCKS, (P + SW_BLOCK - 1) / SW_BLOCK), SW_BLOCK, 0, s>>>(P, cap, keys, hist, tileState, tiles * 256);
        for (int d = 0; d < 3; d++) {
            unsigned int *kA = keys + (size_t)d * cap, *kB = at<unsigned int>(base, lay.keysTmp);
            int *vA = at<int>(base, lay.order[0]) + (size_t)d * cap, *vB = at<int>(base, lay.order[1]) + (size_t)d * cap;
            for (int pass = 0; pass < 4; pass++) {
                const int gp = d * 4 + pass;   // the tile state's tags tell the twelve passes apart: it is cleared once
                const unsigned int* kIn = (pass & 1) ? kB : kA;
                unsigned int* kOut = (pass & 1) ? kA : kB;
                const int* vIn = pass == 0 ? liveIds : ((pass & 1) ? vB : vA);
                int* vOut = (pass & 1) ? vA : vB;
                onesweep_launch<SW_SORT_ITEMS, 0, false>(s, tiles, P, kIn, vIn, kOut, vOut, 1, pass * 8, gp, hist + gp * 256, tileState,
                                                         misc + gp, misc + 12);
            }
        }
        NTR_HIP(hipMemsetAsync(at<int>(base, lay.taskOf[0]), 0, (size_t)P * 4, s));
    }
    NTR_HIP(hipGetLastError());
    ev.mark(2);

    LevelState lv;
    const int nbP = (P + SW_PB - 1) / SW_PB;
    const dim3 gridP(nbP, 3);
    while (lv.T > 0) {
        const int Ti = (int)lv.T, level = lv.level;
        const int nbT = (Ti + SW_BLOCK - 1) / SW_BLOCK;
        SwTask *tasks = at<SwTask>(base, lay.tasks[lv.cur]), *next = at<SwTask>(base, lay.tasks[lv.nxt()]);
        int *order = at<int>(base, lay.order[lv.cur]), *nextOrder = at<int>(base, lay.order[lv.nxt()]);
        int *taskOf = at<int>(base, lay.taskOf[lv.cur]), *nextTaskOf = at<int>(base, lay.taskOf[lv.nxt()]);
        NTR_HIP(hipMemsetAsync(&tot->t, 0, sizeof(U4), s));
        sw_task_begin<<<nbT, SW_BLOCK, 0, s>>>(Ti, tasks, level, minLeaf, dec, cost, minSah, minKey, childBox);
        if (P > 0 && level < SW_MAX_DEPTH) {
            sw_seg_local<<<gridP, SW_PB, 0, s>>>(P, cap, order, taskOf, dec, boxLo, boxHi, agg);
            sw_seg_sums<<<2, SW_SUMS, 0, s>>>(3 * nbP, agg);
            sw_sah<<<gridP, SW_PB, 0, s>>>(P, cap, order, taskOf, tasks, dec, cost, boxLo, boxHi, agg, sah, minSah);
            sw_pick<<<gridP, SW_PB, 0, s>>>(P, cap, taskOf, tasks, dec, sah, minSah, minKey);
        }
        sw_decide_scan_local<<<nbT, SW_BLOCK, 0, s>>>(Ti, tasks, level, maxLeaf, cost, minSah, minKey, dec, tLocal, tBlocks);
        scan_block_sums<SW_BLOCK, U4><<<1, SW_BLOCK, 0, s>>>(nbT, tBlocks, tBlocks, &tot->t);
        if (P > 0) sw_mark<<<nbP, SW_PB, 0, s>>>(P, cap, order, taskOf, tasks, dec, boxLo, boxHi, side, childBox);
        sw_task_emit<<<nbT, SW_BLOCK, 0, s>>>(Ti, tasks, dec, childBox, tLocal, tBlocks, (int)lv.innerBase, (int)lv.rowBase, (int)nodeCap,
                                              (int)rowCap, (int*)d_nodes, (uint4*)d_woop, d_idx, next, place, tot);
        if (P > 0) {
            sw_ref_scan_local<<<gridP, SW_PB, 0, s>>>(P, cap, order, taskOf, dec, side, rLocal, rBlocks);
            // one scan over the three axes' sums: a rank is a difference of two entries of the same axis
            scan_block_sums<SW_SUMS, unsigned int><<<1, SW_SUMS, 0, s>>>(3 * nbP, rBlocks, rBlocks, (unsigned int*)nullptr);
            sw_ref_scatter<<<gridP, SW_PB, 0, s>>>(P, cap, order, taskOf, tasks, dec, place, side, rLocal, rBlocks, nextOrder, nextTaskOf,
                                                   leafRow, tot);
        }
        NTR_HIP(hipGetLastError());
        if (const int rc = read_totals(&h, tot, s)) return rc;
        if (const int rc = lv.check_nodes("ntr_sah_device_build", h.t.x)) return rc;
        if (h.err & 4u)
            return set_error(NTR_ERR_OVERFLOW, "ntr_sah_device_build: level %d does not fit the output buffers (%lld inner nodes, %lld rows so "
                             "far): splits without a winner chain nodes beyond ntr_lbvh_capacity()", level,
                             (long long)(lv.innerBase + h.t.x), (long long)(lv.rowBase + h.t.y));
        if (h.err)
            return set_error(NTR_ERR_LAYOUT, "ntr_sah_device_build: internal check failed: error 0x%x at level %d", h.err, level);
        lv.advance(h.t.x, h.t.y);
    }
    ev.mark(3);
    emit_leaf_rows<SW_BLOCK><<<nbN, SW_BLOCK, 0, s>>>(n, d_tri, d_pos, liveFlag, leafRow, (int)rowCap, (float4*)d_woop, d_idx, &tot->err, 2u);
    NTR_HIP(hipGetLastError());
    ev.mark(4);
    unsigned int sortErr = 0;
    NTR_HIP(hipMemcpyAsync(&sortErr, misc + 12, 4, hipMemcpyDeviceToHost, s));
    if (const int rc = read_totals(&h, tot, s)) return rc;
    if (h.err || sortErr)
        return set_error(NTR_ERR_LAYOUT, "ntr_sah_device_build: internal check failed: error 0x%x in the leaf emit, 0x%x in the sort", h.err,
                         sortErr);

    fill_bvh_result(res, lv);
    res->numDropped = n - P;
    res->prepMs = ev.ms(0, 1);
    res->sortMs = ev.ms(1, 2);
    res->levelsMs = ev.ms(2, 3);
    res->emitMs = ev.ms(3, 4);
    res->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_sah_device_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos, int32_t minLeafSize,
                         int32_t maxLeafSize, void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                         int32_t* d_triIndex, int64_t triIndexCapacity, NtrSahDeviceResult* result, void* stream)
{
    if (!result) return set_error(NTR_ERR_INVALID, "ntr_sah_device_build: null result");
    memset(result, 0, sizeof(*result));
    if (const int rc = check_build_geometry("ntr_sah_device_build", numTris, numVerts, d_triVtxIndex, d_vtxPos)) return rc;
    if (minLeafSize < 1 || maxLeafSize < minLeafSize)
        return set_error(NTR_ERR_INVALID, "ntr_sah_device_build: leaf preferences (%d, %d): 1 <= minLeafSize <= maxLeafSize", (int)minLeafSize,
                         (int)maxLeafSize);
    int64_t nodeCap, rowCap;
    if (const int rc = check_build_outputs("ntr_sah_device_build", numTris, d_nodes, nodesCapacity, d_triWoop, triWoopCapacity, d_triIndex,
                                           triIndexCapacity, &nodeCap, &rowCap))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    return finish_build(sw_build(numTris, d_triVtxIndex, numVerts, d_vtxPos, minLeafSize, maxLeafSize, d_nodes, nodeCap, d_triWoop, rowCap,
                                 d_triIndex, result, s), result, s);
}

int ntr_sah_device_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_sah_device_scratch_bytes", g_swPool, bytes); }

}  // extern "C"
