// kdtree_build_kernels.hip -- on-device kd-tree builder for gfx950: binned SAH over triangle boxes, one level per round
// (ntr_kdtree_device_build).
//
// Rebuilds the reference's persistent kd-tree builder as it is configured (CudaPersistentKDTreeBuilder.cpp, persistent_kdtree.cu
// with SPLIT_TYPE 5, PLANE_COUNT 32, TRIANGLE_CLIPPING 0, BINNING_TYPE 2) without its persistent task pool or device heap.  The
// spec is the numpy restatement tests/np_kdtree_binned.py, which states the rule and its canonical choices; the header comment of
// ntr_kdtree_device_build (include/ntrace_amd.h) lists them too.
//   once per build  kd_prep: each triangle's box, its Woop rows (woop_rows.h) into the tree's buffer, the scene box (integer
//                   atomics on the ordered encoding, -0 < +0), the root's reference list 0..n-1
//   per level       kd_count: every reference of a splitting task against the task's 32 planes; the 64 (plane, side) bits of a wave's
//                     references are reduced per task with ballots and added with one integer atomic per (task, plane, side)
//                   kd_decide: one wave per task, one lane per plane: cost, split choice (lowest cost, then lowest plane), failure
//                     test, children's leaf flags
//                   kd_task_scan_local + scan_block_sums + kd_task_emit: node numbers, leaf list offsets, child tasks and child
//                     reference offsets by an exclusive scan over the tasks; node records, parent links and leaf terminators
//                   kd_ref_scan_local + scan_block_sums + kd_ref_scatter: each task's left / right ranks of its references by a scan
//                     over the whole reference array (a task's rank is the difference to the scan at its first reference), then a
//                     stable scatter into the next level's list or the leaf list
//   end             the staged node and index arrays are copied into the tree's own buffers at their exact sizes
// Phases hand data over only at kernel boundaries.  The host reads one 32-byte record per level (the level's totals and the
// error word) to size the next level; nothing else comes back until the build ends.
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
#include <new>

#include "ntr_internal.h"
#include "level_build.h"
#include "kdtree_kernels.h"
#include "woop_rows.h"

namespace ntr {
namespace {

constexpr int KD_EMPTY = (int)0x80000000;
constexpr int KD_BLOCK = 256;

struct KdTask {         // 48 B
    float lo[3], hi[3];
    int refStart, refCount, parentSlot, fail, forced, pad;
};
struct KdDecision {     // 32 B
    float split;
    int axis, nL, nR, leaf, fail, forcedL, forcedR;
};
struct KdPlace {        // a task's global offsets after the task scan
    int childTask, childRef, leafOff, nodeIdx;
};
struct KdTotals : LevelTotals {   // t.z: next level's references, t.w: non-empty leaves of this level; err bit 2 is never set
    unsigned int pad[3];
};
struct KdParams {
    int triLimit, failureCount, maxDepth, level;
    float ci, ct, failRq, pad;
};

// ---- once per build ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KD_BLOCK) void kd_prep(int n, const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                    float4* __restrict__ boxLo, float4* __restrict__ boxHi, float4* __restrict__ woop,
                                                    int* __restrict__ refs, int* __restrict__ taskOf, unsigned int* __restrict__ sceneBox,
                                                    KdTotals* __restrict__ tot)
{
    const int i = blockIdx.x * KD_BLOCK + threadIdx.x;
    unsigned int mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    if (i < n) {
        int i0, i1, i2;
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, lo = r0, hi = r0;
        if (!tri_indices_checked(tri, numVerts, i, i0, i1, i2)) {
            atomicOr(&tot->err, 1u);
        } else {
            const float v[3][3] = {{pos[3 * i0], pos[3 * i0 + 1], pos[3 * i0 + 2]},
                                   {pos[3 * i1], pos[3 * i1 + 1], pos[3 * i1 + 2]},
                                   {pos[3 * i2], pos[3 * i2 + 1], pos[3 * i2 + 2]}};
            woop_rows_verts(v[0][0], v[0][1], v[0][2], v[1][0], v[1][1], v[1][2], v[2][0], v[2][1], v[2][2], r0, r1, r2);
            lo = make_float4(fminf(fminf(v[0][0], v[1][0]), v[2][0]), fminf(fminf(v[0][1], v[1][1]), v[2][1]),
                             fminf(fminf(v[0][2], v[1][2]), v[2][2]), 0.f);
            hi = make_float4(fmaxf(fmaxf(v[0][0], v[1][0]), v[2][0]), fmaxf(fmaxf(v[0][1], v[1][1]), v[2][1]),
                             fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]), 0.f);
            for (int j = 0; j < 3; j++)
                for (int c = 0; c < 3; c++) {
                    const unsigned int e = ord_enc(v[j][c]);
                    mn[c] = min(mn[c], e);
                    mx[c] = max(mx[c], e);
                }
        }
        boxLo[i] = lo;
        boxHi[i] = hi;
        woop[3 * (size_t)i] = r0;
        woop[3 * (size_t)i + 1] = r1;
        woop[3 * (size_t)i + 2] = r2;
        refs[i] = i;
        taskOf[i] = 0;
    }
    for (int c = 0; c < 3; c++) {
        mn[c] = wave_min_u32(mn[c]);
        mx[c] = wave_max_u32(mx[c]);
    }
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; c++) {
            atomicMin(&sceneBox[c], mn[c]);
            atomicMax(&sceneBox[3 + c], mx[c]);
        }
}

// ---- per level: count --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KD_BLOCK) void kd_count(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                     const KdTask* __restrict__ tasks, const float4* __restrict__ boxLo,
                                                     const float4* __restrict__ boxHi, unsigned int* __restrict__ bins)
{
    const int r = blockIdx.x * KD_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int t = -1;
    bool active = false;
    unsigned long long bits = 0ull;
    if (r < R) {
        t = taskOf[r];
        const KdTask& tk = tasks[t];
        active = tk.forced == 0;
        if (active) {
            const float lo[3] = {tk.lo[0], tk.lo[1], tk.lo[2]}, hi[3] = {tk.hi[0], tk.hi[1], tk.hi[2]};
            const int id = refs[r];
            const float4 bl = boxLo[id], bh = boxHi[id];
            const float tmin[3] = {bl.x, bl.y, bl.z}, tmax[3] = {bh.x, bh.y, bh.z};
#pragma unroll
            for (int k = 0; k < kPlanes; k++) {
                const int a = k / kPlanesPerAxis;
                const float p = plane_pos(lo[a], hi[a], k % kPlanesPerAxis);
                // getPlanePosition over the triangle's extent: left iff p - min > -EPS, right iff p - max < EPS
                bits |= (unsigned long long)((p - tmin[a]) > -kPlaneEps) << (2 * k);
                bits |= (unsigned long long)((p - tmax[a]) < kPlaneEps) << (2 * k + 1);
            }
        }
    }
    unsigned long long pending = __ballot(active);
    while (pending) {
        const int lead = __ffsll((long long)pending) - 1;
        const int tl = __shfl(t, lead);
        const unsigned long long seg = __ballot(active && t == tl);
        unsigned int mine = 0;
#pragma unroll 8
        for (int b = 0; b < 64; b++) {
            const unsigned int c = (unsigned int)__popcll(__ballot((bits >> b) & 1ull) & seg);
            if (lane == b) mine = c;
        }
        if (mine) atomicAdd(&bins[(size_t)tl * 64 + lane], mine);
        pending &= ~seg;
    }
}

// ---- per level: decide (one wave per task) -----------------------------------------------------------------------------
__global__ __launch_bounds__(KD_BLOCK) void kd_decide(int T, const KdTask* __restrict__ tasks, const unsigned int* __restrict__ bins,
                                                      KdDecision* __restrict__ dec, KdParams prm)
{
    const int t = blockIdx.x * (KD_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;   // wave-uniform
    const KdTask tk = tasks[t];
    if (tk.forced) {
        if (lane == 0) dec[t] = KdDecision{0.f, 0, 0, 0, 1, tk.fail, 0, 0};
        return;
    }
    const float dx = tk.hi[0] - tk.lo[0], dy = tk.hi[1] - tk.lo[1], dz = tk.hi[2] - tk.lo[2];
    unsigned long long key = ~0ull;
    float p = 0.f, s = 0.f;
    int nL = 0, nR = 0;
    if (lane < kPlanes) {
        const int a = lane / kPlanesPerAxis;
        p = plane_pos(sel3(tk.lo, a), sel3(tk.hi, a), lane - a * kPlanesPerAxis);
        float l0 = dx, l1 = dy, l2 = dz, r0 = dx, r1 = dy, r2 = dz;   // areaAABBX/Y/Z (rt_common.cu:862-905)
        if (a == 0) { l0 = p - tk.lo[0]; r0 = tk.hi[0] - p; }
        else if (a == 1) { l1 = p - tk.lo[1]; r1 = tk.hi[1] - p; }
        else { l2 = p - tk.lo[2]; r2 = tk.hi[2] - p; }
        const float aL = area3(l0, l1, l2), aR = area3(r0, r1, r2);
        nL = (int)bins[(size_t)t * 64 + 2 * lane];
        nR = (int)bins[(size_t)t * 64 + 2 * lane + 1];
        s = aL * (float)nL + aR * (float)nR;
        if (isfinite(s)) key = ((unsigned long long)__float_as_uint(s + 0.0f) << 32) | (unsigned int)lane;   // -0 -> +0
    }
    key = wave_min_u64(key);
    const int kb = (int)(key & 63ull);
    const float pb = __shfl(p, kb), sb = __shfl(s, kb);
    const int nLb = __shfl(nL, kb), nRb = __shfl(nR, kb);
    if (lane != 0) return;
    KdDecision d{0.f, 0, 0, 0, 1, tk.fail, 0, 0};
    if (key != ~0ull) {
        // taskTerminationCriteria (persistent_kdtree.cu:454-510)
        const float areaParent = area3(dx, dy, dz);
        const float leafCost = prm.ci * (float)tk.refCount;
        const float subdivisionCost = prm.ct + prm.ci * sb / areaParent;
        const float ratioWork = subdivisionCost / leafCost;
        int fail = tk.fail;
        bool leaf = false;
        if (ratioWork > prm.failRq) {
            fail++;
            if (fail > prm.failureCount) leaf = true;
        }
        const bool deep = prm.level > prm.maxDepth - 2;
        d = KdDecision{pb, kb / kPlanesPerAxis, nLb, nRb, leaf ? 1 : 0, fail, (nLb <= prm.triLimit || deep) ? 1 : 0,
                       (nRb <= prm.triLimit || deep) ? 1 : 0};
    }
    dec[t] = d;
}

// ---- per level: task scan + emit -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(KD_BLOCK) void kd_task_scan_local(int T, const KdTask* __restrict__ tasks, const KdDecision* __restrict__ dec,
                                                               U4* __restrict__ local, U4* __restrict__ blockSums)
{
    const int t = blockIdx.x * KD_BLOCK + threadIdx.x;
    U4 v{0, 0, 0, 0};
    if (t < T) {
        const KdDecision d = dec[t];
        const unsigned int n = (unsigned int)tasks[t].refCount;
        if (d.leaf) v = U4{0u, n ? n + 1u : 0u, 0u, n ? 1u : 0u};
        else v = U4{1u, 0u, (unsigned int)d.nL + (unsigned int)d.nR, 0u};
    }
    scan_local_store<KD_BLOCK>(v, t < T, t, local, blockSums, blockIdx.x);
}

__global__ __launch_bounds__(KD_BLOCK) void kd_task_emit(int T, int level, const KdTask* __restrict__ tasks,
                                                         const KdDecision* __restrict__ dec, const U4* __restrict__ local,
                                                         const U4* __restrict__ blockSums, int innerBase, int leafBase, float sceneMaxX,
                                                         int* __restrict__ nodes, int* __restrict__ triIndex, KdTask* __restrict__ next,
                                                         KdPlace* __restrict__ place)
{
    const int t = blockIdx.x * KD_BLOCK + threadIdx.x;
    if (t >= T) return;
    const U4 l = local[t], b = blockSums[blockIdx.x];
    const U4 g = l + b;
    const KdDecision d = dec[t];
    const KdTask tk = tasks[t];
    const int n = tk.refCount;
    if (d.leaf) {
        const int leafOff = leafBase + (int)g.y;
        if (level == 0) {   // DEVIATION (CudaKDTree): one inner node on axis 0 at sceneMax.x over the root leaf and an empty leaf
            nodes[0] = ~0;
            nodes[1] = KD_EMPTY;
            nodes[2] = __float_as_int(sceneMaxX);
            nodes[3] = 0;
        } else if (tk.parentSlot >= 0) {
            nodes[tk.parentSlot] = n ? ~leafOff : KD_EMPTY;
        }
        if (n) triIndex[leafOff + n] = KD_EMPTY;
        place[t] = KdPlace{-1, -1, leafOff, -1};
        return;
    }
    const int nodeIdx = innerBase + (int)g.x;
    if (tk.parentSlot >= 0) nodes[tk.parentSlot] = nodeIdx;
    nodes[4 * nodeIdx + 2] = __float_as_int(d.split);
    nodes[4 * nodeIdx + 3] = (int)((unsigned int)d.axis << 28);
    const int ct = 2 * (int)g.x, cr = (int)g.z;
    for (int side = 0; side < 2; side++) {
        KdTask c = tk;
        // taskCreateSubtask (persistent_kdtree.cu:932-980): the plane lies inside the cell, so fminf / fmaxf give the plane
        if (side == 0) {
            if (d.axis == 0) c.hi[0] = d.split; else if (d.axis == 1) c.hi[1] = d.split; else c.hi[2] = d.split;
        } else {
            if (d.axis == 0) c.lo[0] = d.split; else if (d.axis == 1) c.lo[1] = d.split; else c.lo[2] = d.split;
        }
        c.refStart = cr + (side ? d.nL : 0);
        c.refCount = side ? d.nR : d.nL;
        c.parentSlot = 4 * nodeIdx + side;
        c.fail = d.fail;
        c.forced = side ? d.forcedR : d.forcedL;
        c.pad = 0;
        next[ct + side] = c;
    }
    place[t] = KdPlace{ct, cr, -1, nodeIdx};
}

// ---- per level: reference scan + scatter ---------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ref_bits(const KdDecision& d, const float4& bl, const float4& bh)
{
    const float tmin = d.axis == 0 ? bl.x : (d.axis == 1 ? bl.y : bl.z);
    const float tmax = d.axis == 0 ? bh.x : (d.axis == 1 ? bh.y : bh.z);
    const unsigned long long l = (d.split - tmin) > -kPlaneEps ? 1ull : 0ull;
    const unsigned long long r = (d.split - tmax) < kPlaneEps ? 1ull : 0ull;
    return l | (r << 32);
}

__global__ __launch_bounds__(KD_BLOCK) void kd_ref_scan_local(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                              const KdDecision* __restrict__ dec, const float4* __restrict__ boxLo,
                                                              const float4* __restrict__ boxHi, unsigned long long* __restrict__ local,
                                                              unsigned long long* __restrict__ blockSums)
{
    const int r = blockIdx.x * KD_BLOCK + threadIdx.x;
    unsigned long long v = 0ull;
    if (r < R) {
        const KdDecision d = dec[taskOf[r]];
        if (!d.leaf) {
            const int id = refs[r];
            v = ref_bits(d, boxLo[id], boxHi[id]);
        }
    }
    scan_local_store<KD_BLOCK>(v, r < R, r, local, blockSums, blockIdx.x);
}

__global__ __launch_bounds__(KD_BLOCK) void kd_ref_scatter(int R, const int* __restrict__ refs, const int* __restrict__ taskOf,
                                                           const KdTask* __restrict__ tasks, const KdDecision* __restrict__ dec,
                                                           const KdPlace* __restrict__ place, const float4* __restrict__ boxLo,
                                                           const float4* __restrict__ boxHi, const unsigned long long* __restrict__ local,
                                                           const unsigned long long* __restrict__ blockSums, int* __restrict__ nextRefs,
                                                           int* __restrict__ nextTaskOf, int nextCap, int* __restrict__ triIndex, int idxCap,
                                                           KdTotals* __restrict__ tot)
{
    const int r = blockIdx.x * KD_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int t = taskOf[r];
    const KdDecision d = dec[t];
    const KdPlace pl = place[t];
    const int s0 = tasks[t].refStart;
    const int id = refs[r];
    if (d.leaf) {
        const int o = pl.leafOff + (r - s0);
        if (o >= 0 && o < idxCap) triIndex[o] = id;
        else atomicOr(&tot->err, 2u);
        return;
    }
    const unsigned long long g = local[r] + blockSums[r / KD_BLOCK];
    const unsigned long long b = local[s0] + blockSums[s0 / KD_BLOCK];
    const unsigned long long v = ref_bits(d, boxLo[id], boxHi[id]);
    const unsigned int pL = (unsigned int)(g - b), pR = (unsigned int)((g - b) >> 32);
    if (v & 1ull) {
        const int o = pl.childRef + (int)pL;
        if (pL < (unsigned int)d.nL && o < nextCap) { nextRefs[o] = id; nextTaskOf[o] = pl.childTask; }
        else atomicOr(&tot->err, 2u);
    }
    if (v >> 32) {
        const int o = pl.childRef + d.nL + (int)pR;
        if (pR < (unsigned int)d.nR && o < nextCap) { nextRefs[o] = id; nextTaskOf[o] = pl.childTask + 1; }
        else atomicOr(&tot->err, 2u);
    }
}

// ---- scratch layout ------------------------------------------------------------------------------------------------------
struct KdCaps {
    int64_t tasks = 0, refs = 0, nodes = 0, idx = 0;
};
struct KdLayout {
    size_t off = 0;
    size_t boxLo, boxHi, tasks[2], refs[2], taskOf[2], bins, dec, place, tLocal, tBlocks, rLocal, rBlocks, nodes, idx, sceneBox, totals;
    KdLayout(int64_t n, const KdCaps& c)
    {
        ScratchCarver cv;
        const int64_t nbT = c.tasks / KD_BLOCK + 1, nbR = c.refs / KD_BLOCK + 1;
        boxLo = cv.take((size_t)n * 16);
        boxHi = cv.take((size_t)n * 16);
        for (int k = 0; k < 2; k++) {
            tasks[k] = cv.take((size_t)c.tasks * sizeof(KdTask));
            refs[k] = cv.take((size_t)c.refs * 4);
            taskOf[k] = cv.take((size_t)c.refs * 4);
        }
        bins = cv.take((size_t)c.tasks * 64 * 4);
        dec = cv.take((size_t)c.tasks * sizeof(KdDecision));
        place = cv.take((size_t)c.tasks * sizeof(KdPlace));
        tLocal = cv.take((size_t)c.tasks * sizeof(U4));
        tBlocks = cv.take((size_t)nbT * sizeof(U4));
        rLocal = cv.take((size_t)c.refs * 8);
        rBlocks = cv.take((size_t)(nbR + 1) * 8);   // + the grand total
        nodes = cv.take((size_t)c.nodes * 16);
        idx = cv.take((size_t)c.idx * 4);
        sceneBox = cv.take(6 * 4);
        totals = cv.take(sizeof(KdTotals));
        off = cv.off;
    }
};

DeviceScratchPool g_kdPool;

// Capacities stay within what the kernels index with int: references and leaf index entries below 2^31, node ints (4 per node) too.
constexpr int64_t KD_MAX_ENTRIES = INT_MAX;
constexpr int64_t KD_MAX_NODES = INT_MAX / 4;
int64_t grown(int64_t need, int64_t have, int64_t limit)
{
    return need <= have ? have : std::min(limit, std::max(need, have + have / 2));
}

}  // namespace
}  // namespace ntr

using namespace ntr;

struct NtrDeviceKdtree {
    void* nodes = nullptr;
    void* woop = nullptr;
    int32_t* idx = nullptr;
    NtrDeviceKdtreeInfo info;
};

namespace {

void free_tree(NtrDeviceKdtree* t)
{
    if (!t) return;
    if (t->nodes) (void)hipFree(t->nodes);
    if (t->woop) (void)hipFree(t->woop);
    if (t->idx) (void)hipFree(t->idx);
    delete t;
}

// The build proper: fills *t (whose buffers the caller frees on failure).
int kd_build(NtrDeviceKdtree* t, int n, const int32_t* d_tri, int32_t numVerts, const float* d_pos, const NtrKdtreeDeviceParams& prm,
             int maxDepth, hipStream_t s)
{
    const auto wall0 = std::chrono::steady_clock::now();
    NtrDeviceKdtreeInfo& info = t->info;
    info.triWoopBytes = ((int64_t)n * 48 + 4095) & ~(int64_t)4095;
    {
        const int rc = device_malloc(&t->woop, (size_t)info.triWoopBytes, "ntr_kdtree_device_build: triWoop");
        if (rc != NTR_OK) return rc;
    }
    NTR_HIP(hipMemsetAsync(t->woop, 0, (size_t)info.triWoopBytes, s));

    KdCaps caps;
    caps.tasks = std::max<int64_t>(1024, n / 2);
    caps.refs = 3 * (int64_t)n;
    caps.nodes = std::max<int64_t>(1024, n);
    caps.idx = 3 * (int64_t)n + 1024;
    // a pool left large by an earlier build: take as much of it as fits, so that fewer levels need a relayout
    for (const size_t held = g_kdPool.held();;) {
        KdCaps c2 = caps;
        c2.tasks *= 2; c2.refs *= 2; c2.nodes *= 2; c2.idx *= 2;
        if (c2.tasks > KD_MAX_ENTRIES || c2.refs > KD_MAX_ENTRIES || c2.nodes > KD_MAX_NODES || c2.idx > KD_MAX_ENTRIES) break;
        if (KdLayout((int64_t)n, c2).off > held) break;
        caps = c2;
    }
    KdLayout lay((int64_t)n, caps);
    void* base = nullptr;
    if (const int rc = first_block(g_kdPool, lay.off, &base)) return rc;
    StreamEvents<4> ev(s);
    (void)ev.create();
    ev.mark(0);
    NTR_HIP(hipMemsetAsync(at<KdTotals>(base, lay.totals), 0, sizeof(KdTotals), s));
    const unsigned int boxInit[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    NTR_HIP(hipMemcpyAsync(at<unsigned int>(base, lay.sceneBox), boxInit, sizeof(boxInit), hipMemcpyHostToDevice, s));
    kd_prep<<<(n + KD_BLOCK - 1) / KD_BLOCK, KD_BLOCK, 0, s>>>(n, d_tri, numVerts, d_pos, at<float4>(base, lay.boxLo), at<float4>(base, lay.boxHi),
                                                               (float4*)t->woop, at<int>(base, lay.refs[0]), at<int>(base, lay.taskOf[0]),
                                                               at<unsigned int>(base, lay.sceneBox), at<KdTotals>(base, lay.totals));
    NTR_HIP(hipGetLastError());
    unsigned int box[6];
    KdTotals tot;
    NTR_HIP(hipMemcpyAsync(box, at<unsigned int>(base, lay.sceneBox), sizeof(box), hipMemcpyDeviceToHost, s));
    if (const int rc = read_totals(&tot, at<KdTotals>(base, lay.totals), s)) return rc;
    if (tot.err & 1u) return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: vertex index out of range");
    for (int k = 0; k < 3; k++) {
        info.sceneMin[k] = ord_dec(box[k]);
        info.sceneMax[k] = ord_dec(box[3 + k]);
    }
    {
        KdTask root;
        memset(&root, 0, sizeof(root));
        for (int k = 0; k < 3; k++) { root.lo[k] = info.sceneMin[k]; root.hi[k] = info.sceneMax[k]; }
        root.refStart = 0;
        root.refCount = n;
        root.parentSlot = -1;
        root.forced = n <= prm.triLimit ? 1 : 0;
        NTR_HIP(hipMemcpyAsync(at<KdTask>(base, lay.tasks[0]), &root, sizeof(root), hipMemcpyHostToDevice, s));
        NTR_HIP(hipStreamSynchronize(s));   // `root` leaves scope
    }
    ev.mark(1);

    LevelState lv;   // rowBase: the leaf index entries so far
    int64_t R = n;
    bool rootLeaf = false;
    while (lv.T > 0) {
        const int64_t T = lv.T, innerBase = lv.innerBase, leafBase = lv.rowBase;
        const int level = lv.level;
        if (2 * R > KD_MAX_ENTRIES || 2 * T > KD_MAX_ENTRIES || innerBase + T > KD_MAX_NODES || leafBase + R + T > KD_MAX_ENTRIES)
            return set_error(NTR_ERR_NOMEM, "ntr_kdtree_device_build: level %d (%lld tasks, %lld references) exceeds the builder's int32 "
                             "indexing", level, (long long)T, (long long)R);
        // capacity for this level and the next (at most two children per task, two references per reference)
        KdCaps need;
        need.tasks = 2 * T;
        need.refs = 2 * R;
        need.nodes = innerBase + T;
        need.idx = leafBase + R + T;
        if (need.tasks > caps.tasks || need.refs > caps.refs || need.nodes > caps.nodes || need.idx > caps.idx) {
            KdCaps nc;
            nc.tasks = grown(need.tasks, caps.tasks, KD_MAX_ENTRIES);
            nc.refs = grown(need.refs, caps.refs, KD_MAX_ENTRIES);
            nc.nodes = grown(need.nodes, caps.nodes, KD_MAX_NODES);
            nc.idx = grown(need.idx, caps.idx, KD_MAX_ENTRIES);
            const KdLayout nl((int64_t)n, nc);
            const KdLayout ol = lay;
            const int c0 = lv.cur;
            const int rc = g_kdPool.regrow(nl.off, &base, [&](void* from, void* to) {
                auto cp = [&](size_t dst, size_t src, size_t bytes) {
                    return bytes ? hipMemcpyAsync((char*)to + dst, (char*)from + src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
                };
                hipError_t e = cp(nl.boxLo, ol.boxLo, (size_t)n * 16);
                if (e == hipSuccess) e = cp(nl.boxHi, ol.boxHi, (size_t)n * 16);
                if (e == hipSuccess) e = cp(nl.tasks[c0], ol.tasks[c0], (size_t)T * sizeof(KdTask));
                if (e == hipSuccess) e = cp(nl.refs[c0], ol.refs[c0], (size_t)R * 4);
                if (e == hipSuccess) e = cp(nl.taskOf[c0], ol.taskOf[c0], (size_t)R * 4);
                if (e == hipSuccess) e = cp(nl.nodes, ol.nodes, (size_t)innerBase * 16);
                if (e == hipSuccess) e = cp(nl.idx, ol.idx, (size_t)leafBase * 4);
                if (e == hipSuccess) e = cp(nl.totals, ol.totals, sizeof(KdTotals));
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                return e == hipSuccess ? (int)NTR_OK : hip_fail(e, "kd-tree scratch move");
            }, /*relayout=*/true);
            if (rc != NTR_OK) return rc;
            caps = nc;
            lay = nl;
        }
        const int Ti = (int)T, Ri = (int)R;
        const int nbT = (Ti + KD_BLOCK - 1) / KD_BLOCK, nbR = (Ri + KD_BLOCK - 1) / KD_BLOCK;
        KdParams kp{prm.triLimit, prm.failureCount, maxDepth, level, prm.ci, prm.ct, prm.failRq, 0.f};
        // resolved per level: a relayout moves the block and every array in it
        KdTask *tasks = at<KdTask>(base, lay.tasks[lv.cur]), *next = at<KdTask>(base, lay.tasks[lv.nxt()]);
        int *refs = at<int>(base, lay.refs[lv.cur]), *nextRefs = at<int>(base, lay.refs[lv.nxt()]);
        int *taskOf = at<int>(base, lay.taskOf[lv.cur]), *nextTaskOf = at<int>(base, lay.taskOf[lv.nxt()]);
        float4 *boxLo = at<float4>(base, lay.boxLo), *boxHi = at<float4>(base, lay.boxHi);
        unsigned int* bins = at<unsigned int>(base, lay.bins);
        KdDecision* dec = at<KdDecision>(base, lay.dec);
        KdPlace* place = at<KdPlace>(base, lay.place);
        U4 *tLocal = at<U4>(base, lay.tLocal), *tBlocks = at<U4>(base, lay.tBlocks);
        unsigned long long *rLocal = at<unsigned long long>(base, lay.rLocal), *rBlocks = at<unsigned long long>(base, lay.rBlocks);
        int *nodes = at<int>(base, lay.nodes), *idx = at<int>(base, lay.idx);
        KdTotals* dtot = at<KdTotals>(base, lay.totals);
        NTR_HIP(hipMemsetAsync(bins, 0, (size_t)T * 64 * 4, s));
        if (Ri > 0) kd_count<<<nbR, KD_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, boxLo, boxHi, bins);
        kd_decide<<<(Ti + 3) / 4, KD_BLOCK, 0, s>>>(Ti, tasks, bins, dec, kp);
        kd_task_scan_local<<<nbT, KD_BLOCK, 0, s>>>(Ti, tasks, dec, tLocal, tBlocks);
        scan_block_sums<KD_BLOCK, U4><<<1, KD_BLOCK, 0, s>>>(nbT, tBlocks, tBlocks, &dtot->t);
        kd_task_emit<<<nbT, KD_BLOCK, 0, s>>>(Ti, level, tasks, dec, tLocal, tBlocks, (int)innerBase, (int)leafBase, info.sceneMax[0], nodes, idx,
                                              next, place);
        if (Ri > 0) {
            kd_ref_scan_local<<<nbR, KD_BLOCK, 0, s>>>(Ri, refs, taskOf, dec, boxLo, boxHi, rLocal, rBlocks);
            scan_block_sums<KD_BLOCK, unsigned long long><<<1, KD_BLOCK, 0, s>>>(nbR, rBlocks, rBlocks, rBlocks + nbR);
            kd_ref_scatter<<<nbR, KD_BLOCK, 0, s>>>(Ri, refs, taskOf, tasks, dec, place, boxLo, boxHi, rLocal, rBlocks, nextRefs, nextTaskOf,
                                                    (int)caps.refs, idx, (int)caps.idx, dtot);
        }
        NTR_HIP(hipGetLastError());
        if (const int rc = read_totals(&tot, dtot, s)) return rc;
        if (tot.err) return set_error(NTR_ERR_LAYOUT, "ntr_kdtree_device_build: internal check failed: partition error 0x%x at level %d", tot.err, level);
        const int64_t inner = tot.t.x, nonEmpty = tot.t.w;
        info.numEmptyLeaves += (int32_t)(T - inner - nonEmpty);
        info.numTriRefs += (int32_t)(tot.t.y - nonEmpty);
        if (level == 0 && inner == 0) rootLeaf = true;
        lv.advance(inner, tot.t.y);
        R = tot.t.z;
    }
    info.numLevels = lv.level;
    info.numLeafNodes = lv.numLeaves;
    info.maxDepth = lv.maxDepth;
    if (rootLeaf) {
        lv.innerBase = 1;
        info.numLeafNodes = 2;
        info.numEmptyLeaves = 1;
        info.maxDepth = 1;
    }
    info.numInnerNodes = (int32_t)lv.innerBase;
    ev.mark(2);

    info.nodesBytes = lv.innerBase * 16;
    info.triIndexBytes = lv.rowBase * 4;
    {
        int rc = device_malloc(&t->nodes, (size_t)info.nodesBytes, "ntr_kdtree_device_build: nodes");
        if (rc == NTR_OK) rc = device_malloc((void**)&t->idx, (size_t)info.triIndexBytes, "ntr_kdtree_device_build: triIndex");
        if (rc != NTR_OK) return rc;
    }
    NTR_HIP(hipMemcpyAsync(t->nodes, at<char>(base, lay.nodes), (size_t)info.nodesBytes, hipMemcpyDeviceToDevice, s));
    NTR_HIP(hipMemcpyAsync(t->idx, at<char>(base, lay.idx), (size_t)info.triIndexBytes, hipMemcpyDeviceToDevice, s));
    ev.mark(3);
    NTR_HIP(hipStreamSynchronize(s));

    info.nodes = t->nodes;
    info.triWoop = t->woop;
    info.triIndex = t->idx;
    const float sx = info.sceneMax[0] + info.sceneMin[0], sy = info.sceneMax[1] + info.sceneMin[1], sz = info.sceneMax[2] + info.sceneMin[2];
    info.delta = ::sqrtf(sx * sx + sy * sy + sz * sz) * 0.000001f;   // CudaKDTreeTracer.cpp:97
    info.percentDuplicates = (float)(info.numTriRefs - n) / (float)n * 100.0f;
    info.prepMs = ev.ms(0, 1);
    info.levelsMs = ev.ms(1, 2);
    info.emitMs = ev.ms(2, 3);
    info.seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace

extern "C" {

int ntr_kdtree_device_params_default(NtrKdtreeDeviceParams* p)
{
    if (!p) return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_params_default: null");
    memset(p, 0, sizeof(*p));
    p->triLimit = 16;      // config.conf, block PersistentKDTree
    p->triMaxLimit = 16;
    p->failureCount = 0;
    p->depthK1 = 1.2f;
    p->depthK2 = 2.0f;
    p->ci = 1.0f;
    p->ct = 1.0f;
    p->failRq = 0.9f;
    return NTR_OK;
}

int ntr_kdtree_device_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                            const NtrKdtreeDeviceParams* params, NtrDeviceKdtree** out, void* stream)
{
    if (!out) return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: null out");
    *out = nullptr;
    if (numTris < 1 || numTris > (1 << 28) || numVerts < 1 || !d_triVtxIndex || !d_vtxPos)
        return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: bad geometry arguments (1 <= numTris <= 2^28, numVerts >= 1, non-null buffers)");
    NtrKdtreeDeviceParams p;
    ntr_kdtree_device_params_default(&p);
    if (params) p = *params;
    if (p.triLimit < 1 || p.triMaxLimit < 0 || p.failureCount < 0)
        return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: triLimit < 1, triMaxLimit < 0 or failureCount < 0");
    if (!std::isfinite(p.depthK1) || !std::isfinite(p.depthK2) || !std::isfinite(p.ci) || !std::isfinite(p.ct) || !std::isfinite(p.failRq))
        return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: depthK1, depthK2, ci, ct and failRq must be finite");
    // CudaPersistentKDTreeBuilder.cpp:451
    const float depth = p.depthK1 * std::log2((float)numTris) + p.depthK2;
    if (!std::isfinite(depth) || depth >= (float)(NTR_KDTREE_STACK_DEPTH + 1) || depth <= -1e9f)
        return set_error(NTR_ERR_INVALID, "ntr_kdtree_device_build: maxDepth = int(depthK1 * log2(numTris) + depthK2) = %g is above %d, the trace kernel's stack",
                         (double)depth, NTR_KDTREE_STACK_DEPTH);
    const int maxDepth = (int)depth;
    NtrDeviceKdtree* t = new (std::nothrow) NtrDeviceKdtree();
    if (!t) return set_error(NTR_ERR_NOMEM, "ntr_kdtree_device_build: out of host memory");
    memset(&t->info, 0, sizeof(t->info));
    const int rc = kd_build(t, numTris, d_triVtxIndex, numVerts, d_vtxPos, p, maxDepth, (hipStream_t)stream);
    if (rc != NTR_OK) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        free_tree(t);
        return rc;
    }
    *out = t;
    return NTR_OK;
}

int ntr_device_kdtree_info(const NtrDeviceKdtree* t, NtrDeviceKdtreeInfo* info)
{
    if (!t || !info) return set_error(NTR_ERR_INVALID, "ntr_device_kdtree_info: null argument");
    *info = t->info;
    return NTR_OK;
}

void ntr_device_kdtree_free(NtrDeviceKdtree* t) { free_tree(t); }

int ntr_kdtree_device_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_kdtree_device_scratch_bytes", g_kdPool, bytes); }

int ntr_device_kdtree_download(const NtrDeviceKdtree* t, void* nodes, void* triWoop, int32_t* triIndex)
{
    if (!t) return set_error(NTR_ERR_INVALID, "ntr_device_kdtree_download: null tree");
    if (nodes && t->info.nodesBytes) NTR_HIP(hipMemcpy(nodes, t->nodes, (size_t)t->info.nodesBytes, hipMemcpyDeviceToHost));
    if (triWoop && t->info.triWoopBytes) NTR_HIP(hipMemcpy(triWoop, t->woop, (size_t)t->info.triWoopBytes, hipMemcpyDeviceToHost));
    if (triIndex && t->info.triIndexBytes) NTR_HIP(hipMemcpy(triIndex, t->idx, (size_t)t->info.triIndexBytes, hipMemcpyDeviceToHost));
    return NTR_OK;
}

}  // extern "C"
