// hlbvh_kernels.hip -- on-device HLBVH builder for gfx950: binned SAH over Morton clusters (ntr_hlbvh_build).
//
// Rebuilds HLBVHBuilder::buildHLBVH (src/rt/bvh/HLBVH/HLBVHBuilder.cpp:595-750); the spec is the numpy restatement tests/np_hlbvh.py,
// which lists the canonical choices (bin conversion, split-missed fallback and its box, fewer than two clusters).
//   calcMorton + radixSortCuda   -> lbvh_sort_codes (lbvh_kernels.hip): the LBVH's own codes and stable sort, same launches
//   createClusters (radixSort.cu:48-115), clusterAABB (emitTreeKernel.cu:1090-)
//                                -> hl_head_count / scan_block_sums / hl_head_emit: boundary flags on code >> 3*bits, a scan, cluster
//                                   starts; hl_cluster_box: segmented min / max, 16 positions per thread, wave-level combine of the
//                                   partial segments and integer atomics on the ord_enc_int encoding only where a cluster crosses a chunk
//   buildTopLevel (HLBVHBuilder.cpp:156-317; fillBins / findSplit / distribute, emitTreeKernel.cu:713-1027)
//                                -> per level: hl_fill_bins (integer atomics on the ord_enc encoding, LDS bins when a workgroup's clusters
//                                   share one task), hl_find_split (one thread per task), hl_left_count + scan_block_sums +
//                                   hl_partition (a stable partition by scan keeps every task's clusters contiguous and in Morton
//                                   order, so the object split is "the first cntL of the range"; single clusters become leaves or
//                                   bottom-level roots here), hl_level_end.  Levels are launched in chunks of HL_CHUNK with device-side
//                                   task counts; the host reads one word per chunk, and the number of levels is bounded by the
//                                   number of clusters (every level splits each task into two non-empty parts).  No grid barrier.
//   buildBottomLevel (:319-406)  -> hl_bottom_emit: the reference emit (emitTreeKernel.cu:233-381) one level per launch, starting at
//                                   level 3 * bits - 1 at every bottom-level root (not 29 - depth); node / leaf slots by atomics.
//   calcAABB (:408-449)          -> hl_refit: one launch per creation batch, deepest first (a node's children are always created in
//                                   a later batch), leaf boxes with epsilon and unions of child boxes -- the LBVH's expressions.
// Node numbering and leaf placement follow atomic order as in the reference; the tree is compared in canonical form.
//
// CAPACITY: the outputs fit ntr_lbvh_capacity(numTris).  Every child in the tree is non-empty: a top-level child holds at least one
// cluster and a cluster at least one triangle; a bottom-level node holds more than leafSize >= 1 triangles, and its split (the first
// position where the bit flips, or the median (s + e) >> 1 of at least two) leaves both sides non-empty.  So there are at most numTris
// leaves and, each inner node having two children, at most numTris - 1 inner nodes (< numTris + 2 slots of 64 B); the Woop / index
// buffers take 3 * numTris + leaves <= 4 * numTris entries.  The kernels still check every slot against the capacity they were given.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ntr_internal.h"
#include "compact_bvh.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "woop_rows.h"

namespace ntr {

constexpr int HL_BINS = 8;
constexpr int HL_BIN_WORDS = 3 * HL_BINS * 8;   // per task: [axis][bin][lo.xyz hi.xyz count pad]
constexpr int HL_CHUNK = 8;                     // top levels launched between two read-backs

struct HlState {
    unsigned int nodeCount;           // next free node index (the root is 0)
    unsigned int overflow;            // 1: node slots, 2: Woop / index slots
    unsigned long long leafPtr;       // (triangles << 32) | leaves, like g_leafsPtr
    unsigned int numClusters;
    unsigned int topLevels;
    unsigned int bottomCount[32];     // bottom-level queue length per level
};

struct HlCls {           // clusters, in the current partitioned order
    int* start; int* end;
    int* box;            // 6 per cluster: ord_enc_int(lo.xyz), ord_enc_int(hi.xyz)
    int* task;           // task of the current level, -1: done
};
struct HlTasks {
    int* beg; int* end;  // cluster positions [beg, end)
    float* box;          // 6 per task: lo.xyz hi.xyz
    int* node;
};
struct HlDec { int axis, obj, split, cntL, cntR, left, right, pad; };

struct HlOut {
    int* nodes; unsigned int nodeCap;
    float4* woop; int* idx; long long entryCap;     // float4 / int entries of the Woop and index buffers
    const int* tri; const float* pos; const int* triSorted;
    int leafSize; float eps;
};

// bin words: ~ord_enc(lo) and ord_enc(hi) (through the signed form), so that zero is the identity of both (atomicMax on unsigned) and
// one memset clears them

// clamp((int)floorf(q), 0, 7) with cvt.rzi.s32.f32 semantics: NaN -> 0, +inf -> 7, -inf -> 0 (a plain cast of NaN is undefined)
__device__ __forceinline__ int bin_of(float q)
{
    const float f = floorf(q);
    if (!(f >= 0.0f)) return 0;
    if (f >= (float)(HL_BINS - 1)) return HL_BINS - 1;
    return (int)f;
}

// ---- leaves and nodes ----------------------------------------------------------------------------
__device__ int hl_alloc_node(HlState* st, unsigned int cap)
{
    const unsigned int i = atomicAdd(&st->nodeCount, 1u);
    if (i >= cap) { atomicOr(&st->overflow, 1u); return -1; }
    return (int)i;
}

// createLeaf (emitTreeKernel.cu:170-231), COMPACT_LAYOUT + WOOP_TRIANGLES: returns ~(first float4 entry)
__device__ int hl_leaf(const HlOut& o, HlState* st, int s, int e)
{
    const int cnt = e - s;
    const unsigned long long old = atomicAdd(&st->leafPtr, ((unsigned long long)cnt << 32) | 1ull);
    const long long out = (long long)(old >> 32) * 3 + (long long)(old & 0xFFFFFFFFull);
    if (out + 3ll * cnt + 1 > o.entryCap) { atomicOr(&st->overflow, 2u); return ~0; }
    for (int i = 0; i < cnt; i++) {
        const int t = o.triSorted[s + i];
        float4 r0, r1, r2;
        woop_rows(o.tri, o.pos, t, r0, r1, r2);
        o.woop[out + 3 * i] = r0; o.woop[out + 3 * i + 1] = r1; o.woop[out + 3 * i + 2] = r2;
        o.idx[out + 3 * i] = t; o.idx[out + 3 * i + 1] = 0; o.idx[out + 3 * i + 2] = 0;
    }
    const float term = __int_as_float((int)0x80000000);
    o.woop[out + 3 * cnt] = make_float4(term, term, term, term);
    o.idx[out + 3 * cnt] = 0;
    return (int)~out;
}

// ---- clusters ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const unsigned int* keys, int i, int bits)
{
    return i == 0 || bits == 0 || (keys[i] >> (3 * bits)) != (keys[i - 1] >> (3 * bits));
}

// 1024 positions per workgroup (256 threads x 4): number of cluster heads
__global__ __launch_bounds__(256) void hl_head_count(int n, int bits, const unsigned int* __restrict__ keys, int* __restrict__ blockCnt)
{
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    int v = 0;
    for (int k = 0; k < 4; k++) v += (base + k < n && is_head(keys, base + k, bits)) ? 1 : 0;
    int total;
    block_exclusive_scan<256>(v, &total);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = total;
}

// cluster starts (clsStart[C] = n) and every position's cluster
__global__ __launch_bounds__(256) void hl_head_emit(int n, int bits, const unsigned int* __restrict__ keys, const int* __restrict__ blockExcl,
                                                    int* __restrict__ clsStart, int* __restrict__ clsOf)
{
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    int f[4], v = 0;
    for (int k = 0; k < 4; k++) { f[k] = (base + k < n && is_head(keys, base + k, bits)) ? 1 : 0; v += f[k]; }
    int total;
    int r = blockExcl[blockIdx.x] + block_exclusive_scan<256>(v, &total);
    for (int k = 0; k < 4; k++) {
        const int i = base + k;
        if (i >= n) break;
        if (f[k]) clsStart[r] = i;
        r += f[k];
        clsOf[i] = r - 1;
        if (i == n - 1) clsStart[r] = n;
    }
}

__global__ void hl_cluster_init(int C, const int* __restrict__ clsStart, HlCls c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    c.start[i] = clsStart[i];
    c.end[i] = clsStart[i + 1];
    c.task[i] = 0;
    for (int k = 0; k < 3; k++) { c.box[6 * i + k] = ord_enc_int(FLT_MAX); c.box[6 * i + 3 + k] = ord_enc_int(-FLT_MAX); }
}

__device__ __forceinline__ void tri_raw_box(const int* tri, const float* pos, int t, int lo[3], int hi[3])
{
    const int v[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    for (int k = 0; k < 3; k++) {
        const int a = ord_enc_int(pos[3 * v[0] + k]), b = ord_enc_int(pos[3 * v[1] + k]), c = ord_enc_int(pos[3 * v[2] + k]);
        lo[k] = min(a, min(b, c));
        hi[k] = max(a, max(b, c));
    }
}

__device__ __forceinline__ void box_atomic(int* box, const int lo[3], const int hi[3])
{
    for (int k = 0; k < 3; k++) { atomicMin(&box[k], lo[k]); atomicMax(&box[3 + k], hi[k]); }
}

// Raw vertex box per cluster (emitTreeKernel.cu:1090-, no epsilon) in the ord_enc_int order.  A thread folds 16 consecutive positions: segments
// that start and end inside its chunk are stored, its first segment (when it is not also the last) goes out by atomics, and the last
// segments of a wave's lanes are combined by cluster across the wave first, so a cluster of millions of triangles costs one set of
// atomics per 1024 triangles, not per triangle.
constexpr int HL_BOX_CHUNK = 16;
__global__ __launch_bounds__(256) void hl_cluster_box(int n, const int* __restrict__ tri, const float* __restrict__ pos,
                                                      const int* __restrict__ triSorted, const int* __restrict__ clsOf,
                                                      const int* __restrict__ clsStart, int* __restrict__ box)
{
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * HL_BOX_CHUNK;
    int key = -1;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    if (p0 < n) {
        const int p1 = min(p0 + HL_BOX_CHUNK, n);
        int cur = clsOf[p0];
        bool first = true;
        for (int p = p0; p < p1; p++) {
            const int c = clsOf[p];
            if (c != cur) {
                if (first && clsStart[cur] < p0) box_atomic(box + 6 * cur, lo, hi);
                else for (int k = 0; k < 3; k++) { box[6 * cur + k] = lo[k]; box[6 * cur + 3 + k] = hi[k]; }
                first = false;
                cur = c;
                for (int k = 0; k < 3; k++) { lo[k] = INT_MAX; hi[k] = INT_MIN; }
            }
            int tl[3], th[3];
            tri_raw_box(tri, pos, triSorted[p], tl, th);
            for (int k = 0; k < 3; k++) { lo[k] = min(lo[k], tl[k]); hi[k] = max(hi[k], th[k]); }
        }
        key = cur;
    }
    // wave-level combine of the lanes' last segments (cluster ids are non-decreasing along the lanes)
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const int ok = __shfl_down(key, off, 64);
        int o[6];
        for (int k = 0; k < 3; k++) { o[k] = __shfl_down(lo[k], off, 64); o[3 + k] = __shfl_down(hi[k], off, 64); }
        if (lane + off < 64 && ok == key) for (int k = 0; k < 3; k++) { lo[k] = min(lo[k], o[k]); hi[k] = max(hi[k], o[3 + k]); }
    }
    const int prev = __shfl_up(key, 1, 64);
    if (key >= 0 && (lane == 0 || prev != key)) box_atomic(box + 6 * key, lo, hi);
}

// ---- top level: one level ------------------------------------------------------------------------------
// fillBins (emitTreeKernel.cu:713-777): per cluster its bin on each axis, bin boxes / counts by integer atomics
__global__ __launch_bounds__(256) void hl_fill_bins(int C, HlCls c, HlTasks tk, unsigned int* __restrict__ bins, uchar4* __restrict__ cBin)
{
    __shared__ unsigned int s_bins[HL_BIN_WORDS];
    __shared__ int s_task;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int task = i < C ? c.task[i] : -1;
    if (threadIdx.x == 0) s_task = INT_MAX;
    for (int w = threadIdx.x; w < HL_BIN_WORDS; w += 256) s_bins[w] = 0;
    __syncthreads();
    if (task >= 0) atomicMin(&s_task, task);
    __syncthreads();
    const int t0 = s_task;
    const bool uniform = __syncthreads_and(task < 0 || task == t0) != 0;
    if (task >= 0) {
        float lo[3], hi[3];
        for (int k = 0; k < 3; k++) { lo[k] = ord_dec_int(c.box[6 * i + k]); hi[k] = ord_dec_int(c.box[6 * i + 3 + k]); }
        const float* tb = tk.box + 6 * task;
        int b[3];
        for (int a = 0; a < 3; a++) {
            const float mid = lo[a] + (hi[a] - lo[a]) / 2.0f;
            const float step = (tb[3 + a] - tb[a]) / (float)HL_BINS;
            b[a] = bin_of((mid - tb[a]) / step);
        }
        cBin[i] = make_uchar4((unsigned char)b[0], (unsigned char)b[1], (unsigned char)b[2], 0);
        unsigned int* dst = uniform ? s_bins : bins + (size_t)task * HL_BIN_WORDS;
        for (int a = 0; a < 3; a++) {
            unsigned int* w = dst + (a * HL_BINS + b[a]) * 8;
            for (int k = 0; k < 3; k++) {
                atomicMax(&w[k], ~ord_from_int(ord_enc_int(lo[k])));
                atomicMax(&w[3 + k], ord_from_int(ord_enc_int(hi[k])));
            }
            atomicAdd(&w[6], 1u);
        }
    }
    if (uniform && t0 != INT_MAX) {
        __syncthreads();
        unsigned int* g = bins + (size_t)t0 * HL_BIN_WORDS;
        for (int w = threadIdx.x; w < HL_BIN_WORDS; w += 256) {
            const unsigned int v = s_bins[w];
            if (!v) continue;
            if ((w & 7) == 6) atomicAdd(&g[w], v); else atomicMax(&g[w], v);
        }
    }
}

// findSplit (emitTreeKernel.cu:779-938), one thread per task; the sweeps run on the ord_enc_int encoding (min / max there are fminf / fmaxf)
__global__ __launch_bounds__(256) void hl_find_split(const unsigned int* __restrict__ taskCount, unsigned int* __restrict__ nextCount,
                                                     HlTasks tin, HlTasks tout, unsigned int* __restrict__ bins, HlDec* __restrict__ dec,
                                                     HlOut o, HlState* st)
{
    const int nt = (int)*taskCount;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
        unsigned int* bw = bins + (size_t)t * HL_BIN_WORDS;
        float best = FLT_MAX;
        int axis = 0, split = -1, cntL = 0, cntR = 0;
        float bl[6], br[6];
        for (int a = 0; a < 3; a++) {
            int blo[HL_BINS][3], bhi[HL_BINS][3], bc[HL_BINS];
            for (int b = 0; b < HL_BINS; b++) {
                const unsigned int* w = bw + (a * HL_BINS + b) * 8;
                bc[b] = (int)w[6];
                for (int k = 0; k < 3; k++) {
                    blo[b][k] = bc[b] ? ord_to_int(~w[k]) : ord_enc_int(FLT_MAX);
                    bhi[b][k] = bc[b] ? ord_to_int(w[3 + k]) : ord_enc_int(-FLT_MAX);
                }
            }
            int mn[HL_BINS - 1][3], mx[HL_BINS - 1][3], cr[HL_BINS - 1];
            int mnr[3] = {ord_enc_int(FLT_MAX), ord_enc_int(FLT_MAX), ord_enc_int(FLT_MAX)};
            int mxr[3] = {ord_enc_int(-FLT_MAX), ord_enc_int(-FLT_MAX), ord_enc_int(-FLT_MAX)};
            int cc = 0;
            for (int b = HL_BINS - 1; b > 0; b--) {
                for (int k = 0; k < 3; k++) { mnr[k] = min(mnr[k], blo[b][k]); mxr[k] = max(mxr[k], bhi[b][k]); mn[b - 1][k] = mnr[k]; mx[b - 1][k] = mxr[k]; }
                cc += bc[b];
                cr[b - 1] = cc;
            }
            int mnl[3] = {ord_enc_int(FLT_MAX), ord_enc_int(FLT_MAX), ord_enc_int(FLT_MAX)};
            int mxl[3] = {ord_enc_int(-FLT_MAX), ord_enc_int(-FLT_MAX), ord_enc_int(-FLT_MAX)};
            cc = 0;
            for (int b = 0; b < HL_BINS - 1; b++) {
                for (int k = 0; k < 3; k++) { mnl[k] = min(mnl[k], blo[b][k]); mxl[k] = max(mxl[k], bhi[b][k]); }
                cc += bc[b];
                const float s = (float)cc * area3(ord_dec_int(mxl[0]) - ord_dec_int(mnl[0]), ord_dec_int(mxl[1]) - ord_dec_int(mnl[1]),
                                                  ord_dec_int(mxl[2]) - ord_dec_int(mnl[2])) +
                                (float)cr[b] * area3(ord_dec_int(mx[b][0]) - ord_dec_int(mn[b][0]), ord_dec_int(mx[b][1]) - ord_dec_int(mn[b][1]),
                                                     ord_dec_int(mx[b][2]) - ord_dec_int(mn[b][2]));
                if (s < best) {
                    best = s; split = b; axis = a; cntL = cc; cntR = cr[b];
                    for (int k = 0; k < 3; k++) {
                        bl[k] = ord_dec_int(mnl[k]); bl[3 + k] = ord_dec_int(mxl[k]);
                        br[k] = ord_dec_int(mn[b][k]); br[3 + k] = ord_dec_int(mx[b][k]);
                    }
                }
            }
        }
        const int tBeg = tin.beg[t], nCls = tin.end[t] - tBeg;
        HlDec d;
        d.obj = split < 0;
        if (d.obj) {   // split missed: object split, both children get the box of the first occupied bin on axis 0 (canonical)
            for (int b = 0; b < HL_BINS; b++) {
                const unsigned int* w = bw + b * 8;
                if (w[6]) {
                    for (int k = 0; k < 3; k++) {
                        bl[k] = br[k] = ord_dec_int(ord_to_int(~w[k]));
                        bl[3 + k] = br[3 + k] = ord_dec_int(ord_to_int(w[3 + k]));
                    }
                    break;
                }
            }
            cntR = nCls / 2;
            cntL = nCls - cntR;
            axis = 0;
        }
        d.axis = axis; d.split = split; d.cntL = cntL; d.cntR = cntR; d.left = -1; d.right = -1; d.pad = 0;
        const int node = tin.node[t];
        int* nw = o.nodes + (size_t)node * 16;
        for (int side = 0; side < 2; side++) {
            const int cnt = side ? cntR : cntL;
            if (cnt <= 1) continue;
            const int ni = hl_alloc_node(st, o.nodeCap);
            const int slot = (int)atomicAdd(nextCount, 1u);
            const float* bx = side ? br : bl;
            tout.beg[slot] = side ? tBeg + cntL : tBeg;
            tout.end[slot] = side ? tBeg + nCls : tBeg + cntL;
            for (int k = 0; k < 6; k++) tout.box[6 * slot + k] = bx[k];
            tout.node[slot] = ni < 0 ? 0 : ni;
            if (side) d.right = slot; else d.left = slot;
            nw[12 + side] = ni < 0 ? 0 : ni * 64;
        }
        nw[14] = axis;
        nw[15] = 0;
        dec[t] = d;
        for (int w = 0; w < HL_BIN_WORDS; w++) bw[w] = 0;   // clean for the next level's task of this index
    }
}

__device__ __forceinline__ bool goes_left(const HlDec& d, int i, int tBeg, uchar4 b)
{
    if (d.obj) return i - tBeg < d.cntL;
    const int bin = d.axis == 0 ? b.x : (d.axis == 1 ? b.y : b.z);
    return bin <= d.split;
}

// left flags of the partition: per 1024 positions the count, per position the count before it inside its block
__global__ __launch_bounds__(256) void hl_left_count(int C, HlCls c, HlTasks tk, const HlDec* __restrict__ dec, const uchar4* __restrict__ cBin,
                                                     int* __restrict__ inBlock, int* __restrict__ blockCnt)
{
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    int f[4], v = 0;
    for (int k = 0; k < 4; k++) {
        const int i = base + k;
        f[k] = 0;
        if (i < C) {
            const int t = c.task[i];
            if (t >= 0) f[k] = goes_left(dec[t], i, tk.beg[t], cBin[i]) ? 1 : 0;
        }
        v += f[k];
    }
    int total;
    int r = block_exclusive_scan<256>(v, &total);
    for (int k = 0; k < 4; k++) {
        if (base + k < C) inBlock[base + k] = r;
        r += f[k];
    }
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = total;
}

// distribute (emitTreeKernel.cu:940-1027) as a stable partition: every cluster moves to its place in its child's range; a child of one
// cluster is terminated here -- a leaf, or the root of a bottom-level tree (queued for hl_bottom_emit)
__global__ __launch_bounds__(256) void hl_partition(int C, HlCls cin, HlCls cout, HlTasks tk, const HlDec* __restrict__ dec,
                                                    const uchar4* __restrict__ cBin, const int* __restrict__ inBlock,
                                                    const int* __restrict__ blockExcl, int4* __restrict__ bq, HlOut o, HlState* st)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C) return;
    const int t = cin.task[i];
    int pos = i, ntask = -1;
    const int s = cin.start[i], e = cin.end[i];
    if (t >= 0) {
        const HlDec d = dec[t];
        const int tBeg = tk.beg[t];
        const bool left = goes_left(d, i, tBeg, cBin[i]);
        const int lb = (blockExcl[i >> 10] + inBlock[i]) - (blockExcl[tBeg >> 10] + inBlock[tBeg]);
        pos = left ? tBeg + lb : tBeg + d.cntL + (i - tBeg - lb);
        if (pos < tBeg || pos >= tk.end[t]) { atomicOr(&st->overflow, 4u); return; }   // cannot happen; never write outside the range
        const int cnt = left ? d.cntL : d.cntR;
        if (cnt > 1) {
            ntask = left ? d.left : d.right;
        } else {
            const int side = left ? 0 : 1;
            int* nw = o.nodes + (size_t)tk.node[t] * 16;
            if (e - s <= o.leafSize) {
                nw[12 + side] = hl_leaf(o, st, s, e);
                nw[4 * side] = s;
                nw[4 * side + 1] = e;
            } else {
                const int ni = hl_alloc_node(st, o.nodeCap);
                nw[12 + side] = ni < 0 ? 0 : ni * 64;
                if (ni >= 0) {
                    const unsigned int q = atomicAdd(&st->bottomCount[0], 1u);
                    bq[q] = make_int4(ni, s, e, 0);
                }
            }
        }
    }
    cout.start[pos] = s;
    cout.end[pos] = e;
    for (int k = 0; k < 6; k++) cout.box[6 * pos + k] = cin.box[6 * i + k];
    cout.task[pos] = ntask;
}

__global__ void hl_level_end(int batch, const unsigned int* __restrict__ taskCount, unsigned int* __restrict__ lvlEnd, HlState* st, int topLevel)
{
    lvlEnd[batch] = st->nodeCount;
    if (taskCount && *taskCount > 0) st->topLevels = (unsigned int)topLevel + 1;
}

// ---- bottom level (emitTreeKernel.cu:233-381; host loop HLBVHBuilder.cpp:337-361 with bOfs = 3 * (10 - bits)) ------------------------
__global__ __launch_bounds__(256) void hl_bottom_emit(int level, const unsigned int* __restrict__ inCount, const int4* __restrict__ qin,
                                                      unsigned int* __restrict__ outCount, int4* __restrict__ qout, unsigned int qCap,
                                                      const unsigned int* __restrict__ keys, HlOut o, HlState* st)
{
    const int nq = (int)min(*inCount, qCap);
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int4 e4 = qin[q];
        const int nIdx = e4.x, nStart = e4.y, nEnd = e4.z;
        int lv = level;
        const int oldLevel = level;
        while (lv >= 0 && (((keys[nStart] >> lv) & 1u) == ((keys[nEnd - 1] >> lv) & 1u))) lv--;
        int split;
        if (lv >= 0) {
            const unsigned int startBit = (keys[nStart] >> lv) & 1u;
            int a = nStart, b = nEnd;
            for (;;) {
                split = (a + b) >> 1;
                const unsigned int splitBit = (keys[split] >> lv) & 1u;
                if (((keys[split - 1] >> lv) & 1u) != splitBit) break;
                if (splitBit == startBit) a = split; else b = split;
            }
        } else {
            split = (nStart + nEnd) >> 1;
        }
        int* nw = o.nodes + (size_t)nIdx * 16;
        for (int side = 0; side < 2; side++) {
            const int cs = side ? split : nStart, ce = side ? nEnd : split;
            if (ce - cs <= o.leafSize || oldLevel == 0) {
                nw[12 + side] = hl_leaf(o, st, cs, ce);
                nw[4 * side] = cs;
                nw[4 * side + 1] = ce;
            } else {
                const int ni = hl_alloc_node(st, o.nodeCap);
                nw[12 + side] = ni < 0 ? 0 : ni * 64;
                if (ni >= 0) {
                    const unsigned int s = atomicAdd(outCount, 1u);
                    if (s < qCap) qout[s] = make_int4(ni, cs, ce, 0); else atomicOr(&st->overflow, 4u);
                }
            }
        }
        nw[14] = lv % 3;
        nw[15] = 0;
    }
}

// ---- refit (calcAABB, emitTreeKernel.cu:383-562): one creation batch, deepest batch first --------------------------------------------
__global__ __launch_bounds__(256) void hl_refit(int batch, const unsigned int* __restrict__ lvlEnd, HlOut o)
{
    const int a = batch == 0 ? 0 : (int)lvlEnd[batch - 1], b = (int)lvlEnd[batch];
    for (int i = a + blockIdx.x * 256 + threadIdx.x; i < b; i += gridDim.x * 256) {
        int* w = o.nodes + (size_t)i * 16;
        float box[2][6];
        for (int k = 0; k < 2; k++) {
            const int ref = w[12 + k];
            if (ref < 0) {
                const int s = w[4 * k], e = w[4 * k + 1];
                float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
                for (int p = s; p < e; p++) {
                    const int t = o.triSorted[p];
                    const int v0 = o.tri[3 * t], v1 = o.tri[3 * t + 1], v2 = o.tri[3 * t + 2];
                    for (int c = 0; c < 3; c++) {
                        const float x = o.pos[3 * v0 + c], y = o.pos[3 * v1 + c], z = o.pos[3 * v2 + c];
                        lo[c] = fminf(lo[c], fminf(x, fminf(y, z)) - o.eps);
                        hi[c] = fmaxf(hi[c], fmaxf(x, fmaxf(y, z)) + o.eps);
                    }
                }
                box[k][0] = lo[0]; box[k][1] = hi[0]; box[k][2] = lo[1]; box[k][3] = hi[1]; box[k][4] = lo[2]; box[k][5] = hi[2];
            } else {
                const float* cn = (const float*)(o.nodes + (size_t)(ref / 64) * 16);
                box[k][0] = fminf(cn[0], cn[4]); box[k][1] = fmaxf(cn[1], cn[5]);
                box[k][2] = fminf(cn[2], cn[6]); box[k][3] = fmaxf(cn[3], cn[7]);
                box[k][4] = fminf(cn[8], cn[10]); box[k][5] = fmaxf(cn[9], cn[11]);
            }
        }
        float* f = (float*)w;
        f[0] = box[0][0]; f[1] = box[0][1]; f[2] = box[0][2]; f[3] = box[0][3];
        f[4] = box[1][0]; f[5] = box[1][1]; f[6] = box[1][2]; f[7] = box[1][3];
        f[8] = box[0][4]; f[9] = box[0][5]; f[10] = box[1][4]; f[11] = box[1][5];
    }
}

// Two grow-only pools per device: the first (codes, sort, clusters) is sized by numTris, the second (top-level tasks and bins) by the
// number of clusters, which is only known after the first phase.
namespace {
DeviceScratchPool g_hlA, g_hlB;
}  // namespace

}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_hlbvh_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                    const float sceneMin[3], const float sceneMax[3], int32_t leafSize, float epsilon, int32_t hlbvhBits,
                    void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                    int32_t* d_triIndex, int64_t triIndexCapacity, NtrHlbvhResult* result, void* stream)
{
    if (!result) return set_error(NTR_ERR_INVALID, "ntr_hlbvh_build: null result");
    memset(result, 0, sizeof(*result));
    if (hlbvhBits < 0 || hlbvhBits > 10) return set_error(NTR_ERR_INVALID, "ntr_hlbvh_build: hlbvhBits %d outside 0..10", (int)hlbvhBits);
    if (numTris < 1 || numVerts < 1 || leafSize < 1 || !d_triVtxIndex || !d_vtxPos || !sceneMin || !sceneMax)
        return set_error(NTR_ERR_INVALID, "ntr_hlbvh_build: bad geometry arguments");
    if (const int rc = check_build_outputs("ntr_hlbvh_build", numTris, d_nodes, nodesCapacity, d_triWoop, triWoopCapacity, d_triIndex,
                                           triIndexCapacity, nullptr, nullptr))
        return rc;
    const int n = numTris;
    if (n >= (1 << 27)) return set_error(NTR_ERR_INVALID, "ntr_hlbvh_build: at most 2^27 - 1 triangles");
    if (stream_is_capturing((hipStream_t)stream))
        return set_error(NTR_ERR_INVALID, "ntr_hlbvh_build: the call reads its counts back and cannot be captured");
    // HLBVHBuilder.cpp:44-47: hlbvhBits == 10 is buildLBVH; n <= leafSize is the LBVH's single root too (canonical)
    if (hlbvhBits == 10 || n <= leafSize) {
        const int rc = ntr_lbvh_build(numTris, d_triVtxIndex, numVerts, d_vtxPos, sceneMin, sceneMax, leafSize, epsilon, d_nodes, nodesCapacity,
                                      d_triWoop, triWoopCapacity, d_triIndex, triIndexCapacity, &result->lbvh, stream);
        return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const int bits = hlbvhBits;

    // ---- phase 1: codes, sort, clusters (pool A, sized by n) ----
    const int nb = (n + 1023) / 1024;
    ScratchCarver ca;
    const size_t oSort = ca.take(lbvh_sort_scratch_bytes(n));
    const size_t oState = ca.take(sizeof(HlState));
    const size_t oBlk = ca.take((size_t)nb * 4), oBlkEx = ca.take((size_t)nb * 4);
    const size_t oClsStart = ca.take(((size_t)n + 1) * 4), oClsOf = ca.take((size_t)n * 4);
    const size_t oBq0 = ca.take(((size_t)n + 2) * 16), oBq1 = ca.take(((size_t)n + 2) * 16);
    void* baseA = nullptr;
    {
        const int rc = g_hlA.reserve(ca.off, &baseA);
        if (rc != NTR_OK) return rc;
    }
    char* wa = (char*)baseA;
    HlState* st = (HlState*)(wa + oState);
    int* clsStart = (int*)(wa + oClsStart);
    int* clsOf = (int*)(wa + oClsOf);
    int4* bq[2] = {(int4*)(wa + oBq0), (int4*)(wa + oBq1)};

    StreamEvents<6> pe(s);
    (void)pe.create();
    pe.mark(0);
    {
        HlState init;
        memset(&init, 0, sizeof(init));
        init.nodeCount = 1;
        NTR_HIP(hipMemcpyAsync(st, &init, sizeof(init), hipMemcpyHostToDevice, s));
    }
    const unsigned int* keys = nullptr;
    const int* triSorted = nullptr;
    const unsigned int* sortErr = nullptr;
    {
        const int rc = lbvh_sort_codes(n, d_triVtxIndex, d_vtxPos, sceneMin, sceneMax, wa + oSort, s, &keys, &triSorted, &sortErr);
        if (rc != NTR_OK) return rc;
    }
    pe.mark(1);
    hipLaunchKernelGGL(hl_head_count, dim3(nb), dim3(256), 0, s, n, bits, keys, (int*)(wa + oBlk));
    hipLaunchKernelGGL((scan_block_sums<1024, int>), dim3(1), dim3(1024), 0, s, nb, (const int*)(wa + oBlk), (int*)(wa + oBlkEx),
                       (int*)&st->numClusters);
    hipLaunchKernelGGL(hl_head_emit, dim3(nb), dim3(256), 0, s, n, bits, keys, (const int*)(wa + oBlkEx), clsStart, clsOf);
    NTR_HIP(hipGetLastError());
    unsigned int C = 0;
    NTR_HIP(hipMemcpyAsync(&C, &st->numClusters, 4, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    if (C < 1 || C > (unsigned int)n) return set_error(NTR_ERR_HIP, "ntr_hlbvh_build: cluster count %u out of range (internal error)", C);

    // ---- phase 2 buffers (pool B, sized by the cluster count) ----
    const int maxTasks = (int)C / 2 + 2;
    const int maxLevels = (int)C + HL_CHUNK + 2;
    const int maxBatches = maxLevels + 3 * bits + 2;
    const int cb = ((int)C + 1023) / 1024;
    ScratchCarver cbv;
    size_t oC[2][4], oT[2][4];
    for (int p = 0; p < 2; p++) {
        oC[p][0] = cbv.take((size_t)C * 4); oC[p][1] = cbv.take((size_t)C * 4); oC[p][2] = cbv.take((size_t)C * 24); oC[p][3] = cbv.take((size_t)C * 4);
        oT[p][0] = cbv.take((size_t)maxTasks * 4); oT[p][1] = cbv.take((size_t)maxTasks * 4); oT[p][2] = cbv.take((size_t)maxTasks * 24);
        oT[p][3] = cbv.take((size_t)maxTasks * 4);
    }
    const size_t oBin = cbv.take((size_t)maxTasks * HL_BIN_WORDS * 4);
    const size_t oCBin = cbv.take((size_t)C * 4);
    const size_t oDec = cbv.take((size_t)maxTasks * sizeof(HlDec));
    const size_t oInBlock = cbv.take((size_t)C * 4);
    const size_t oCBlk = cbv.take((size_t)cb * 4), oCBlkEx = cbv.take((size_t)cb * 4);
    const size_t oTCount = cbv.take((size_t)maxLevels * 4);
    const size_t oLvl = cbv.take((size_t)maxBatches * 4);
    const size_t oZeroEnd = cbv.off;
    void* baseB = nullptr;
    {
        const int rc = g_hlB.reserve(cbv.off, &baseB);
        if (rc != NTR_OK) return rc;
    }
    char* wb = (char*)baseB;
    HlCls cls[2];
    HlTasks tks[2];
    for (int p = 0; p < 2; p++) {
        cls[p] = {(int*)(wb + oC[p][0]), (int*)(wb + oC[p][1]), (int*)(wb + oC[p][2]), (int*)(wb + oC[p][3])};
        tks[p] = {(int*)(wb + oT[p][0]), (int*)(wb + oT[p][1]), (float*)(wb + oT[p][2]), (int*)(wb + oT[p][3])};
    }
    unsigned int* bins = (unsigned int*)(wb + oBin);
    uchar4* cBin = (uchar4*)(wb + oCBin);
    HlDec* dec = (HlDec*)(wb + oDec);
    unsigned int* tCount = (unsigned int*)(wb + oTCount);
    unsigned int* lvlEnd = (unsigned int*)(wb + oLvl);
    NTR_HIP(hipMemsetAsync(wb + oBin, 0, oZeroEnd - oBin, s));   // bins, bin ids, decisions, scans, task counts, batch ends

    HlOut o;
    o.nodes = (int*)d_nodes; o.nodeCap = (unsigned int)(nodesCapacity / 64);
    o.woop = (float4*)d_triWoop; o.idx = d_triIndex;
    o.entryCap = triWoopCapacity / 16 < triIndexCapacity / 4 ? triWoopCapacity / 16 : triIndexCapacity / 4;
    o.tri = d_triVtxIndex; o.pos = d_vtxPos; o.triSorted = triSorted; o.leafSize = leafSize; o.eps = epsilon;

    const unsigned int one = 1;
    NTR_HIP(hipMemcpyAsync(lvlEnd, &one, 4, hipMemcpyHostToDevice, s));   // batch 0: the root
    const int gC = ((int)C + 255) / 256;
    if (C >= 2) {
        hipLaunchKernelGGL(hl_cluster_init, dim3(gC), dim3(256), 0, s, (int)C, (const int*)clsStart, cls[0]);
        const int boxThreads = (n + HL_BOX_CHUNK - 1) / HL_BOX_CHUNK;
        hipLaunchKernelGGL(hl_cluster_box, dim3((boxThreads + 255) / 256), dim3(256), 0, s, n, d_triVtxIndex, d_vtxPos, triSorted,
                           (const int*)clsOf, (const int*)clsStart, cls[0].box);
        // the root task: every cluster, the caller's scene box (HLBVHBuilder.cpp:227-233)
        const int rootTask[2] = {0, (int)C};
        const float rootBox[6] = {sceneMin[0], sceneMin[1], sceneMin[2], sceneMax[0], sceneMax[1], sceneMax[2]};
        const int zero = 0;
        NTR_HIP(hipMemcpyAsync(tks[0].beg, &rootTask[0], 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(tks[0].end, &rootTask[1], 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(tks[0].box, rootBox, 24, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(tks[0].node, &zero, 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(tCount, &one, 4, hipMemcpyHostToDevice, s));
    } else {
        // fewer than two clusters: the whole range is one bottom-level tree (canonical; the reference writes a self-referencing root)
        const int4 root = make_int4(0, 0, n, 0);
        NTR_HIP(hipMemcpyAsync(bq[0], &root, 16, hipMemcpyHostToDevice, s));
        NTR_HIP(hipMemcpyAsync(&st->bottomCount[0], &one, 4, hipMemcpyHostToDevice, s));
    }
    pe.mark(2);

    // ---- phase 3: top level, HL_CHUNK levels per read-back ----
    int topLevels = 0;
    if (C >= 2) {
        const int gT = (maxTasks + 255) / 256 < 1024 ? (maxTasks + 255) / 256 : 1024;
        int level = 0;
        for (;;) {
            for (int k = 0; k < HL_CHUNK; k++, level++) {
                const int p = level & 1;
                hipLaunchKernelGGL(hl_fill_bins, dim3(gC), dim3(256), 0, s, (int)C, cls[p], tks[p], bins, cBin);
                hipLaunchKernelGGL(hl_find_split, dim3(gT), dim3(256), 0, s, (const unsigned int*)(tCount + level), tCount + level + 1, tks[p],
                                   tks[p ^ 1], bins, dec, o, st);
                hipLaunchKernelGGL(hl_left_count, dim3(cb), dim3(256), 0, s, (int)C, cls[p], tks[p], (const HlDec*)dec, (const uchar4*)cBin,
                                   (int*)(wb + oInBlock), (int*)(wb + oCBlk));
                hipLaunchKernelGGL((scan_block_sums<1024, int>), dim3(1), dim3(1024), 0, s, cb, (const int*)(wb + oCBlk), (int*)(wb + oCBlkEx), (int*)nullptr);
                hipLaunchKernelGGL(hl_partition, dim3(gC), dim3(256), 0, s, (int)C, cls[p], cls[p ^ 1], tks[p], (const HlDec*)dec, (const uchar4*)cBin,
                                   (const int*)(wb + oInBlock), (const int*)(wb + oCBlkEx), bq[0], o, st);
                hipLaunchKernelGGL(hl_level_end, dim3(1), dim3(1), 0, s, level + 1, (const unsigned int*)(tCount + level), lvlEnd, st, level);
            }
            NTR_HIP(hipGetLastError());
            unsigned int alive = 0;
            NTR_HIP(hipMemcpyAsync(&alive, tCount + level, 4, hipMemcpyDeviceToHost, s));
            NTR_HIP(hipStreamSynchronize(s));
            if (!alive) break;
            if (level + HL_CHUNK + 1 >= maxLevels)
                return set_error(NTR_ERR_HIP, "ntr_hlbvh_build: top level did not finish within %u levels (internal error)", C);
        }
        unsigned int tl = 0;
        NTR_HIP(hipMemcpyAsync(&tl, &st->topLevels, 4, hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        topLevels = (int)tl;
    }
    pe.mark(3);

    // ---- phase 4: bottom level, 3 * bits levels from level 3 * bits - 1 down to 0 ----
    const int gB = 1024;
    for (int l = 0; l < 3 * bits; l++) {
        hipLaunchKernelGGL(hl_bottom_emit, dim3(gB), dim3(256), 0, s, 3 * bits - 1 - l, (const unsigned int*)&st->bottomCount[l],
                           (const int4*)bq[l & 1], &st->bottomCount[l + 1], bq[(l + 1) & 1], (unsigned int)n + 2u, keys, o, st);
        hipLaunchKernelGGL(hl_level_end, dim3(1), dim3(1), 0, s, topLevels + 1 + l, (const unsigned int*)nullptr, lvlEnd, st, 0);
    }
    pe.mark(4);
    // ---- phase 5: refit, deepest batch first ----
    const int numBatches = topLevels + 1 + 3 * bits;
    for (int b = numBatches - 1; b >= 0; b--) hipLaunchKernelGGL(hl_refit, dim3(gB), dim3(256), 0, s, b, (const unsigned int*)lvlEnd, o);
    pe.mark(5);
    NTR_HIP(hipGetLastError());
    HlState h;
    unsigned int sortBad = 0;
    NTR_HIP(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipMemcpyAsync(&sortBad, sortErr, 4, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    if (sortBad) return set_error(NTR_ERR_HIP, "ntr_hlbvh_build: a chained scan timed out waiting for a predecessor tile (status %u)", sortBad);
    if (h.overflow & 4u) return set_error(NTR_ERR_HIP, "ntr_hlbvh_build: a work queue left its bounds (internal error)");
    if (h.overflow) return set_error(NTR_ERR_OVERFLOW, "ntr_hlbvh_build: output buffer overflow (flags %u)", h.overflow);
    if (h.bottomCount[3 * bits] != 0) return set_error(NTR_ERR_HIP, "ntr_hlbvh_build: bottom level did not terminate (internal error)");
    if ((int64_t)h.nodeCount > kMaxNodes)
        return set_error(NTR_ERR_OVERFLOW, "ntr_hlbvh_build: %u nodes exceed what BVHLayout_Compact's 32-bit child offsets address", h.nodeCount);
    const unsigned int leafs = (unsigned int)(h.leafPtr & 0xFFFFFFFFull);
    NtrLbvhResult& r = result->lbvh;
    r.numNodes = (int32_t)h.nodeCount;
    r.numLeaves = (int32_t)leafs;
    r.numLevels = numBatches;
    r.nodesBytes = (int64_t)h.nodeCount * 64;
    r.triWoopBytes = ((int64_t)n * 3 + leafs) * 16;
    r.triIndexBytes = ((int64_t)n * 3 + leafs) * 4;
    r.mortonMs = 0.0f;
    r.sortMs = pe.ms(0, 1);
    r.emitMs = pe.ms(3, 4);
    r.refitMs = pe.ms(4, 5);
    r.seconds = pe.ms(0, 5) * 1e-3f;
    result->numClusters = (int32_t)C;
    result->topNodes = C >= 2 ? (int32_t)C - 1 : 0;
    result->topLevels = topLevels;
    result->clusterMs = pe.ms(1, 2);
    result->topMs = pe.ms(2, 3);
    result->bottomMs = pe.ms(3, 5);
    return NTR_OK;
}

}  // extern "C"
