// device_prims.h -- device primitives of the on-device builders and tree passes (hlbvh_, kdtree_build_, bvh_build_, sah_build_,
// bvh_refit_, bvh_optimize_, bvh_reorder_kernels.hip, bvh_utils.hip) and the ray sort (rayops_kernels.hip): workgroup scans and the four-counter
// value the level loops scan, wave folds, the order-preserving float encoding with its min / max, a box as six words merged by integer
// max, box areas, a triangle's checked indices and box, the leaf rows' emit kernel.  The LBVH keeps its own tuned scans (radix_sort.h).
// The level loop's shared parts: level_build.h.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <string.h>

#include "woop_rows.h"

namespace ntr {

// Four counters scanned together (a level loop's inner nodes, rows, references, ...)
struct U4 {
    unsigned int x, y, z, w;
    __device__ U4 operator+(const U4& b) const { return U4{x + b.x, y + b.y, z + b.z, w + b.w}; }
};

// Exclusive scan over a workgroup of THREADS threads (Hillis-Steele in LDS); *total receives the workgroup's sum.  V is an integer
// type or a struct of them with operator+ (V{} is its zero), so the sums are exact.  Every thread of the workgroup calls it.
template <int THREADS, class V>
__device__ V block_exclusive_scan(V v, V* total)
{
    __shared__ V sh[THREADS];
    const int i = threadIdx.x;
    sh[i] = v;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const V a = i >= off ? sh[i - off] : V{};
        __syncthreads();
        if (i >= off) sh[i] = sh[i] + a;
        __syncthreads();
    }
    *total = sh[THREADS - 1];
    const V ex = i > 0 ? sh[i - 1] : V{};
    __syncthreads();   // sh is reused by the next call
    return ex;
}

// The first of a scan's three launches, for the thread of item i (all threads of the workgroup call it): the item's rank inside the
// workgroup to local[i] if `valid`, the workgroup's sum to blockSums[block].
template <int THREADS, class V>
__device__ __forceinline__ void scan_local_store(V v, bool valid, size_t i, V* __restrict__ local, V* __restrict__ blockSums, int block)
{
    V total;
    const V ex = block_exclusive_scan<THREADS>(v, &total);
    if (valid) local[i] = ex;
    if (threadIdx.x == 0) blockSums[block] = total;
}

// One workgroup: exclusive scan of nb block sums, in[i] -> out[i] (in place when in == out); the grand total to *total unless it
// is null.
template <int THREADS, class V>
__global__ __launch_bounds__(THREADS) void scan_block_sums(int nb, const V* in, V* out, V* total)
{
    V carry{};
    for (int base = 0; base < nb; base += THREADS) {
        const int i = base + threadIdx.x;
        const V v = i < nb ? in[i] : V{};
        V chunk;
        const V ex = block_exclusive_scan<THREADS>(v, &chunk);
        if (i < nb) out[i] = carry + ex;
        carry = carry + chunk;
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

// Order-preserving float encoding for integer atomics on floats: a < b in the floats' total order (-0 < +0, NaNs beyond the
// infinities by their sign) iff ord_enc(a) < ord_enc(b) as unsigned words.  The signed form ord_enc_int(f) == ord_to_int(ord_enc(f))
// is the same order under signed compares; it is written out on its own because the HLBVH kernels' code is smaller that way.
__device__ __forceinline__ unsigned int ord_enc(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord_dec(unsigned int u)
{
    const unsigned int b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
__host__ __device__ __forceinline__ int ord_to_int(unsigned int u) { return (int)(u ^ 0x80000000u); }
__host__ __device__ __forceinline__ unsigned int ord_from_int(int i) { return (unsigned int)i ^ 0x80000000u; }
__device__ __forceinline__ int ord_enc_int(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7FFFFFFF; }
__device__ __forceinline__ float ord_dec_int(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

// min / max in that total order (-0 < +0), so that no result depends on the order of the operands
__device__ __forceinline__ float ord_min(float a, float b) { return ord_enc(a) <= ord_enc(b) ? a : b; }
__device__ __forceinline__ float ord_max(float a, float b) { return ord_enc(a) >= ord_enc(b) ? a : b; }

// ---- wave folds: the result in every lane; all 64 lanes call them ---------------------------------------------------------
template <class F>
__device__ __forceinline__ unsigned int wave_fold_u32(unsigned int v, F f)
{
    for (int off = 32; off > 0; off >>= 1) v = f(v, (unsigned int)__shfl_xor((int)v, off));
    return v;
}
__device__ __forceinline__ unsigned int wave_max_u32(unsigned int v) { return wave_fold_u32(v, [](unsigned int a, unsigned int b) { return max(a, b); }); }
__device__ __forceinline__ unsigned int wave_min_u32(unsigned int v) { return wave_fold_u32(v, [](unsigned int a, unsigned int b) { return min(a, b); }); }
__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) { return wave_fold_u32(v, [](unsigned int a, unsigned int b) { return a + b; }); }
__device__ __forceinline__ unsigned int wave_or_u32(unsigned int v) { return wave_fold_u32(v, [](unsigned int a, unsigned int b) { return a | b; }); }
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, off);
        const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}
// every lane of the wave holds the same g
__device__ __forceinline__ bool wave_uniform(int g) { return __all(g == __shfl(g, 0)) != 0; }
// Lanes with g >= 0 merge v into group g by the atomic op(g, v): one atomic of the wave's fold when the wave shares one group
template <class V, class Fold, class Op>
__device__ __forceinline__ void wave_grouped_atomic(int g, V v, Fold fold, Op op)
{
    if (wave_uniform(g)) {
        const V m = fold(v);
        if (g >= 0 && (threadIdx.x & 63) == 0) op(g, m);
    } else if (g >= 0) op(g, v);
}

__device__ __forceinline__ float sel3(const float* v, int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }
// areaAABB (rt_common.cu:850-858, emitTreeKernel.cu:119-121) of a box of extents x, y, z
__device__ __forceinline__ float area3(float x, float y, float z) { return (x * y + y * z + z * x) * 2.0f; }
// Two rules for a box given by its corners, kept apart on purpose: box_area is areaAABB as it stands (an inverted box gives whatever the
// arithmetic gives; the binned builders' costs rely on it), box_area_valid is AABB::area of the host builders, 0 for an invalid box.
__device__ __forceinline__ float box_area(const float* lo, const float* hi) { return area3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]); }
__device__ __forceinline__ float box_area_valid(const float* lo, const float* hi)
{
    return (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) ? box_area(lo, hi) : 0.0f;
}

// ---- a box as six words merged by integer max: ~ord_enc(min) x3, ord_enc(max) x3; all zero is the empty box ----------------
__device__ __forceinline__ void box_words(const float4& lo, const float4& hi, unsigned int* w)
{
    w[0] = ~ord_enc(lo.x); w[1] = ~ord_enc(lo.y); w[2] = ~ord_enc(lo.z);
    w[3] = ord_enc(hi.x); w[4] = ord_enc(hi.y); w[5] = ord_enc(hi.z);
}
__device__ __forceinline__ void atomic_max_box(unsigned int* dst, const unsigned int* w)
{
#pragma unroll
    for (int k = 0; k < 6; k++) atomicMax(&dst[k], w[k]);
}
// words -> corners; with grow: fl(min - eps), fl(max + eps).  A box of no members (count == 0) is (FLT_MAX, -FLT_MAX), AABB's initial box.
__device__ __forceinline__ void words_box(int count, const unsigned int* w, float eps, bool grow, float* lo, float* hi)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float l = ord_dec(~w[k]), h = ord_dec(w[3 + k]);
        lo[k] = count ? (grow ? l - eps : l) : FLT_MAX;
        hi[k] = count ? (grow ? h + eps : h) : -FLT_MAX;
    }
}
// box_area_valid of the words as they are (the empty box decodes to an invalid one: 0)
__device__ __forceinline__ float words_area(const unsigned int* w)
{
    float lo[3], hi[3];
    words_box(1, w, 0.0f, false, lo, hi);
    return box_area_valid(lo, hi);
}

// ---- a triangle of the mesh -------------------------------------------------------------------------------------------------
// triangle t's vertex indices; false if one is outside [0, numVerts)
__device__ __forceinline__ bool tri_indices_checked(const int* __restrict__ tri, int numVerts, int t, int& i0, int& i1, int& i2)
{
    i0 = tri[3 * (size_t)t]; i1 = tri[3 * (size_t)t + 1]; i2 = tri[3 * (size_t)t + 2];
    return !(i0 < 0 || i0 >= numVerts || i1 < 0 || i1 >= numVerts || i2 < 0 || i2 >= numVerts);
}
// ... and its box by ord_min / ord_max; lo and hi are left alone when an index is out of range
__device__ __forceinline__ bool tri_box_checked(const int* __restrict__ tri, int numVerts, const float* __restrict__ pos, int t, float* lo,
                                                float* hi)
{
    int i0, i1, i2;
    if (!tri_indices_checked(tri, numVerts, t, i0, i1, i2)) return false;
    for (int k = 0; k < 3; k++) {
        const float a = pos[3 * (size_t)i0 + k], b = pos[3 * (size_t)i1 + k], d = pos[3 * (size_t)i2 + k];
        lo[k] = ord_min(ord_min(a, b), d);
        hi[k] = ord_max(ord_max(a, b), d);
    }
    return true;
}

// The end of a level-synchronous build: every triangle's three Woop rows (woop_rows.h) and its triIndex entries at its leaf row.
// liveFlag (or null: every triangle) leaves out the triangles the build dropped; a row outside [0, rowCap - 2) sets errBit in *err.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void emit_leaf_rows(int n, const int* __restrict__ tri, const float* __restrict__ pos,
                                                          const unsigned char* __restrict__ liveFlag, const int* __restrict__ leafRow,
                                                          int rowCap, float4* __restrict__ woop, int* __restrict__ triIndex,
                                                          unsigned int* __restrict__ err, unsigned int errBit)
{
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n || (liveFlag && !liveFlag[i])) return;
    const int row = leafRow[i];
    if (row < 0 || row + 2 >= rowCap) { atomicOr(err, errBit); return; }
    float4 r0, r1, r2;
    woop_rows(tri, pos, i, r0, r1, r2);
    woop[row] = r0; woop[row + 1] = r1; woop[row + 2] = r2;
    triIndex[row] = i; triIndex[row + 1] = 0; triIndex[row + 2] = 0;
}

}  // namespace ntr
