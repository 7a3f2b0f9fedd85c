// device_prims.h -- device primitives of the on-device builders (hlbvh_kernels.hip, kdtree_build_kernels.hip) and the ray sort
// (rayops_kernels.hip): a workgroup exclusive scan, a one-workgroup scan of block sums, the order-preserving float encoding and the
// surface area of a box.  The LBVH keeps its own tuned scans (lbvh_kernels.hip, radix_sort.h).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

namespace ntr {

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

// areaAABB (rt_common.cu:850-858, emitTreeKernel.cu:119-121) of a box of extents x, y, z
__device__ __forceinline__ float area3(float x, float y, float z) { return (x * y + y * z + z * x) * 2.0f; }

}  // namespace ntr
