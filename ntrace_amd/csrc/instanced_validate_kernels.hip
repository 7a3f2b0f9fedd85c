// instanced_validate_kernels.hip -- the validate flags of a two-level scene, kept on the device (ntr_instanced_validate,
// ntr_instanced_flags_read; the rule is tests/np_instanced_fast.py, validate).  ntr_bvh_validate allocates, blocks on a
// read-back and refreshes the single-level top-of-tree table: it cannot run inside a captured frame, and its answer goes stale each time
// vertices move.  This pass clears the four words and makes one grid-stride launch over the top-level nodes and the pool's nodes; the
// fast two-level trace (trace_instanced_fast_kernels.hip) reads the two words at launch or replay time.  The clear is a one-wave kernel
// and not hipMemsetAsync: a 16-byte memset node of a captured graph left other bytes than zeros in the words when the graph was replayed
// (tests/test_instanced_fast_gpu.py, the captured validate; sched_kernels.hip met the same with its counters), kernels replay as captured.
//   d_flags[0], d_flags[1]   the WITHHELD bits of the top-level tree and of the pool (NTR_BVH_FINITE / FASTDIV / NOTINY / ORDERED): an OR
//                            from any wave is the whole protocol, no wave has to see the others' answer
//   d_flags[2], d_flags[3]   zero
// The rule is bvh_validate_kernel's (bvh_utils.hip) for those four flags: the twelve box floats of every 64-byte node, never the child
// words; every node slot in [0, bytes) counts, a pool's slack and gaps too.
// ntr_instanced_wide_validate (the rule is tests/np_instanced_wide_fast.py, validate) is the same pass over the 4-wide
// buffers of the same scene, for ntr_trace_instanced_wide_fast: the all-wide update path runs no binary refit, so the binary buffers'
// flags say nothing about the wide boxes.  The same two kernels serve it: a 128-byte wide node (wide_bvh.h) is rows 0..2 and 4..6 of
// (lo, hi) pairs in Compact's box words, row 3 the links and row 7 the count -- every fourth float4 is skipped in either layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "instanced_wide_bvh.h"

namespace ntr {
namespace {

// float4 i of the joint range: [0, tlas4) the top level, [tlas4, tlas4 + pool4) the pool.  A wave may straddle the seam: it keeps the
// two levels' bits apart.
__global__ __launch_bounds__(256) void instanced_validate_kernel(const float4* __restrict__ tlas, int64_t tlas4, const float4* __restrict__ pool,
                                                                 int64_t pool4, unsigned int* __restrict__ flags)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, total = tlas4 + pool4;
    unsigned int held[2] = {0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        // the child words of a 64-byte node; of a 128-byte wide node row 3, the links, and row 7, the count (both buffers are whole
        // nodes, so the seam keeps i's phase)
        if ((i & 3) == 3) continue;
        const bool top = i < tlas4;
        const float4 v = top ? tlas[i] : pool[i - tlas4];
        const float c[4] = {v.x, v.y, v.z, v.w};
        unsigned int bits = (!(v.x <= v.y) || !(v.z <= v.w)) ? NTR_BVH_ORDERED : 0u;   // every box float4 is two (lo, hi) pairs
        for (int k = 0; k < 4; k++) {
            const float a = fabsf(c[k]);
            if (!(a < 0x1p100f)) bits |= NTR_BVH_FINITE;                    // also true for NaN
            if (!(a < 0x1p55f)) bits |= NTR_BVH_FASTDIV;
            if (!(c[k] == 0.0f || a >= 0x1p-93f)) bits |= NTR_BVH_NOTINY;   // a NaN is neither
        }
        held[top ? 0 : 1] |= bits;
    }
    for (int l = 0; l < 2; l++) {
        unsigned int w = 0u;
        for (unsigned int b = 1u; b <= NTR_BVH_ORDERED; b <<= 1)
            if (__ballot((held[l] & b) != 0u) != 0ull) w |= b;
        if (w && (threadIdx.x & 63) == 0) atomicOr(&flags[l], w);
    }
}

__global__ __launch_bounds__(64) void instanced_flags_clear_kernel(unsigned int* __restrict__ flags)
{
    if (threadIdx.x < 4) flags[threadIdx.x] = 0u;
}

constexpr uint32_t kFourFlags = NTR_BVH_FINITE | NTR_BVH_FASTDIV | NTR_BVH_NOTINY | NTR_BVH_ORDERED;

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_instanced_validate(const void* d_tlasNodes, int64_t tlasNodesBytes, const void* d_poolNodes, int64_t poolNodesBytes,
                                      uint32_t* d_flags, void* stream)
{
    const char* fn = "ntr_instanced_validate";
    if (!d_flags || !d_poolNodes) return set_error(NTR_ERR_INVALID, "%s: null flags or null pool", fn);
    if (tlasNodesBytes < 0 || (tlasNodesBytes % kNodeBytes) != 0 || tlasNodesBytes > kMaxNodesBytes)
        return set_error(NTR_ERR_INVALID, "%s: tlasNodesBytes must be a multiple of 64 in [0, 0x%llx]", fn, (unsigned long long)kMaxNodesBytes);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (((((uintptr_t)d_flags) | ((uintptr_t)d_tlasNodes) | ((uintptr_t)d_poolNodes)) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: the flags and the node buffers must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tlas4 = d_tlasNodes ? tlasNodesBytes / 16 : 0, pool4 = poolNodesBytes / 16;
    int64_t blocks = (tlas4 + pool4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(instanced_flags_clear_kernel, dim3(1), dim3(64), 0, s, (unsigned int*)d_flags);
    hipLaunchKernelGGL(instanced_validate_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)d_tlasNodes, tlas4,
                       (const float4*)d_poolNodes, pool4, (unsigned int*)d_flags);
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

extern "C" int ntr_instanced_wide_validate(const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, const void* d_widePoolNodes,
                                           int64_t widePoolNodesBytes, uint32_t* d_flags, void* stream)
{
    const char* fn = "ntr_instanced_wide_validate";
    if (!d_flags || !d_widePoolNodes) return set_error(NTR_ERR_INVALID, "%s: null flags or null pool", fn);
    if (wideTlasNodesBytes != 0)
        if (const int rc = check_wide_bytes(fn, wideTlasNodesBytes)) return rc;
    if (const int rc = check_wide_pool_bytes(fn, "widePoolNodesBytes", widePoolNodesBytes)) return rc;
    if (((((uintptr_t)d_flags) | ((uintptr_t)d_wideTlasNodes) | ((uintptr_t)d_widePoolNodes)) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: the flags and the node buffers must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tlas4 = d_wideTlasNodes ? wideTlasNodesBytes / 16 : 0, pool4 = widePoolNodesBytes / 16;
    int64_t blocks = (tlas4 + pool4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(instanced_flags_clear_kernel, dim3(1), dim3(64), 0, s, (unsigned int*)d_flags);
    hipLaunchKernelGGL(instanced_validate_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)d_wideTlasNodes, tlas4,
                       (const float4*)d_widePoolNodes, pool4, (unsigned int*)d_flags);
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

extern "C" int ntr_instanced_flags_read(const uint32_t* d_flags, uint32_t* tlasFlags, uint32_t* poolFlags, void* stream)
{
    const char* fn = "ntr_instanced_flags_read";
    if (tlasFlags) *tlasFlags = 0;
    if (poolFlags) *poolFlags = 0;
    if (!d_flags || !tlasFlags || !poolFlags || (((uintptr_t)d_flags) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: null argument, or flags that are not 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads back and cannot be captured", fn);
    uint32_t h[2] = {0u, 0u};
    NTR_HIP(hipMemcpyAsync(h, d_flags, sizeof(h), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    *tlasFlags = ~h[0] & kFourFlags;
    *poolFlags = ~h[1] & kFourFlags;
    return NTR_OK;
}
