// instances_update_kernels.hip -- the NtrInstance array from a hierarchy of transforms, on the device for gfx950 (ntr_instances_update,
// ntr_instances_status_read).  EXTENSION: the rule is the numpy spec tests/np_instance_update.py, which the kernel equals byte for byte;
// the header comment of ntr_instances_update (include/ntrace_amd.h) states it, DESIGN.md 6z measures it.
//   iu_reset    one thread: the status words (0, 0xFFFFFFFF, 0, 0), ahead of the kernel on the same stream
//   iu_update   one thread per instance: walks its chain upward (at most 16 dependent 4-byte loads, the indices kept in registers), folds
//               downward from the root in binary64 (instance_math.h: the host's statements), rounds once, inverts the rounded matrix
//               and writes the 112-byte record as seven 16-byte stores.  No thread reads what another wrote: a shared ancestor is
//               recomputed by every instance below it, which keeps one launch, no scratch and one association order.  A wave with a
//               bad lane folds (bits, lowest index, count) and its first lane sets the status words with one atomic each, as
//               tl_boxes does for its box.
// The call allocates nothing and keeps nothing on the host, so it is capturable from the first call on.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <chrono>

#include "ntr_internal.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instance_math.h"

namespace ntr {
namespace {

constexpr int IU_BLOCK = 256;
constexpr int IU_MAX_CHAIN = NTR_INSTANCE_MAX_CHAIN;
static_assert(IU_BLOCK % 64 == 0, "whole waves fold the status");
static_assert(sizeof(NtrInstance) == 7 * sizeof(uint4), "the record is seven 16-byte stores");

__global__ __launch_bounds__(64) void iu_reset(uint4* __restrict__ status)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = make_uint4(0u, 0xFFFFFFFFu, 0u, 0u);
}

__device__ __forceinline__ uint4 iu_words(const float* f)
{
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
}

__global__ __launch_bounds__(IU_BLOCK) void iu_update(int numNodes, const float4* __restrict__ local, const int* __restrict__ parent /* or null */,
                                                      int n, const int* __restrict__ node /* or null */, const int* __restrict__ blas,
                                                      uint4* __restrict__ out, unsigned int* __restrict__ status)
{
    const int i = blockIdx.x * IU_BLOCK + threadIdx.x;
    unsigned int bad = 0u;
    if (i < n) {
        // upward: path[0] the instance's own node ... path[len - 1] the root.  Constant indices only: the path lives in registers
        int path[IU_MAX_CHAIN];
        int len = 0, k = node ? node[i] : i;
        bool walking = true;
        if (k < 0 || k >= numNodes) { bad = NTR_INSTANCE_ERR_CHAIN; walking = false; }
#pragma unroll
        for (int j = 0; j < IU_MAX_CHAIN; j++) {
            path[j] = 0;
            if (walking) {
                path[j] = k;
                len = j + 1;
                const int p = parent ? parent[k] : -1;
                if (p == -1) walking = false;
                else if (p < 0 || p >= numNodes) { bad = NTR_INSTANCE_ERR_CHAIN; walking = false; }
                else k = p;
            }
        }
        if (walking) bad = NTR_INSTANCE_ERR_CHAIN;   // a seventeenth transform, or a cycle

        float m[12], inv[12];
#pragma unroll
        for (int c = 0; c < 12; c++) m[c] = inv[c] = 0.0f;
        if (!bad) {
            double acc[12];
#pragma unroll
            for (int j = IU_MAX_CHAIN - 1; j >= 0; j--) {
                if (j < len) {
                    const float4* src = local + 3 * (size_t)path[j];
                    const float4 r0 = src[0], r1 = src[1], r2 = src[2];
                    const float l[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
                    if (j == len - 1) {
#pragma unroll
                        for (int c = 0; c < 12; c++) acc[c] = (double)l[c];
                    } else {
                        instance_compose(acc, l);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 12; c++) m[c] = (float)acc[c];
            if (!instance_invert(m, inv)) bad = NTR_INSTANCE_ERR_SINGULAR;   // (nothing written: inv stays twelve +0)
        }
        uint4* rec = out + 7 * (size_t)i;
        rec[0] = iu_words(m);
        rec[1] = iu_words(m + 4);
        rec[2] = iu_words(m + 8);
        rec[3] = iu_words(inv);
        rec[4] = iu_words(inv + 4);
        rec[5] = iu_words(inv + 8);
        rec[6] = make_uint4((unsigned int)blas[i], 0u, 0u, 0u);
    }
    // all 64 lanes: lanes without an instance fold nothing in
    const unsigned int bits = wave_or_u32(bad);
    if (bits) {   // (wave-uniform)
        const unsigned int first = wave_min_u32(bad ? (unsigned int)i : 0xFFFFFFFFu);
        const unsigned int count = wave_sum_u32(bad ? 1u : 0u);
        if ((threadIdx.x & 63) == 0) {
            atomicOr(&status[0], bits);
            atomicMin(&status[1], first);
            atomicAdd(&status[2], count);
        }
    }
}

int iu_check_args(const char* fn, int32_t numNodes, const void* nodeLocal, int32_t numInstances, const void* instanceNode, const void* blas,
                  const void* out, const void* status)
{
    if (!nodeLocal || !blas || !out || !status) return set_error(NTR_ERR_INVALID, "%s: null argument", fn);
    if (numInstances < 1 || numNodes < 1) return set_error(NTR_ERR_INVALID, "%s: numInstances < 1 or numNodes < 1", fn);
    if (!instanceNode && numNodes < numInstances)
        return set_error(NTR_ERR_INVALID, "%s: without instanceNode instance i uses node i: numNodes %d < numInstances %d", fn, (int)numNodes,
                         (int)numInstances);
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_instances_update(int32_t numNodes, const float* d_nodeLocal, const int32_t* d_nodeParent, int32_t numInstances,
                         const int32_t* d_instanceNode, const int32_t* d_blas, NtrInstance* d_instances, uint32_t* d_status,
                         NtrInstancesUpdateResult* result, void* stream)
{
    const char* fn = "ntr_instances_update";
    const auto wall0 = std::chrono::steady_clock::now();
    if (result) memset(result, 0, sizeof(*result));
    if (const int rc = iu_check_args(fn, numNodes, d_nodeLocal, numInstances, d_instanceNode, d_blas, d_instances, d_status)) return rc;
    if (((uintptr_t)d_nodeLocal | (uintptr_t)d_instances | (uintptr_t)d_status) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: d_nodeLocal, d_instances and d_status must be 16-byte aligned", fn);
    if (((uintptr_t)d_nodeParent | (uintptr_t)d_instanceNode | (uintptr_t)d_blas) & 3u)
        return set_error(NTR_ERR_INVALID, "%s: the index arrays must be 4-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));   // (no device: NTR_ERR_NO_DEVICE before any work)
    if (result && stream_is_capturing(s))
        return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);

    StreamEvents<2> ev(s);
    if (result) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
    }
    hipLaunchKernelGGL(iu_reset, dim3(1), dim3(64), 0, s, (uint4*)d_status);
    hipLaunchKernelGGL(iu_update, dim3((unsigned int)(((int64_t)numInstances + IU_BLOCK - 1) / IU_BLOCK)), dim3(IU_BLOCK), 0, s, (int)numNodes,
                       (const float4*)d_nodeLocal, (const int*)d_nodeParent, (int)numInstances, (const int*)d_instanceNode, (const int*)d_blas,
                       (uint4*)d_instances, (unsigned int*)d_status);
    NTR_HIP(hipGetLastError());
    if (!result) return NTR_OK;

    NTR_HIP(ev.record(1));
    uint32_t h[4] = {0u, 0u, 0u, 0u};
    NTR_HIP(hipMemcpyAsync(h, d_status, sizeof(h), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->numInstances = numInstances;
    result->numNodes = numNodes;
    result->statusBits = h[0];
    result->firstBad = h[1];
    result->numBad = h[2];
    result->updateMs = ms;
    result->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    if (h[0]) return set_error(NTR_ERR_INVALID, kInstanceBadFormat, fn, h[1], h[2], h[0]);
    return NTR_OK;
}

int ntr_instances_status_read(const uint32_t* d_status, uint32_t status[4], void* stream)
{
    const char* fn = "ntr_instances_status_read";
    if (status) memset(status, 0, 4 * sizeof(uint32_t));
    if (!d_status || !status || (((uintptr_t)d_status) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: null argument, or a status that is not 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads back and cannot be captured", fn);
    uint32_t h[4] = {0u, 0u, 0u, 0u};
    NTR_HIP(hipMemcpyAsync(h, d_status, sizeof(h), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    memcpy(status, h, sizeof(h));
    return NTR_OK;
}

}  // extern "C"
