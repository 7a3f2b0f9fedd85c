// ray_times_kernels.hip -- the times of a motion-blurred frame's rays, for gfx950 (ntr_ray_times_primary, ntr_ray_times_secondary;
// DESIGN.md 6ab).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_motion_frame.py (ray_times_primary, ray_times_secondary), and the header
// comment of ntr_ray_times_primary (include/ntrace_amd.h) states the contract.  ntr_trace_instanced_motion takes a time per ray and
// nothing made one:
//   primary     a hash of the ray's PIXEL id and the frame's seed, mapped into the shutter [open, close]: a thread per slot, one 4-byte
//               load of the slot-to-id table (none without one), one 4-byte store.  The id and not the slot is hashed, so
//               ntr_ray_morton_sort and the pixel table may reorder the rays without changing a pixel's time
//   secondary   output slot k * numSamples + j takes the word of input slot firstInputSlot + k -- ntr_raygen_ao_normals' slot rule: a
//               secondary ray sees its instance where its primary ray saw it.  A thread per output word, copied as an integer
// No scratch, no read-back, no atomics: both calls are capturable as they stand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"

namespace ntr {
namespace {

constexpr int RT_BLOCK = 256;

__global__ __launch_bounds__(RT_BLOCK) void ray_times_primary_kernel(int numRays, const int* __restrict__ slotToID, unsigned int seedTerm,
                                                                     float open, float close, float span, float* __restrict__ times)
{
    const unsigned int s = blockIdx.x * (unsigned int)RT_BLOCK + threadIdx.x;   // < 2^31 + RT_BLOCK
    if (s >= (unsigned int)numRays) return;
    unsigned int x = (unsigned int)(slotToID ? slotToID[s] : (int)s) + seedTerm;
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    const float u = (float)(x >> 8) * 0x1p-24f;   // exact: 24 bits, in [0, 1 - 2^-24]
    const float t = open + u * span;              // (the product rounded, then the sum: the library is built without contraction)
    times[s] = t < close ? t : close;
}

__global__ __launch_bounds__(RT_BLOCK) void ray_times_secondary_kernel(unsigned int numOut, unsigned int numSamples,
                                                                       const unsigned int* __restrict__ inTimes,
                                                                       unsigned int* __restrict__ outTimes)
{
    const unsigned int o = blockIdx.x * (unsigned int)RT_BLOCK + threadIdx.x;   // < 2^31 + RT_BLOCK
    if (o >= numOut) return;
    outTimes[o] = inTimes[o / numSamples];        // (inTimes starts at firstInputSlot; the word verbatim, a NaN included)
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_ray_times_primary(int32_t numRays, const int32_t* d_slotToID, uint32_t seed, float open, float close, float* d_times, void* stream)
{
    const char* fn = "ntr_ray_times_primary";
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    // (a NaN fails the comparisons, an infinity the bounds)
    if (!(open >= 0.0f && open <= close && close <= 1.0f))
        return set_error(NTR_ERR_INVALID, "%s: open and close must be finite with 0 <= open <= close <= 1", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_times) return set_error(NTR_ERR_INVALID, "%s: d_times is null", fn);
    if ((uintptr_t)d_times & 3u) return set_error(NTR_ERR_INVALID, "%s: d_times must be 4-byte aligned", fn);

    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    const float span = close - open;
    hipLaunchKernelGGL(ray_times_primary_kernel, dim3((unsigned int)(((long long)numRays + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0,
                       (hipStream_t)stream, (int)numRays, d_slotToID, (seed + 1u) * 0x9E3779B9u, open, close, span, d_times);
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

int ntr_ray_times_secondary(const float* d_inTimes, int32_t firstInputSlot, int32_t numInputRays, int32_t numSamples, float* d_outTimes,
                            void* stream)
{
    const char* fn = "ntr_ray_times_secondary";
    if (numInputRays < 0 || firstInputSlot < 0) return set_error(NTR_ERR_INVALID, "%s: negative count or slot", fn);
    if (numSamples < 1) return set_error(NTR_ERR_INVALID, "%s: numSamples < 1", fn);
    const long long numOut = (long long)numInputRays * numSamples;
    if (numOut >= (1ll << 31)) return set_error(NTR_ERR_INVALID, "%s: numInputRays * numSamples must be below 2^31", fn);
    if (numOut == 0) return NTR_OK;
    if (!d_inTimes || !d_outTimes) return set_error(NTR_ERR_INVALID, "%s: null buffer", fn);
    if (((uintptr_t)d_inTimes | (uintptr_t)d_outTimes) & 3u) return set_error(NTR_ERR_INVALID, "%s: d_inTimes and d_outTimes must be 4-byte aligned", fn);

    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    hipLaunchKernelGGL(ray_times_secondary_kernel, dim3((unsigned int)((numOut + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0,
                       (hipStream_t)stream, (unsigned int)numOut, (unsigned int)numSamples,
                       reinterpret_cast<const unsigned int*>(d_inTimes) + firstInputSlot, reinterpret_cast<unsigned int*>(d_outTimes));
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // extern "C"
