// tlas_wide_refit_parts.h -- what the two in-place refits of a 4-wide top-level tree share, stated once
// (tlas_wide_refit_kernels.hip, tlas_wide_motion_refit_kernels.hip): the argument checks and the range table of
// ntr_tlas_wide_refit and ntr_tlas_wide_motion_refit, as tlas_refit_parts.h states them for the two binary refits, and on the device
// the object box of a wide BLAS.  Both units' kernels compile to the code they have with the statements in place
// (scripts/kernel_isa_diff.sh).  The device parts
// that all top-level refits share are tlas_refit_parts.h's, the climb is wide_climb.h's, the call's protocol refit_launch.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ntr_internal.h"
#include "device_prims.h"
#include "instanced_wide_bvh.h"
#include "wide_climb.h"

namespace ntr {

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// The object box (lo x, hi x, lo y, hi y, lo z, hi z) of the wide BLAS whose table entry is `range`: the union, in the integer order,
// of the slots of its root, which lies at range.x of the wide pool (the host has checked the range against the pool).  -> false: the
// root's count word lies outside 2..4
__device__ __forceinline__ bool tlw_root_box(const char* __restrict__ widePool, const uint4 range, float (&b)[6])
{
    const float* root = (const float*)(widePool + range.x);
    const int count = ((const int*)root)[kWideCountWord];
    if (!wide_count_ok(count)) return false;
#pragma unroll
    for (int j = 0; j < 6; j++) b[j] = root[wide_box_word(0, j)];
    for (int s = 1; s < count; s++) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            b[2 * q] = ord_min(b[2 * q], root[wide_box_word(s, 2 * q)]);
            b[2 * q + 1] = ord_max(b[2 * q + 1], root[wide_box_word(s, 2 * q + 1)]);
        }
    }
    return true;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// The arguments that ntr_tlas_wide_refit and ntr_tlas_wide_motion_refit share
struct TlasWideArgs {
    int32_t numInstances;
    const NtrInstance* d_instances;              // (key 0's)
    int32_t numBlas;
    const NtrBlasRange* blasRanges;
    const NtrWideBlasRange* wideRanges;
    const void* d_widePoolNodes;
    int64_t widePoolNodesBytes;
    void* d_wideTlasNodes;
    int64_t wideTlasNodesBytes;
    int32_t rootLink;
    void* d_wideRecords;
    int64_t recordsCapacity;
};

// The checks up to the records' capacity.  ownBuffers: the entry point's further buffers are all non-null
inline int tlas_wide_check_extents(const char* fn, const TlasWideArgs& a, bool ownBuffers = true)
{
    if (a.numInstances < 1 || (int64_t)a.numInstances * kRecordBytes > kPoolMaxBytes || a.numBlas < 1 || !a.d_instances || !ownBuffers ||
        !a.blasRanges || !a.wideRanges || !a.d_widePoolNodes || !a.d_wideRecords || (!a.d_wideTlasNodes && a.numInstances > 1))
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numInstances <= %lld, numBlas >= 1, non-null buffers)", fn,
                         (long long)(kPoolMaxBytes / kRecordBytes));
    const int n = a.numInstances;
    if (n == 1 ? a.wideTlasNodesBytes != 0 : check_wide_bytes(fn, a.wideTlasNodesBytes) != NTR_OK)
        return set_error(NTR_ERR_INVALID, "%s: wideTlasNodesBytes must be the extent ntr_tlas_widen reported: a multiple of 128 in [128, 0x%llx], "
                         "0 for one instance", fn, (unsigned long long)kMaxWideBytes);
    if (a.rootLink != (n == 1 ? leaf_link(0) : 0))
        return set_error(NTR_ERR_INVALID, "%s: rootLink must be 0, or ~0 for one instance, as ntr_tlas_build reported it", fn);
    if (a.recordsCapacity < (int64_t)kRecordBytes * n) return set_error(NTR_ERR_INVALID, "%s: recordsCapacity below 64 * numInstances", fn);
    return NTR_OK;
}

// The checks from the buffers' alignment on, and the device's range table: per BLAS the wide offset, triWoopOffset / 16, the wide
// extent, 0.  ownPointers: the entry point's further buffers, or-ed
inline int tlas_wide_range_table(const char* fn, const TlasWideArgs& a, uintptr_t ownPointers, std::vector<uint32_t>& table)
{
    if (((uintptr_t)a.d_widePoolNodes | (uintptr_t)a.d_wideRecords | (uintptr_t)a.d_wideTlasNodes | (uintptr_t)a.d_instances | ownPointers) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_wide_pool_bytes(fn, "widePoolNodesBytes", a.widePoolNodesBytes)) return rc;
    if (!wide_box_granules_aligned()) return set_error(NTR_ERR_INVALID, "%s: a wide box is not three aligned 8-byte granules", fn);
    table = std::vector<uint32_t>(4 * (size_t)a.numBlas);
    for (int k = 0; k < a.numBlas; k++) {
        const NtrBlasRange& r = a.blasRanges[k];
        const NtrWideBlasRange& w = a.wideRanges[k];
        if (r.triWoopOffset < 0 || (r.triWoopOffset % kRowBytes) != 0 || r.triWoopOffset > kPoolMaxBytes - kRowBytes)
            return set_error(NTR_ERR_INVALID, "%s: BLAS %d: triWoopOffset must be a multiple of 16 inside a pool of at most 0x%llx bytes", fn, k,
                             (unsigned long long)kPoolMaxBytes);
        if (w.nodesOffset < 0 || (w.nodesOffset % kWideBytes) != 0 || w.nodesBytes < kWideBytes || (w.nodesBytes % kWideBytes) != 0 ||
            w.nodesBytes > kMaxWideBytes || w.nodesOffset > a.widePoolNodesBytes - w.nodesBytes)
            return set_error(NTR_ERR_INVALID, "%s: wide BLAS %d: offset and extent must be multiples of 128 inside the wide pool's %lld bytes", fn,
                             k, (long long)a.widePoolNodesBytes);
        table[4 * k] = (uint32_t)w.nodesOffset;
        table[4 * k + 1] = (uint32_t)(r.triWoopOffset / kRowBytes);
        table[4 * k + 2] = (uint32_t)w.nodesBytes;
        table[4 * k + 3] = 0u;
    }
    return NTR_OK;
}

}  // namespace ntr
