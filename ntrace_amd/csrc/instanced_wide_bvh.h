// instanced_wide_bvh.h -- the two-level layout over 4-wide trees, stated once, for the code that widens a pool and a top-level tree
// (instanced_widen_kernels.hip) and the kernel that traverses them (trace_instanced_wide_kernels.hip).  It joins instanced_bvh.h (pool,
// top level, record, exit marker) and wide_bvh.h (the 128-byte node); the rule is tests/np_instanced_wide.py.
//   wide pool   ONE more node buffer beside the pool; the pool's triWoop and triIndex are used unchanged.  Wide BLAS k is byte for byte
//               what ntr_bvh_widen writes for binary BLAS k when handed pool + nodesOffset_k, and lies at the sum of the exact wide
//               extents (NtrBvhWideResult::nodesBytes) of the BLASes before it: every offset is a multiple of 128, there are no gaps, and
//               links stay relative to the BLAS's own start.  The buffer is at most kPoolMaxBytes long
//   wide TLAS   ntr_bvh_widen applied to the top-level node buffer; leaf links ~i pass through verbatim.  N == 1: no node, rootLink ~0
//   record i    16 words: 0..11 worldToObject, 12 the wide BLAS's offset in the wide pool, 13 triWoopOffset / 16 (as the binary record),
//               14 the wide BLAS's extent, 15 zero -- or, after ntr_tlas_wide_motion_refit (tlas_wide_motion_refit_kernels.hip), 1 for an
//               instance that moves within the shutter, as word 15 of the binary record (instanced_bvh.h, kRecMoving).  Only the wide
//               motion kernels (trace_instanced_wide_motion_kernels.hip) read word 15: every other wide trace kernel takes x, y, z of
//               the record's fourth row in its entering step and nothing else of it (trace_instanced_wide_body.h; the w that
//               wide_advance reads is a wide NODE's fourth link), ntr_instanced_wide_validate reads node buffers only, the attribute
//               kernels take no records, and the writers (wide_write_record below: ntr_tlas_widen, ntr_tlas_wide_refit) write 0 --
//               searched in csrc/ when the word was given its meaning.  An instance whose blas index lies outside
//               [0, numBlas) gets offset, row offset and extent 0: a lane inside an instance fetches a wide node only below the extent,
//               so nothing of such an instance is read
//   marker      kExitMarker, as in instanced_bvh.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "instanced_bvh.h"
#include "wide_bvh.h"

namespace ntr {

constexpr int kWideRecOffset = 12, kWideRecRowOffset = 13, kWideRecExtent = 14;
static_assert(kPoolMaxBytes % kWideBytes == 0, "a wide pool of the largest size is a whole number of wide nodes");

// Wide record i from the current instance i: table[b] is (wide offset, triWoopOffset / 16, wide extent, 0) of BLAS b.  For the record
// launch of ntr_tlas_widen and the prepare launch of ntr_tlas_wide_refit
__device__ __forceinline__ void wide_write_record(const NtrInstance* __restrict__ inst, int i, int numBlas, const uint4* __restrict__ table,
                                                  uint4* __restrict__ records)
{
    const int b = inst[i].blas;
    const uint4 range = (b >= 0 && b < numBlas) ? table[b] : make_uint4(0u, 0u, 0u, 0u);   // wide offset, row offset, wide extent, 0
    const uint32_t* inv = reinterpret_cast<const uint32_t*>(inst[i].worldToObject);
    uint4* rec = records + 4 * (size_t)i;
    rec[0] = make_uint4(inv[0], inv[1], inv[2], inv[3]);
    rec[1] = make_uint4(inv[4], inv[5], inv[6], inv[7]);
    rec[2] = make_uint4(inv[8], inv[9], inv[10], inv[11]);
    rec[3] = make_uint4(range.x, range.y, range.z, 0u);
}

// bvh_widen_kernels.hip: `bytes` of the widening pass's per-device scratch pool (the pass is blocking, so between two passes the pool
// is idle: the pool and TLAS widening keep their BLAS table there and add no pool of their own)
int widen_scratch_reserve(size_t bytes, void** out);

// A wide pool's size: a multiple of 128 in [128, kPoolMaxBytes]
inline int check_wide_pool_bytes(const char* fn, const char* what, int64_t bytes)
{
    if (bytes < kWideBytes || (bytes % kWideBytes) != 0 || bytes > kPoolMaxBytes)
        return set_error(NTR_ERR_INVALID, "%s: %s must be a multiple of 128 in [128, 0x%llx]", fn, what, (unsigned long long)kPoolMaxBytes);
    return NTR_OK;
}

}  // namespace ntr
