// instanced_widen_kernels.hip -- widening an instanced scene for gfx950 (ntr_pool_widen, ntr_tlas_widen): the pool's BLASes
// and the top-level tree through ntr_bvh_widen, and the wide instance records.  EXTENSION without a reference counterpart: the rule is
// the numpy spec tests/np_instanced_wide.py; instanced_wide_bvh.h states the layout.
//   ntr_pool_widen   a host loop of ntr_bvh_widen, BLAS k at the sum of the exact extents before it.  Not batched: every BLAS pays the
//                    pass's launches and read-backs (DESIGN.md 6r has what that costs for 1 024 BLASes).  The batched pass is
//                    ntr_pool_widen_batch (pool_widen_batch_kernels.hip), which writes the same bytes
//   ntr_tlas_widen   ntr_bvh_widen on the top-level nodes (none for one instance), then iw_records: a thread per instance copies
//                    worldToObject and looks its BLAS up in a table of (wide offset, row offset, wide extent) -- zeros for a blas index
//                    outside the table.  The table lives in the widening pass's scratch pool, which is idle once the pass has returned
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "device_scratch.h"

namespace ntr {
namespace {

constexpr int IW_BLOCK = 256;

__global__ __launch_bounds__(IW_BLOCK) void iw_records(int n, const NtrInstance* __restrict__ inst, int numBlas, const uint4* __restrict__ table,
                                                       uint4* __restrict__ records)
{
    const int i = blockIdx.x * IW_BLOCK + threadIdx.x;
    if (i >= n) return;
    wide_write_record(inst, i, numBlas, table, records);
}

bool iw_ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bn && b0 < a0 + (uintptr_t)an;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_pool_widen_capacity(int32_t numBlas, const NtrBlasRange* blasRanges, int64_t* widePoolNodesBytes)
{
    const char* fn = "ntr_pool_widen_capacity";
    if (!widePoolNodesBytes) return set_error(NTR_ERR_INVALID, "%s: null", fn);
    *widePoolNodesBytes = 0;
    if (numBlas < 1 || !blasRanges) return set_error(NTR_ERR_INVALID, "%s: no BLAS ranges", fn);
    int64_t sum = 0;
    for (int k = 0; k < numBlas; k++) {
        int64_t cap = 0;
        if (const int rc = ntr_bvh_widen_capacity(blasRanges[k].nodesBytes, &cap)) return rc;
        sum += cap;
    }
    *widePoolNodesBytes = sum;
    return NTR_OK;
}

int ntr_pool_widen(int32_t numBlas, const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes, void* d_widePoolNodes,
                   int64_t capacity, NtrWideBlasRange* wideRanges, NtrBvhWideResult* result, void* stream)
{
    const char* fn = "ntr_pool_widen";
    if (result) memset(result, 0, sizeof(*result));
    if (numBlas < 1 || !blasRanges || !wideRanges) return set_error(NTR_ERR_INVALID, "%s: no BLAS ranges", fn);
    memset(wideRanges, 0, sizeof(NtrWideBlasRange) * (size_t)numBlas);
    if (!d_poolNodes || !d_widePoolNodes || !result) return set_error(NTR_ERR_INVALID, "%s: null buffer or result", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    int64_t need = 0;
    for (int k = 0; k < numBlas; k++) {
        if (const int rc = check_blas_range(fn, k, blasRanges[k], poolNodesBytes)) return rc;
        int64_t cap = 0;
        if (const int rc = ntr_bvh_widen_capacity(blasRanges[k].nodesBytes, &cap)) return rc;
        need += cap;
    }
    if (capacity < need) return set_error(NTR_ERR_INVALID, "%s: capacity is below ntr_pool_widen_capacity()", fn);
    if (iw_ranges_overlap(d_widePoolNodes, capacity, d_poolNodes, poolNodesBytes))
        return set_error(NTR_ERR_INVALID, "%s: d_widePoolNodes overlaps d_poolNodes (the pass is out of place)", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads extents back and cannot be captured", fn);

    int layoutRc = NTR_OK;
    int64_t off = 0;
    NtrBvhWideResult sum;
    memset(&sum, 0, sizeof(sum));
    for (int k = 0; k < numBlas; k++) {
        const NtrBlasRange& r = blasRanges[k];
        // BLAS k's bound fits behind `off`: off is the sum of extents, each at most its BLAS's bound, and capacity >= the sum of bounds
        NtrBvhWideResult one;
        const int rc = ntr_bvh_widen((const char*)d_poolNodes + r.nodesOffset, r.nodesBytes, (char*)d_widePoolNodes + off, capacity - off, &one, s);
        if (rc == NTR_ERR_LAYOUT) layoutRc = rc;   // the tree is complete and `one` describes it: the loop goes on
        else if (rc != NTR_OK) { memset(wideRanges, 0, sizeof(NtrWideBlasRange) * (size_t)numBlas); return rc; }
        wideRanges[k].nodesOffset = off; wideRanges[k].nodesBytes = one.nodesBytes;
        wideRanges[k].numNodes = one.numNodes; wideRanges[k].stackBound = one.stackBound;
        off += one.nodesBytes;
        if (off > kPoolMaxBytes) {
            memset(wideRanges, 0, sizeof(NtrWideBlasRange) * (size_t)numBlas);
            return set_error(NTR_ERR_OVERFLOW, "%s: the wide pool exceeds 0x%llx bytes at BLAS %d", fn, (unsigned long long)kPoolMaxBytes, k);
        }
        sum.numNodes += one.numNodes;
        for (int c = 0; c < 3; c++) sum.counts[c] += one.counts[c];
        sum.numLeafLinks += one.numLeafLinks;
        sum.height = one.height > sum.height ? one.height : sum.height;
        sum.stackBound = one.stackBound > sum.stackBound ? one.stackBound : sum.stackBound;
        sum.seconds += one.seconds;
    }
    sum.nodesBytes = off;
    *result = sum;
    return layoutRc;   // (ntr_bvh_widen's message of the last such BLAS stands)
}

int ntr_tlas_widen(int32_t numInstances, const NtrInstance* d_instances, const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                   int32_t numBlas, const NtrBlasRange* blasRanges, const NtrWideBlasRange* wideRanges, void* d_wideTlasNodes, int64_t capacity,
                   void* d_wideRecords, int64_t recordsCapacity, NtrTlasWideResult* result, void* stream)
{
    const char* fn = "ntr_tlas_widen";
    if (result) memset(result, 0, sizeof(*result));
    if (numInstances < 1 || (int64_t)numInstances * kRecordBytes > kPoolMaxBytes) return set_error(NTR_ERR_INVALID, "%s: numInstances out of range", fn);
    if (!d_instances || !d_wideRecords || !result) return set_error(NTR_ERR_INVALID, "%s: null buffer or result", fn);
    if ((((uintptr_t)d_instances) | ((uintptr_t)d_wideRecords) | ((uintptr_t)d_wideTlasNodes) | ((uintptr_t)d_tlasNodes)) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_root_link(fn, rootLink, numInstances)) return rc;
    if (rootLink == 0) {
        if (!d_tlasNodes || !d_wideTlasNodes) return set_error(NTR_ERR_INVALID, "%s: null top-level buffer", fn);
        if (const int rc = check_nodes_bytes(fn, "tlasNodesBytes", tlasNodesBytes)) return rc;
        int64_t need = 0;
        if (const int rc = ntr_bvh_widen_capacity(tlasNodesBytes, &need)) return rc;
        if (capacity < need)
            return set_error(NTR_ERR_INVALID, "%s: capacity is below ntr_bvh_widen_capacity()", fn);
    }
    if (recordsCapacity < (int64_t)numInstances * kRecordBytes) return set_error(NTR_ERR_INVALID, "%s: recordsCapacity is below 64 * numInstances", fn);
    if (numBlas < 1 || !blasRanges || !wideRanges) return set_error(NTR_ERR_INVALID, "%s: no BLAS ranges", fn);
    int32_t poolBound = 0;
    for (int k = 0; k < numBlas; k++) {
        const NtrBlasRange& r = blasRanges[k];
        const NtrWideBlasRange& w = wideRanges[k];
        if (r.triWoopOffset < 0 || (r.triWoopOffset % kRowBytes) != 0 || r.triWoopOffset > kPoolMaxBytes - kRowBytes)
            return set_error(NTR_ERR_INVALID, "%s: BLAS %d: triWoopOffset must be a multiple of 16 inside a pool of at most 0x%llx bytes", fn, k,
                             (unsigned long long)kPoolMaxBytes);
        if (w.nodesOffset < 0 || (w.nodesOffset % kWideBytes) != 0 || w.nodesBytes < kWideBytes || (w.nodesBytes % kWideBytes) != 0 ||
            w.nodesBytes > kMaxWideBytes || w.nodesOffset > kPoolMaxBytes - w.nodesBytes || w.stackBound < 0)
            return set_error(NTR_ERR_INVALID, "%s: wide BLAS %d: offset and extent must be multiples of 128 inside a pool of at most 0x%llx bytes",
                             fn, k, (unsigned long long)kPoolMaxBytes);
        poolBound = w.stackBound > poolBound ? w.stackBound : poolBound;
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads extents back and cannot be captured", fn);

    int layoutRc = NTR_OK;
    NtrBvhWideResult top;
    memset(&top, 0, sizeof(top));
    if (rootLink == 0) {
        const int rc = ntr_bvh_widen(d_tlasNodes, tlasNodesBytes, d_wideTlasNodes, capacity, &top, s);
        if (rc == NTR_ERR_LAYOUT) layoutRc = rc;
        else if (rc != NTR_OK) return rc;
    }
    // the table, in the pass's own pool (idle: the pass has returned).  One uint4 per BLAS
    std::vector<uint4> table((size_t)numBlas);
    for (int k = 0; k < numBlas; k++)
        table[(size_t)k] = make_uint4((uint32_t)wideRanges[k].nodesOffset, (uint32_t)(blasRanges[k].triWoopOffset / kRowBytes),
                                      (uint32_t)wideRanges[k].nodesBytes, 0u);
    void* d_table = nullptr;
    if (const int rc = widen_scratch_reserve(table.size() * sizeof(uint4), &d_table)) return rc;
    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(uint4), hipMemcpyHostToDevice, s));
    NTR_HIP(ev.record(0));
    hipLaunchKernelGGL(iw_records, dim3((unsigned int)((numInstances + IW_BLOCK - 1) / IW_BLOCK)), dim3(IW_BLOCK), 0, s, (int)numInstances,
                       d_instances, (int)numBlas, (const uint4*)d_table, (uint4*)d_wideRecords);
    NTR_HIP(hipGetLastError());
    NTR_HIP(ev.record(1));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->nodesBytes = top.nodesBytes;
    result->recordsBytes = (int64_t)numInstances * kRecordBytes;
    result->numNodes = top.numNodes;
    for (int c = 0; c < 3; c++) result->counts[c] = top.counts[c];
    result->numLeafLinks = top.numLeafLinks;
    result->height = top.height;
    result->tlasStackBound = top.stackBound;
    result->stackBound = top.stackBound + 1 + poolBound;
    result->seconds = top.seconds + ms * 1e-3f;
    return layoutRc;
}

}  // extern "C"
