// tlas_wide_refit_kernels.hip -- in-place refit of a 4-wide top-level tree to moved instances for gfx950 (ntr_tlas_wide_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_wide_refit.py (refit_wide_tlas), and the header comment of ntr_tlas_wide_refit
// (include/ntrace_amd.h) states the contract.  ntr_tlas_widen blocks and reads extents back; a frame whose instances move, or whose wide
// BLASes were refitted (ntr_pool_wide_refit), only needs the wide records and the boxes again.  Two launches keep the topology and
// rewrite both:
//   tlw_prepare   one thread per index up to max(wide nodes, N): the topology step of wide_climb.h for wide node i, and wide record i
//                 of instance i (wide_write_record, instanced_wide_bvh.h: ntr_tlas_widen's record launch)
//   tlw_climb     one thread per slot: a leaf link ~i forms instance i's world box from the union of the root slots of its wide BLAS
//                 (tlr_world_box, tlas_world_box.h: the binary refit's function), publishes it and runs the climb of wide_climb.h
//   tlw_single    N == 1 has no node: record 0 and the scene box in one small launch
// The arrival protocol and its memory ordering are wide_climb.h's and are not restated.  A bad part is never followed: a link that names
// no wide node, a leaf link beyond the instances and an instance whose blas index names no BLAS are skipped, so their ancestors keep an
// arrival short and stay as they are; everything else is refitted completely.
// No host read-back unless a result is asked for, and no memset node on the asynchronous path: the first launch re-initialises the
// arrival counters, and the counters of the blocking form, which is never captured, are the one memset.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_wide_bvh.h"
#include "level_build.h"
#include "tlas_world_box.h"
#include "wide_climb.h"

namespace ntr {
namespace {

constexpr int TLW_BLOCK = 256;
enum : unsigned int { TLW_ERR_BLAS = 1u, TLW_ERR_LINK = 2u, TLW_ERR_LEAF = 4u };

// Counters of the blocking form, as tlas_refit_kernels.hip's; the scene box of the blocking form (6 floats, zero while the root has not
// been refitted) lies behind them.
constexpr int TLW_STAT_SLOTS = 256;
struct TlwStats {
    unsigned int innerLinks, leafLinks, err;
    unsigned int pad[13];        // a slot per 64-byte line
};
static_assert(sizeof(TlwStats) == 64, "TlwStats must be 64 bytes");

DeviceScratchPool g_tlwPool;

// The world box of instance i, whose blas index the caller has checked, from the current root of its wide BLAS: range.x is the wide
// BLAS's offset in the wide pool (the host has checked the range against the pool).  -> false: the root's count word lies outside 2..4
__device__ __forceinline__ bool tlw_instance_box(const NtrInstance* __restrict__ inst, int i, const uint4 range, const char* __restrict__ widePool,
                                                 float (&wlo)[3], float (&whi)[3])
{
    const float* root = (const float*)(widePool + range.x);
    const int count = ((const int*)root)[kWideCountWord];
    if (!wide_count_ok(count)) return false;
    float b[6];
#pragma unroll
    for (int j = 0; j < 6; j++) b[j] = root[wide_box_word(0, j)];
    for (int s = 1; s < count; s++) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            b[2 * q] = ord_min(b[2 * q], root[wide_box_word(s, 2 * q)]);
            b[2 * q + 1] = ord_max(b[2 * q + 1], root[wide_box_word(s, 2 * q + 1)]);
        }
    }
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = inst[i].objectToWorld[k];
    // the object box as a binary node 0 both of whose children hold it
    const float4 n01 = make_float4(b[0], b[1], b[2], b[3]), nz = make_float4(b[4], b[5], b[4], b[5]);
    tlr_world_box(n01, n01, nz, m, wlo, whi);
    return true;
}

__global__ __launch_bounds__(TLW_BLOCK) void tlw_prepare(int n, int numNodes, const NtrInstance* __restrict__ inst, int numBlas,
                                                         const uint4* __restrict__ table, const int* __restrict__ nodes,
                                                         uint4* __restrict__ records, unsigned int* __restrict__ parent,
                                                         unsigned int* __restrict__ arrive, TlwStats* __restrict__ stats /* or null */)
{
    const int idx = blockIdx.x * TLW_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0;
    if (idx < numNodes) {
        int kind[kWideChildren];
        if (!wide_topology_node(idx, numNodes, nodes, parent, arrive, kind)) err |= TLW_ERR_LINK;
#pragma unroll
        for (int k = 0; k < kWideChildren; k++) {
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= TLW_ERR_LINK;
            if (kind[k] == LINK_LEAF) {
                leaf += 1u;
                if (leaf_row(nodes[(size_t)idx * kWideWords + kWideLinkWord + k]) >= n) err |= TLW_ERR_LEAF;
            }
        }
    }
    if (idx < n) {
        const int b = inst[idx].blas;
        if (b < 0 || b >= numBlas) err |= TLW_ERR_BLAS;
        wide_write_record(inst, idx, numBlas, table, records);   // (with the empty extent for such an instance)
    }
    if (!stats) return;
    stats += blockIdx.x % TLW_STAT_SLOTS;
    // one add per wave and counter
    inner = wave_sum_u32(inner);
    leaf = wave_sum_u32(leaf);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (inner) atomicAdd(&stats->innerLinks, inner);
        if (leaf) atomicAdd(&stats->leafLinks, leaf);
        if (err) atomicOr(&stats->err, err);
    }
}

__global__ __launch_bounds__(TLW_BLOCK) void tlw_climb(int n, int numNodes, const NtrInstance* __restrict__ inst, int numBlas,
                                                       const uint4* __restrict__ table, const char* __restrict__ widePool, int* nodes,
                                                       const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                       float* sceneBox /* or null */, float* sceneCopy /* or null: the blocking form's */,
                                                       TlwStats* __restrict__ stats /* or null */)
{
    const unsigned int gid = blockIdx.x * (unsigned int)TLW_BLOCK + threadIdx.x;   // < 4 * numNodes + TLW_BLOCK < 2^27
    const int node = (int)(gid >> 2), k = (int)(gid & 3u);
    if (node >= numNodes) return;
    const int count = nodes[(size_t)node * kWideWords + kWideCountWord];
    if (!wide_count_ok(count) || k >= count) return;   // a node with a bad count word has no slots (the first launch reported it)
    const int link = nodes[(size_t)node * kWideWords + kWideLinkWord + k];
    if (link > 0) {                              // an inner slot arrives with the owner of its node
        // a node named by two links: one namer's parent word was overwritten, and that namer says so
        if (stats && is_wide_link(link, numNodes) && !wide_names_child(parent, node, k, link))
            atomicOr(&stats[blockIdx.x % TLW_STAT_SLOTS].err, TLW_ERR_LINK);
        return;
    }
    if (link < 0) {                              // (an empty slot keeps its box and only arrives)
        const int i = leaf_row(link);            // >= 0
        if (i >= n) return;                      // after a bad part the nodes above keep an arrival short and stay as they are
        const int b = inst[i].blas;
        if (b < 0 || b >= numBlas) return;
        float wlo[3], whi[3];
        if (!tlw_instance_box(inst, i, table[b], widePool, wlo, whi)) return;
        const float box[6] = {wlo[0], whi[0], wlo[1], whi[1], wlo[2], whi[2]};
        wide_publish_box(nodes, node, k, box);
    }
    wide_climb(node, numNodes, nodes, parent, arrive, sceneBox, sceneCopy);
}

// N == 1: one thread
__global__ __launch_bounds__(64) void tlw_single(const NtrInstance* __restrict__ inst, int numBlas, const uint4* __restrict__ table,
                                                 const char* __restrict__ widePool, uint4* __restrict__ records, float* sceneBox /* or null */,
                                                 float* sceneCopy /* or null */, TlwStats* __restrict__ stats /* or null */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    wide_write_record(inst, 0, numBlas, table, records);
    const int b = inst[0].blas;
    if (b < 0 || b >= numBlas) {
        if (stats) stats->err = TLW_ERR_BLAS;
        return;
    }
    float wlo[3], whi[3];
    if (!tlw_instance_box(inst, 0, table[b], widePool, wlo, whi)) return;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (sceneBox) { sceneBox[q] = wlo[q]; sceneBox[3 + q] = whi[q]; }
        if (sceneCopy) { sceneCopy[q] = wlo[q]; sceneCopy[3 + q] = whi[q]; }
    }
}

struct TlwLayout {
    size_t stats, scene, zeroBytes, table, parent, arrive, end;
    TlwLayout(int64_t nodes, int64_t numBlas)
    {
        ScratchCarver c;
        stats = c.take(sizeof(TlwStats) * TLW_STAT_SLOTS);   // one zeroed block: the counters and the blocking form's scene box
        scene = c.take(6 * sizeof(float));
        zeroBytes = c.off;
        table = c.take((size_t)numBlas * 16);
        parent = c.take((size_t)nodes * 4);
        arrive = c.take((size_t)nodes * 4);
        end = c.off;
    }
};

// What the device's range table holds, per device: the table the last uncaptured call uploaded and that call's counts.  valid is
// cleared whenever the pool has been released or has to grow, so a table on the host never vouches for bytes that are gone.
struct TlwUploaded {
    bool valid = false;
    int instances = 0, nodes = 0;
    std::vector<uint32_t> table;
};
TlwUploaded g_tlwUploaded[kMaxDevices];

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_tlas_wide_refit(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                        const NtrWideBlasRange* wideRanges, const void* d_widePoolNodes, int64_t widePoolNodesBytes, void* d_wideTlasNodes,
                        int64_t wideTlasNodesBytes, int32_t rootLink, void* d_wideRecords, int64_t recordsCapacity, float* d_sceneBox,
                        NtrTlasRefitResult* result, void* stream)
{
    const char* fn = "ntr_tlas_wide_refit";
    if (result) memset(result, 0, sizeof(*result));
    if (numInstances < 1 || (int64_t)numInstances * kRecordBytes > kPoolMaxBytes || numBlas < 1 || !d_instances || !blasRanges || !wideRanges ||
        !d_widePoolNodes || !d_wideRecords || (!d_wideTlasNodes && numInstances > 1))
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numInstances <= %lld, numBlas >= 1, non-null buffers)", fn,
                         (long long)(kPoolMaxBytes / kRecordBytes));
    const int n = numInstances;
    if (n == 1 ? wideTlasNodesBytes != 0 : check_wide_bytes(fn, wideTlasNodesBytes) != NTR_OK)
        return set_error(NTR_ERR_INVALID, "%s: wideTlasNodesBytes must be the extent ntr_tlas_widen reported: a multiple of 128 in [128, 0x%llx], "
                         "0 for one instance", fn, (unsigned long long)kMaxWideBytes);
    const int numNodes = (int)(wideTlasNodesBytes / kWideBytes);
    if (rootLink != (n == 1 ? leaf_link(0) : 0))
        return set_error(NTR_ERR_INVALID, "%s: rootLink must be 0, or ~0 for one instance, as ntr_tlas_build reported it", fn);
    if (recordsCapacity < (int64_t)kRecordBytes * n) return set_error(NTR_ERR_INVALID, "%s: recordsCapacity below 64 * numInstances", fn);
    if (((uintptr_t)d_widePoolNodes | (uintptr_t)d_wideRecords | (uintptr_t)d_wideTlasNodes | (uintptr_t)d_instances) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_wide_pool_bytes(fn, "widePoolNodesBytes", widePoolNodesBytes)) return rc;
    if (!wide_box_granules_aligned()) return set_error(NTR_ERR_INVALID, "%s: a wide box is not three aligned 8-byte granules", fn);
    std::vector<uint32_t> table(4 * (size_t)numBlas);
    for (int k = 0; k < numBlas; k++) {
        const NtrBlasRange& r = blasRanges[k];
        const NtrWideBlasRange& w = wideRanges[k];
        if (r.triWoopOffset < 0 || (r.triWoopOffset % kRowBytes) != 0 || r.triWoopOffset > kPoolMaxBytes - kRowBytes)
            return set_error(NTR_ERR_INVALID, "%s: BLAS %d: triWoopOffset must be a multiple of 16 inside a pool of at most 0x%llx bytes", fn, k,
                             (unsigned long long)kPoolMaxBytes);
        if (w.nodesOffset < 0 || (w.nodesOffset % kWideBytes) != 0 || w.nodesBytes < kWideBytes || (w.nodesBytes % kWideBytes) != 0 ||
            w.nodesBytes > kMaxWideBytes || w.nodesOffset > widePoolNodesBytes - w.nodesBytes)
            return set_error(NTR_ERR_INVALID, "%s: wide BLAS %d: offset and extent must be multiples of 128 inside the wide pool's %lld bytes", fn,
                             k, (long long)widePoolNodesBytes);
        table[4 * k] = (uint32_t)w.nodesOffset;
        table[4 * k + 1] = (uint32_t)(r.triWoopOffset / kRowBytes);
        table[4 * k + 2] = (uint32_t)w.nodesBytes;
        table[4 * k + 3] = 0u;
    }

    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
    const TlwLayout lay(numNodes, numBlas);
    TlwUploaded& up = g_tlwUploaded[dev];
    if (g_tlwPool.held() < lay.end) up.valid = false;   // released, never reserved, or about to be regrown
    const bool same = up.valid && up.table == table;
    const bool capturing = stream_is_capturing(s);
    if (capturing && result) return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);
    if (capturing && !(same && up.instances == n && up.nodes == numNodes))
        return set_error(NTR_ERR_INVALID, "%s: a captured call uploads and allocates nothing: the device must hold this range table already "
                         "-- make one uncaptured call with the same ranges, instance count and extent first (and none with others, and no "
                         "ntr_lbvh_release_workspace, between it and the capture)", fn);
    void* base = nullptr;
    if (const int rc = g_tlwPool.reserve(lay.end, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    if (!same) {
        // the host copy is what the upload reads and what the next call compares with: the upload is waited for, so the copy never
        // changes under it.  A frame loop over one pool pays this once
        up.valid = false;
        up.table.swap(table);
        NTR_HIP(hipMemcpyAsync(d_table, up.table.data(), up.table.size() * 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipStreamSynchronize(s));
        up.valid = true;
    }
    if (!capturing) { up.instances = n; up.nodes = numNodes; }
    TlwStats* stats = result ? at<TlwStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    StreamEvents<2> ev(s);
    if (result) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
        NTR_HIP(hipMemsetAsync(at<char>(base, 0), 0, lay.zeroBytes, s));
    }
    if (n == 1) {
        hipLaunchKernelGGL(tlw_single, dim3(1), dim3(64), 0, s, d_instances, (int)numBlas, (const uint4*)d_table, (const char*)d_widePoolNodes,
                           (uint4*)d_wideRecords, d_sceneBox, sceneCopy, stats);
    } else {
        const int threads = std::max(n, numNodes);
        hipLaunchKernelGGL(tlw_prepare, dim3((threads + TLW_BLOCK - 1) / TLW_BLOCK), dim3(TLW_BLOCK), 0, s, n, numNodes, d_instances, (int)numBlas,
                           (const uint4*)d_table, (const int*)d_wideTlasNodes, (uint4*)d_wideRecords, parent, arrive, stats);
        hipLaunchKernelGGL(tlw_climb, dim3((unsigned int)((4ll * numNodes + TLW_BLOCK - 1) / TLW_BLOCK)), dim3(TLW_BLOCK), 0, s, n, numNodes,
                           d_instances, (int)numBlas, (const uint4*)d_table, (const char*)d_widePoolNodes, (int*)d_wideTlasNodes,
                           (const unsigned int*)parent, arrive, d_sceneBox, sceneCopy, stats);
    }
    NTR_HIP(hipGetLastError());
    if (!result) return NTR_OK;

    NTR_HIP(ev.record(1));
    std::vector<char> host(lay.zeroBytes);       // the copy is waited for right here
    NTR_HIP(hipMemcpyAsync(host.data(), at<char>(base, 0), lay.zeroBytes, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    uint64_t inner = 0, leafLinks = 0;
    unsigned int err = 0;
    const TlwStats* hs = (const TlwStats*)(host.data() + lay.stats);
    for (int k = 0; k < TLW_STAT_SLOTS; k++) { inner += hs[k].innerLinks; leafLinks += hs[k].leafLinks; err |= hs[k].err; }
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    result->numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    result->errBits = (int32_t)err;
    memcpy(result->sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(result->sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    result->seconds = ms * 1e-3f;
    if (err & TLW_ERR_BLAS)
        return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d) (error bits 0x%x); its record has the empty extent, "
                         "its leaf box and the boxes above it were left as they were, everything else was refitted", fn, (int)numBlas, err);
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed wide top-level tree (error bits 0x%x: 2 a link that names no wide node, a node named "
                         "twice or a count word outside 2..4, 4 a leaf link beyond the instances); the boxes above such a place were left as "
                         "they were, everything else was refitted", fn, err);
    return NTR_OK;
}

int ntr_tlas_wide_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_wide_refit_scratch_bytes", g_tlwPool, bytes); }

}  // extern "C"
