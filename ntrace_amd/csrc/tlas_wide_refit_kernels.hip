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
// The error bits, the wave fold of the counters, the scene-box write and the scratch layout are tlas_refit_parts.h's; the held range
// table, the refusals of a captured call and the bracket of the blocking form are refit_launch.h's.  The 4-wide
// classification of tlw_prepare is this unit's own; the checks and the table (wide ranges beside the binary ones) are
// tlas_wide_refit_parts.h's, shared with tlas_wide_motion_refit_kernels.hip.
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
#include "refit_launch.h"
#include "tlas_refit_parts.h"
#include "tlas_wide_refit_parts.h"
#include "tlas_world_box.h"
#include "wide_climb.h"

namespace ntr {
namespace {

constexpr int TLW_BLOCK = 256;

// A counter slot of the blocking form (refit_launch.h), as tlas_refit_kernels.hip's
struct TlwStats {
    unsigned int innerLinks, leafLinks, err;
    unsigned int pad[13];        // a slot per 64-byte line
};
static_assert(sizeof(TlwStats) == 64, "TlwStats must be 64 bytes");

DeviceScratchPool g_tlwPool;
RefitHeld g_tlwHeld[kMaxDevices];

// The world box of instance i, whose blas index the caller has checked, from the current root of its wide BLAS: range.x is the wide
// BLAS's offset in the wide pool (the host has checked the range against the pool).  -> false: the root's count word lies outside 2..4
__device__ __forceinline__ bool tlw_instance_box(const NtrInstance* __restrict__ inst, int i, const uint4 range, const char* __restrict__ widePool,
                                                 float (&wlo)[3], float (&whi)[3])
{
    float b[6];
    if (!tlw_root_box(widePool, range, b)) return false;
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
        if (!wide_topology_node(idx, numNodes, nodes, parent, arrive, kind)) err |= TLAS_ERR_LINK;
#pragma unroll
        for (int k = 0; k < kWideChildren; k++) {
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= TLAS_ERR_LINK;
            if (kind[k] == LINK_LEAF) {
                leaf += 1u;
                if (leaf_row(nodes[(size_t)idx * kWideWords + kWideLinkWord + k]) >= n) err |= TLAS_ERR_LEAF;
            }
        }
    }
    if (idx < n) {
        const int b = inst[idx].blas;
        if (b < 0 || b >= numBlas) err |= TLAS_ERR_BLAS;
        wide_write_record(inst, idx, numBlas, table, records);   // (with the empty extent for such an instance)
    }
    if (!stats) return;
    stats += blockIdx.x % kRefitStatSlots;
    tlas_fold_counters(stats, inner, leaf, err);
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
            atomicOr(&stats[blockIdx.x % kRefitStatSlots].err, TLAS_ERR_LINK);
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
        if (stats) stats->err = TLAS_ERR_BLAS;
        return;
    }
    float wlo[3], whi[3];
    if (!tlw_instance_box(inst, 0, table[b], widePool, wlo, whi)) return;
    tlas_write_scene_box(sceneBox, sceneCopy, wlo, whi);
}

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
    const TlasWideArgs args = {numInstances, d_instances, numBlas, blasRanges, wideRanges, d_widePoolNodes, widePoolNodesBytes, d_wideTlasNodes,
                               wideTlasNodesBytes, rootLink, d_wideRecords, recordsCapacity};
    if (const int rc = tlas_wide_check_extents(fn, args)) return rc;
    const int n = numInstances, numNodes = (int)(wideTlasNodesBytes / kWideBytes);
    const TlasRefitLayout lay(numNodes, numBlas);
    RefitTable held = {1, {}, {lay.table, 0}, {n, numNodes}};
    if (const int rc = tlas_wide_range_table(fn, args, 0, held.words[0])) return rc;

    hipStream_t s = (hipStream_t)stream;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitRangeExtentWords, g_tlwPool, g_tlwHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    TlwStats* stats = result ? at<TlwStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, base, lay.zeroBytes, &host, &seconds, [&] {
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
    });
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0;
    unsigned int err = 0;
    refit_fold_slots<TlwStats>(host.data() + lay.stats, [&](const TlwStats& v) { inner += v.innerLinks; leafLinks += v.leafLinks; err |= v.err; });
    result->numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    result->numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    result->errBits = (int32_t)err;
    memcpy(result->sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(result->sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    result->seconds = seconds;
    if (err & TLAS_ERR_BLAS)
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
