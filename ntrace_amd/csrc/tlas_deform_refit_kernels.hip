// tlas_deform_refit_kernels.hip -- on-device refit of a top-level tree to instances that move within the shutter AND whose BLASes may
// deform within it, for gfx950 (ntr_tlas_deform_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_deform.py (deform_refit), and the header comment of ntr_tlas_deform_refit
// (include/ntrace_amd.h) states the contract.  It is tlas_motion_refit_kernels.hip's refit with the pool's second node buffer and a
// device-resident flag per BLAS, two changes and the same two launches:
//   tdr_prepare   as tmr_prepare; word 15 of record i is bit 0 "moving" | bit 1 "the instance's BLAS deforms" (d_blasDeforming[blas],
//                 read here, so a replay sees the current flags)
//   tdr_climb     a leaf link ~i forms instance i's world box (tlr_world_box of tlas_world_box.h) over ALL pairs of {key 0's transform,
//                 and key 1's where the instance moves} x {node 0 of the BLAS in poolNodes, and in poolNodes1 where the BLAS deforms}:
//                 up to four boxes, united in the integer order, then the climb of bvh_climb.h
//   tdr_single    N == 1 has no node: record 0, key entry 0 and the scene box in one small launch
// Why four boxes: a posed point is M(t) c(t) with both factors linear in t, a quadratic Bezier curve with the control points M0 c0,
// (M0 c1 + M1 c0) / 2 and M1 c1; it lies in the hull of the four products, not in the hull of its two ends.  No padding.
// With no flag set every byte written is ntr_tlas_motion_refit's.  The arrival protocol is bvh_climb.h's; the error bits, the load of
// node 0, the leaf's climb, the scene-box write, the scratch layout, the argument checks and the range table are tlas_refit_parts.h's;
// the held range table, the refusals of a captured call and the bracket of the blocking form are refit_launch.h's.  The key loads, the
// comparison, the key entry and the record are tlas_motion_refit_kernels.hip's statements a second time: shared, that unit's kernels
// would have to be shown unchanged (scripts/kernel_isa_diff.sh), and they are a dozen lines.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_bvh.h"
#include "level_build.h"
#include "refit_launch.h"
#include "tlas_refit_parts.h"
#include "tlas_world_box.h"

namespace ntr {
namespace {

constexpr int TDR_BLOCK = 256;

// A counter slot of the blocking form (refit_launch.h): the motion refit's counters and the instances of deforming BLASes
struct TdrStats {
    unsigned int innerLinks, leafLinks, err, moving, deforming;
    unsigned int pad[11];        // a slot per 64-byte line
};
static_assert(sizeof(TdrStats) == 64, "TdrStats must be 64 bytes");

DeviceScratchPool g_tdrPool;
RefitHeld g_tdrHeld[kMaxDevices];

// objectToWorld of instance i: 48 bytes at the start of a 112-byte struct of a 16-byte aligned array
__device__ __forceinline__ void tdr_load_key(const NtrInstance* __restrict__ inst, int i, uint4 (&m)[3])
{
    const uint4* src = reinterpret_cast<const uint4*>(inst[i].objectToWorld);
    m[0] = src[0]; m[1] = src[1]; m[2] = src[2];
}

__device__ __forceinline__ bool tdr_differs(const uint4 (&a)[3], const uint4 (&b)[3])
{
    unsigned int d = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) d |= (a[k].x ^ b[k].x) | (a[k].y ^ b[k].y) | (a[k].z ^ b[k].z) | (a[k].w ^ b[k].w);
    return d != 0u;
}

// Motion key entry i (instanced_bvh.h), whatever instance i's blas index is.  -> the instance moves
__device__ __forceinline__ bool tdr_write_key(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                              uint4* __restrict__ keys)
{
    uint4 a[3], b[3];
    tdr_load_key(inst0, i, a);
    tdr_load_key(inst1, i, b);
    uint4* e = keys + (kMotionKeyBytes / 16) * (size_t)i;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    e[0] = a[0]; e[1] = a[1]; e[2] = a[2]; e[3] = zero;
    e[4] = b[0]; e[5] = b[1]; e[6] = b[2]; e[7] = zero;
    return tdr_differs(a, b);
}

// Record i of key-0 instance i, whose blas index the caller has checked; range is the table's entry of its BLAS
__device__ __forceinline__ void tdr_write_record(const NtrInstance* __restrict__ inst0, int i, const uint4 range, bool moving, bool deforming,
                                                 uint4* __restrict__ records)
{
    const uint4* inv = reinterpret_cast<const uint4*>(inst0[i].worldToObject);
    uint4* rec = records + 4 * (size_t)i;
    rec[0] = inv[0];
    rec[1] = inv[1];
    rec[2] = inv[2];
    rec[3] = make_uint4(range.x, range.y, range.z, (moving ? 1u : 0u) | (deforming ? 2u : 0u));
}

__device__ __forceinline__ void tdr_matrix(const uint4 (&k)[3], float (&m)[12])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        m[4 * r] = __uint_as_float(k[r].x); m[4 * r + 1] = __uint_as_float(k[r].y);
        m[4 * r + 2] = __uint_as_float(k[r].z); m[4 * r + 3] = __uint_as_float(k[r].w);
    }
}

// [wlo, whi] united, in the integer order, with the world box of node 0 (n0, n1, nz) under m
__device__ __forceinline__ void tdr_unite(const float4& n0, const float4& n1, const float4& nz, const float (&m)[12], float (&wlo)[3],
                                          float (&whi)[3])
{
    float lo1[3], hi1[3];
    tlr_world_box(n0, n1, nz, m, lo1, hi1);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        wlo[q] = ord_min(wlo[q], lo1[q]);
        whi[q] = ord_max(whi[q], hi1[q]);
    }
}

// The swept world box of instance i, whose blas index the caller has checked: the union over {key 0, key 1 where it moves} x {the BLAS's
// node 0 in poolNodes, and in poolNodes1 where the BLAS deforms}.  range.x lies inside both buffers (the host has checked it against
// poolNodesBytes, the extent of either)
__device__ __forceinline__ void tdr_instance_box(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                                 const uint4 range, const char* __restrict__ poolNodes, const char* __restrict__ poolNodes1,
                                                 bool deforming, float (&wlo)[3], float (&whi)[3])
{
    float4 n0, n1, nz;
    tlas_load_node0(poolNodes, range, n0, n1, nz);
    uint4 a[3], b[3];
    tdr_load_key(inst0, i, a);
    tdr_load_key(inst1, i, b);
    const bool moving = tdr_differs(a, b);
    float m0[12], m1[12];
    tdr_matrix(a, m0);
    tdr_matrix(b, m1);
    tlr_world_box(n0, n1, nz, m0, wlo, whi);
    if (moving) tdr_unite(n0, n1, nz, m1, wlo, whi);
    if (!deforming) return;
    tlas_load_node0(poolNodes1, range, n0, n1, nz);
    tdr_unite(n0, n1, nz, m0, wlo, whi);
    if (moving) tdr_unite(n0, n1, nz, m1, wlo, whi);
}

__global__ __launch_bounds__(TDR_BLOCK) void tdr_prepare(int n, int numSlots, const NtrInstance* __restrict__ inst0,
                                                         const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                         const unsigned int* __restrict__ blasDeforming, const int* __restrict__ nodes,
                                                         uint4* __restrict__ records, uint4* __restrict__ keys,
                                                         unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                         TdrStats* __restrict__ stats /* or null */)
{
    const int idx = blockIdx.x * TDR_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0, moving = 0, deforming = 0;
    if (idx < numSlots) {
        int kind[2];
        topology_slot(idx, numSlots, nodes, parent, arrive, kind);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= TLAS_ERR_LINK;
            if (kind[k] == LINK_LEAF) {
                leaf += 1u;
                if (leaf_row(nodes[(size_t)idx * kNodeWords + kLinkWord + k]) >= n) err |= TLAS_ERR_LEAF;
            }
        }
    }
    if (idx < n) {
        const bool mv = tdr_write_key(inst0, inst1, idx, keys);
        moving = mv ? 1u : 0u;
        const int b = inst0[idx].blas;
        if (b < 0 || b >= numBlas) err |= TLAS_ERR_BLAS;
        else {
            const bool df = blasDeforming[b] != 0u;
            deforming = df ? 1u : 0u;
            tdr_write_record(inst0, idx, table[b], mv, df, records);
        }
    }
    if (!stats) return;
    stats += blockIdx.x % kRefitStatSlots;
    inner = wave_sum_u32(inner);
    leaf = wave_sum_u32(leaf);
    moving = wave_sum_u32(moving);
    deforming = wave_sum_u32(deforming);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (inner) atomicAdd(&stats->innerLinks, inner);
        if (leaf) atomicAdd(&stats->leafLinks, leaf);
        if (moving) atomicAdd(&stats->moving, moving);
        if (deforming) atomicAdd(&stats->deforming, deforming);
        if (err) atomicOr(&stats->err, err);
    }
}

__global__ __launch_bounds__(TDR_BLOCK) void tdr_climb(int n, int numSlots, const NtrInstance* __restrict__ inst0,
                                                       const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                       const unsigned int* __restrict__ blasDeforming, const char* __restrict__ poolNodes,
                                                       const char* __restrict__ poolNodes1, int* nodes, const unsigned int* __restrict__ parent,
                                                       unsigned int* __restrict__ arrive, float* sceneBox /* or null */,
                                                       float* sceneCopy /* or null: the blocking form's */)
{
    const unsigned int gid = blockIdx.x * (unsigned int)TDR_BLOCK + threadIdx.x;   // < 2 * numSlots + TDR_BLOCK < 2^26
    const int node = (int)(gid >> 1), k = (int)(gid & 1u);
    if (node >= numSlots) return;
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (link >= 0) return;                       // an inner child arrives with the owner of its node; offset 0 is no child at all
    const int i = leaf_row(link);                // >= 0
    if (i >= n) return;                          // after a bad part the nodes above keep an arrival short and stay as they are
    const int b = inst0[i].blas;
    if (b < 0 || b >= numBlas) return;
    float wlo[3], whi[3];
    tdr_instance_box(inst0, inst1, i, table[b], poolNodes, poolNodes1, blasDeforming[b] != 0u, wlo, whi);
    tlas_leaf_climb(node, k, numSlots, nodes, parent, arrive, wlo, whi, sceneBox, sceneCopy);
}

// N == 1: one thread
__global__ __launch_bounds__(64) void tdr_single(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int numBlas,
                                                 const uint4* __restrict__ table, const unsigned int* __restrict__ blasDeforming,
                                                 const char* __restrict__ poolNodes, const char* __restrict__ poolNodes1,
                                                 uint4* __restrict__ records, uint4* __restrict__ keys, float* sceneBox /* or null */,
                                                 float* sceneCopy /* or null */, TdrStats* __restrict__ stats /* or null */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool mv = tdr_write_key(inst0, inst1, 0, keys);
    if (stats) stats->moving = mv ? 1u : 0u;
    const int b = inst0[0].blas;
    if (b < 0 || b >= numBlas) {
        if (stats) stats->err = TLAS_ERR_BLAS;
        return;
    }
    const uint4 range = table[b];
    const bool df = blasDeforming[b] != 0u;
    if (stats) stats->deforming = df ? 1u : 0u;
    tdr_write_record(inst0, 0, range, mv, df, records);
    float wlo[3], whi[3];
    tdr_instance_box(inst0, inst1, 0, range, poolNodes, poolNodes1, df, wlo, whi);
    tlas_write_scene_box(sceneBox, sceneCopy, wlo, whi);
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_tlas_deform_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1, int32_t numBlas,
                          const NtrBlasRange* blasRanges, const void* d_poolNodes, const void* d_poolNodes1, int64_t poolNodesBytes,
                          const uint32_t* d_blasDeforming, void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, void* d_records,
                          int64_t recordsCapacity, void* d_motionKeys, int64_t motionKeysCapacity, float* d_sceneBox,
                          NtrTlasDeformRefitResult* result, void* stream)
{
    const char* fn = "ntr_tlas_deform_refit";
    if (result) memset(result, 0, sizeof(*result));
    const TlasBinaryArgs args = {numInstances, d_instances0, numBlas, blasRanges, d_poolNodes, poolNodesBytes, d_tlasNodes, tlasNodesBytes,
                                 rootLink, d_records, recordsCapacity};
    if (const int rc = tlas_binary_check_extents(fn, args, d_instances1 && d_motionKeys && d_poolNodes1 && d_blasDeforming)) return rc;
    const int n = numInstances, slots = numInstances - 1;
    if (motionKeysCapacity < (int64_t)kMotionKeyBytes * n)
        return set_error(NTR_ERR_INVALID, "%s: motionKeysCapacity below 128 * numInstances", fn);
    if (((uintptr_t)d_blasDeforming) & 3u) return set_error(NTR_ERR_INVALID, "%s: d_blasDeforming must be 4-byte aligned", fn);
    const TlasRefitLayout lay(slots, numBlas);
    RefitTable held = {1, {}, {lay.table, 0}, {slots, 0}};
    if (const int rc = tlas_binary_range_table(fn, args, (uintptr_t)d_instances1 | (uintptr_t)d_motionKeys | (uintptr_t)d_poolNodes1, held.words[0]))
        return rc;

    hipStream_t s = (hipStream_t)stream;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitRangeWords, g_tdrPool, g_tdrHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    TdrStats* stats = result ? at<TdrStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, base, lay.zeroBytes, &host, &seconds, [&] {
        if (n == 1) {
            hipLaunchKernelGGL(tdr_single, dim3(1), dim3(64), 0, s, d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table,
                               (const unsigned int*)d_blasDeforming, (const char*)d_poolNodes, (const char*)d_poolNodes1, (uint4*)d_records,
                               (uint4*)d_motionKeys, d_sceneBox, sceneCopy, stats);
        } else {
            hipLaunchKernelGGL(tdr_prepare, dim3((n + TDR_BLOCK - 1) / TDR_BLOCK), dim3(TDR_BLOCK), 0, s, n, slots, d_instances0, d_instances1,
                               (int)numBlas, (const uint4*)d_table, (const unsigned int*)d_blasDeforming, (const int*)d_tlasNodes,
                               (uint4*)d_records, (uint4*)d_motionKeys, parent, arrive, stats);
            hipLaunchKernelGGL(tdr_climb, dim3((unsigned int)((2ll * slots + TDR_BLOCK - 1) / TDR_BLOCK)), dim3(TDR_BLOCK), 0, s, n, slots,
                               d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table, (const unsigned int*)d_blasDeforming,
                               (const char*)d_poolNodes, (const char*)d_poolNodes1, (int*)d_tlasNodes, (const unsigned int*)parent, arrive,
                               d_sceneBox, sceneCopy);
        }
    });
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0, moving = 0, deforming = 0;
    unsigned int err = 0;
    refit_fold_slots<TdrStats>(host.data() + lay.stats, [&](const TdrStats& v) {
        inner += v.innerLinks; leafLinks += v.leafLinks; moving += v.moving; deforming += v.deforming; err |= v.err;
    });
    NtrTlasRefitResult& rr = result->motion.refit;
    rr.numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    rr.numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    rr.errBits = (int32_t)err;
    memcpy(rr.sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(rr.sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    rr.seconds = seconds;
    result->motion.numMoving = (int32_t)moving;
    result->numDeforming = (int32_t)deforming;
    if (err & TLAS_ERR_BLAS)
        return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d) (error bits 0x%x); its record, its leaf box and "
                         "the boxes above it were left as they were, everything else was refitted", fn, (int)numBlas, err);
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed top-level tree (error bits 0x%x: 2 a child link that names no slot, 4 a leaf link "
                         "beyond the instances); the boxes above such a place were left as they were, everything else was refitted", fn, err);
    return NTR_OK;
}

int ntr_tlas_deform_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_deform_refit_scratch_bytes", g_tdrPool, bytes); }

}  // extern "C"
