// tlas_wide_motion_refit_kernels.hip -- in-place refit of a 4-wide top-level tree to instances that move within the shutter, for gfx950
// (ntr_tlas_wide_motion_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_wide_motion.py (wide_motion_refit), and the header comment of
// ntr_tlas_wide_motion_refit (include/ntrace_amd.h) states the contract.  It is tlas_wide_refit_kernels.hip's refit over two instance
// arrays -- key 0, the shutter's opening, and key 1, its close -- with the three changes tlas_motion_refit_kernels.hip makes to the
// binary refit, and the same two launches:
//   twm_prepare   one thread per index up to max(wide nodes, N): the topology step of wide_climb.h for wide node i; wide record i of
//                 key-0 instance i (wide_write_record, instanced_wide_bvh.h, as it is) with word 15 = 1 where the twelve objectToWorld
//                 words differ between the keys; and motion key entry i (128 bytes: key 0's objectToWorld, zeros, key 1's, zeros),
//                 for every instance -- byte for byte ntr_tlas_motion_refit's, so the all-wide update needs no binary motion refit
//   twm_climb     one thread per slot: a leaf link ~i forms instance i's world box under key 0 and, where it moves, under key 1 -- both
//                 from the union of the root slots of its wide BLAS (tlw_root_box; the pool's node 0 is not read), through
//                 tlr_world_box of tlas_world_box.h, called twice and not restated -- publishes their integer-order union and runs the
//                 climb of wide_climb.h
//   twm_single    N == 1 has no node: record 0, key entry 0 and the scene box in one small launch
// Every corner of the object box moves on a straight line between its two end positions, up to rounding, so the union of the two end
// boxes bounds the sweep; no padding, as everywhere else in the instanced path.
// The arrival protocol and its memory ordering are wide_climb.h's and are not restated.  A bad part is never followed, as in
// tlas_wide_refit_kernels.hip: a link that names no wide node, a leaf link beyond the instances and an instance whose blas index (key
// 0's) names no BLAS are skipped; such an instance gets the record with the empty extent, and its key entry is written all the same
// (it depends on the transforms only).
// The error bits and the scene-box write are tlas_refit_parts.h's; the argument checks, the range table and the object box of a wide
// BLAS are tlas_wide_refit_parts.h's (this entry point adds its second instance array and the motion keys where they stand in the
// order of the checks); the held table, the refusals of a captured call and the bracket of the blocking form are refit_launch.h's.
// Kept as text, as tmr_prepare keeps it and for its reason: the wave fold with the moving counter between the shared fold's
// statements.  The key loads, the comparison and the key entry are tlas_motion_refit_kernels.hip's statements a second time: that
// unit's kernels hold them in its anonymous namespace, and a move into a header would have to leave its three kernels' code as it is.
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

constexpr int TWM_BLOCK = 256;

// A counter slot of the blocking form (refit_launch.h): tlas_wide_refit_kernels.hip's counters and the moving instances
struct TwmStats {
    unsigned int innerLinks, leafLinks, err, moving;
    unsigned int pad[12];        // a slot per 64-byte line
};
static_assert(sizeof(TwmStats) == 64, "TwmStats must be 64 bytes");

DeviceScratchPool g_twmPool;
RefitHeld g_twmHeld[kMaxDevices];

// objectToWorld of instance i: 48 bytes at the start of a 112-byte struct of a 16-byte aligned array
__device__ __forceinline__ void twm_load_key(const NtrInstance* __restrict__ inst, int i, uint4 (&m)[3])
{
    const uint4* src = reinterpret_cast<const uint4*>(inst[i].objectToWorld);
    m[0] = src[0]; m[1] = src[1]; m[2] = src[2];
}

__device__ __forceinline__ bool twm_differs(const uint4 (&a)[3], const uint4 (&b)[3])
{
    unsigned int d = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) d |= (a[k].x ^ b[k].x) | (a[k].y ^ b[k].y) | (a[k].z ^ b[k].z) | (a[k].w ^ b[k].w);
    return d != 0u;
}

// Motion key entry i (instanced_bvh.h), whatever instance i's blas index is.  -> the instance moves
__device__ __forceinline__ bool twm_write_key(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                              uint4* __restrict__ keys)
{
    uint4 a[3], b[3];
    twm_load_key(inst0, i, a);
    twm_load_key(inst1, i, b);
    uint4* e = keys + (kMotionKeyBytes / 16) * (size_t)i;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    e[0] = a[0]; e[1] = a[1]; e[2] = a[2]; e[3] = zero;
    e[4] = b[0]; e[5] = b[1]; e[6] = b[2]; e[7] = zero;
    return twm_differs(a, b);
}

// Wide record i of key-0 instance i: ntr_tlas_widen's record (wide_write_record writes word 15 = 0), then word 15 of a moving instance
__device__ __forceinline__ void twm_write_record(const NtrInstance* __restrict__ inst0, int i, int numBlas, const uint4* __restrict__ table,
                                                 bool moving, uint4* __restrict__ records)
{
    wide_write_record(inst0, i, numBlas, table, records);
    if (moving) reinterpret_cast<uint32_t*>(records + 4 * (size_t)i)[kRecMoving] = 1u;
}

__device__ __forceinline__ void twm_matrix(const uint4 (&k)[3], float (&m)[12])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        m[4 * r] = __uint_as_float(k[r].x); m[4 * r + 1] = __uint_as_float(k[r].y);
        m[4 * r + 2] = __uint_as_float(k[r].z); m[4 * r + 3] = __uint_as_float(k[r].w);
    }
}

// The swept world box of instance i, whose blas index the caller has checked, from the current root of its wide BLAS.  -> false: the
// root's count word lies outside 2..4
__device__ __forceinline__ bool twm_instance_box(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                                 const uint4 range, const char* __restrict__ widePool, float (&wlo)[3], float (&whi)[3])
{
    float b[6];
    if (!tlw_root_box(widePool, range, b)) return false;
    // the object box as a binary node 0 both of whose children hold it
    const float4 n01 = make_float4(b[0], b[1], b[2], b[3]), nz = make_float4(b[4], b[5], b[4], b[5]);
    uint4 k0[3], k1[3];
    twm_load_key(inst0, i, k0);
    twm_load_key(inst1, i, k1);
    float m[12];
    twm_matrix(k0, m);
    tlr_world_box(n01, n01, nz, m, wlo, whi);
    if (!twm_differs(k0, k1)) return true;
    twm_matrix(k1, m);
    float lo1[3], hi1[3];
    tlr_world_box(n01, n01, nz, m, lo1, hi1);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        wlo[q] = ord_min(wlo[q], lo1[q]);
        whi[q] = ord_max(whi[q], hi1[q]);
    }
    return true;
}

__global__ __launch_bounds__(TWM_BLOCK) void twm_prepare(int n, int numNodes, const NtrInstance* __restrict__ inst0,
                                                         const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                         const int* __restrict__ nodes, uint4* __restrict__ records, uint4* __restrict__ keys,
                                                         unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                         TwmStats* __restrict__ stats /* or null */)
{
    const int idx = blockIdx.x * TWM_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0, moving = 0;
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
        const bool mv = twm_write_key(inst0, inst1, idx, keys);
        moving = mv ? 1u : 0u;
        const int b = inst0[idx].blas;
        if (b < 0 || b >= numBlas) err |= TLAS_ERR_BLAS;
        twm_write_record(inst0, idx, numBlas, table, mv, records);   // (with the empty extent for such an instance)
    }
    if (!stats) return;
    stats += blockIdx.x % kRefitStatSlots;
    // one add per wave and counter: tlas_fold_counters (tlas_refit_parts.h) with `moving` between its statements, as tmr_prepare has it
    inner = wave_sum_u32(inner);
    leaf = wave_sum_u32(leaf);
    moving = wave_sum_u32(moving);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (inner) atomicAdd(&stats->innerLinks, inner);
        if (leaf) atomicAdd(&stats->leafLinks, leaf);
        if (moving) atomicAdd(&stats->moving, moving);
        if (err) atomicOr(&stats->err, err);
    }
}

__global__ __launch_bounds__(TWM_BLOCK) void twm_climb(int n, int numNodes, const NtrInstance* __restrict__ inst0,
                                                       const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                       const char* __restrict__ widePool, int* nodes, const unsigned int* __restrict__ parent,
                                                       unsigned int* __restrict__ arrive, float* sceneBox /* or null */,
                                                       float* sceneCopy /* or null: the blocking form's */, TwmStats* __restrict__ stats /* or null */)
{
    const unsigned int gid = blockIdx.x * (unsigned int)TWM_BLOCK + threadIdx.x;   // < 4 * numNodes + TWM_BLOCK < 2^27
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
        const int b = inst0[i].blas;
        if (b < 0 || b >= numBlas) return;
        float wlo[3], whi[3];
        if (!twm_instance_box(inst0, inst1, i, table[b], widePool, wlo, whi)) return;
        const float box[6] = {wlo[0], whi[0], wlo[1], whi[1], wlo[2], whi[2]};
        wide_publish_box(nodes, node, k, box);
    }
    wide_climb(node, numNodes, nodes, parent, arrive, sceneBox, sceneCopy);
}

// N == 1: one thread
__global__ __launch_bounds__(64) void twm_single(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int numBlas,
                                                 const uint4* __restrict__ table, const char* __restrict__ widePool,
                                                 uint4* __restrict__ records, uint4* __restrict__ keys, float* sceneBox /* or null */,
                                                 float* sceneCopy /* or null */, TwmStats* __restrict__ stats /* or null */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool mv = twm_write_key(inst0, inst1, 0, keys);
    if (stats) stats->moving = mv ? 1u : 0u;
    twm_write_record(inst0, 0, numBlas, table, mv, records);
    const int b = inst0[0].blas;
    if (b < 0 || b >= numBlas) {
        if (stats) stats->err = TLAS_ERR_BLAS;
        return;
    }
    float wlo[3], whi[3];
    if (!twm_instance_box(inst0, inst1, 0, table[b], widePool, wlo, whi)) return;
    tlas_write_scene_box(sceneBox, sceneCopy, wlo, whi);
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_tlas_wide_motion_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1, int32_t numBlas,
                               const NtrBlasRange* blasRanges, const NtrWideBlasRange* wideRanges, const void* d_widePoolNodes,
                               int64_t widePoolNodesBytes, void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                               void* d_wideRecords, int64_t recordsCapacity, void* d_motionKeys, int64_t motionKeysCapacity, float* d_sceneBox,
                               NtrTlasMotionRefitResult* result, void* stream)
{
    const char* fn = "ntr_tlas_wide_motion_refit";
    if (result) memset(result, 0, sizeof(*result));
    const TlasWideArgs args = {numInstances, d_instances0, numBlas, blasRanges, wideRanges, d_widePoolNodes, widePoolNodesBytes, d_wideTlasNodes,
                               wideTlasNodesBytes, rootLink, d_wideRecords, recordsCapacity};
    if (const int rc = tlas_wide_check_extents(fn, args, d_instances1 && d_motionKeys)) return rc;
    const int n = numInstances, numNodes = (int)(wideTlasNodesBytes / kWideBytes);
    if (motionKeysCapacity < (int64_t)kMotionKeyBytes * n)
        return set_error(NTR_ERR_INVALID, "%s: motionKeysCapacity below 128 * numInstances", fn);
    const TlasRefitLayout lay(numNodes, numBlas);
    RefitTable held = {1, {}, {lay.table, 0}, {n, numNodes}};
    if (const int rc = tlas_wide_range_table(fn, args, (uintptr_t)d_instances1 | (uintptr_t)d_motionKeys, held.words[0])) return rc;

    hipStream_t s = (hipStream_t)stream;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitRangeExtentWords, g_twmPool, g_twmHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    TwmStats* stats = result ? at<TwmStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, base, lay.zeroBytes, &host, &seconds, [&] {
        if (n == 1) {
            hipLaunchKernelGGL(twm_single, dim3(1), dim3(64), 0, s, d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table,
                               (const char*)d_widePoolNodes, (uint4*)d_wideRecords, (uint4*)d_motionKeys, d_sceneBox, sceneCopy, stats);
        } else {
            const int threads = std::max(n, numNodes);
            hipLaunchKernelGGL(twm_prepare, dim3((threads + TWM_BLOCK - 1) / TWM_BLOCK), dim3(TWM_BLOCK), 0, s, n, numNodes, d_instances0,
                               d_instances1, (int)numBlas, (const uint4*)d_table, (const int*)d_wideTlasNodes, (uint4*)d_wideRecords,
                               (uint4*)d_motionKeys, parent, arrive, stats);
            hipLaunchKernelGGL(twm_climb, dim3((unsigned int)((4ll * numNodes + TWM_BLOCK - 1) / TWM_BLOCK)), dim3(TWM_BLOCK), 0, s, n, numNodes,
                               d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table, (const char*)d_widePoolNodes,
                               (int*)d_wideTlasNodes, (const unsigned int*)parent, arrive, d_sceneBox, sceneCopy, stats);
        }
    });
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0, moving = 0;
    unsigned int err = 0;
    refit_fold_slots<TwmStats>(host.data() + lay.stats, [&](const TwmStats& v) {
        inner += v.innerLinks; leafLinks += v.leafLinks; moving += v.moving; err |= v.err;
    });
    NtrTlasRefitResult& rr = result->refit;
    rr.numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    rr.numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    rr.errBits = (int32_t)err;
    memcpy(rr.sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(rr.sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    rr.seconds = seconds;
    result->numMoving = (int32_t)moving;
    if (err & TLAS_ERR_BLAS)
        return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d) (error bits 0x%x); its record has the empty extent, "
                         "its leaf box and the boxes above it were left as they were, everything else was refitted", fn, (int)numBlas, err);
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed wide top-level tree (error bits 0x%x: 2 a link that names no wide node, a node named "
                         "twice or a count word outside 2..4, 4 a leaf link beyond the instances); the boxes above such a place were left as "
                         "they were, everything else was refitted", fn, err);
    return NTR_OK;
}

int ntr_tlas_wide_motion_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_wide_motion_refit_scratch_bytes", g_twmPool, bytes); }

}  // extern "C"
