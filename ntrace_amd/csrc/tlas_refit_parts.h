// tlas_refit_parts.h -- what the three in-place top-level refits share, stated once (tlas_refit_kernels.hip, tlas_motion_refit_kernels.hip
// and, where it says so, tlas_wide_refit_kernels.hip).  The world box itself is tlas_world_box.h's; the protocol of the
// call is refit_launch.h's.  Every kernel over these functions compiles to the code it had when it held their statements itself
// (scripts/kernel_isa_diff.sh): a part that does not is taken out again, and the kernel's file says so.
//   device, all three      the error bits; the wave fold of the counters (the stats type is the unit's own: a kernel's parameter list
//                          is part of its name); the scene-box write at the root, from a box or from its two corners
//   device, binary links   the load of a BLAS's node 0; the leaf's climb
//   host, all three        the scratch layout
//   host, binary links     the argument checks and the range table of ntr_tlas_refit and ntr_tlas_motion_refit
// Not here: the classification of a binary slot's two links (tlr_prepare, tmr_prepare) and tmr_prepare's fold with its moving counter,
// which changed the kernels' code when shared; their files say so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_refit_leaf.h"
#include "device_prims.h"
#include "device_scratch.h"
#include "instanced_bvh.h"
#include "refit_launch.h"
#include "tlas_world_box.h"

namespace ntr {

enum : unsigned int { TLAS_ERR_BLAS = 1u, TLAS_ERR_LINK = 2u, TLAS_ERR_LEAF = 4u };

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// One add per wave and counter into the workgroup's slot; the whole wave is here
template <class Stats>
__device__ __forceinline__ void tlas_fold_counters(Stats* __restrict__ slot, unsigned int inner, unsigned int leaf, unsigned int err)
{
    inner = wave_sum_u32(inner);
    leaf = wave_sum_u32(leaf);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (inner) atomicAdd(&slot->innerLinks, inner);
        if (leaf) atomicAdd(&slot->leafLinks, leaf);
        if (err) atomicOr(&slot->err, err);
    }
}

// The root's box (lo x, hi x, lo y, hi y, lo z, hi z) as the scene box (min, then max), to whichever of the two is asked for
__device__ __forceinline__ void tlas_write_scene_box(float* sceneBox /* or null */, float* sceneCopy /* or null */, const float (&box)[6])
{
    if (sceneBox) {
        sceneBox[0] = box[0]; sceneBox[1] = box[2]; sceneBox[2] = box[4];
        sceneBox[3] = box[1]; sceneBox[4] = box[3]; sceneBox[5] = box[5];
    }
    if (sceneCopy) {
        sceneCopy[0] = box[0]; sceneCopy[1] = box[2]; sceneCopy[2] = box[4];
        sceneCopy[3] = box[1]; sceneCopy[4] = box[3]; sceneCopy[5] = box[5];
    }
}

// The same from the two corners: the one instance of a tree without nodes
__device__ __forceinline__ void tlas_write_scene_box(float* sceneBox /* or null */, float* sceneCopy /* or null */, const float (&wlo)[3],
                                                     const float (&whi)[3])
{
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (sceneBox) { sceneBox[q] = wlo[q]; sceneBox[3 + q] = whi[q]; }
        if (sceneCopy) { sceneCopy[q] = wlo[q]; sceneCopy[3 + q] = whi[q]; }
    }
}

// The first three float4 of the node 0 of the BLAS whose table entry is `range` (the host has checked the range against the pool)
__device__ __forceinline__ void tlas_load_node0(const char* __restrict__ poolNodes, const uint4 range, float4& n0, float4& n1, float4& nz)
{
    const float4* nd = (const float4*)(poolNodes + range.x);
    n0 = nd[0]; n1 = nd[1]; nz = nd[2];
}

// Child slot k of `node` is a leaf whose world box is [wlo, whi]: publishes it into the node and runs the climb of bvh_climb.h with
// the integer-order union; the thread that completes the root writes the scene box
__device__ __forceinline__ void tlas_leaf_climb(int node, int k, int numSlots, int* nodes, const unsigned int* __restrict__ parent,
                                                unsigned int* __restrict__ arrive, const float (&wlo)[3], const float (&whi)[3],
                                                float* sceneBox /* or null */, float* sceneCopy /* or null */)
{
    float box[6] = {wlo[0], whi[0], wlo[1], whi[1], wlo[2], whi[2]};
    rf_publish_box(nodes, node, k, box);
    float sib[6];
    climb(
        node, k, numSlots, nodes, parent, arrive, [&](int pn, int pk) { rf_publish_box(nodes, pn, pk, box); },
        [&](int nd, int sk) { rf_acquire_box(nodes, nd, sk, sib); },
        [&](int nd, int) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                box[2 * q] = ord_min(box[2 * q], sib[2 * q]);
                box[2 * q + 1] = ord_max(box[2 * q + 1], sib[2 * q + 1]);
            }
            if (nd == 0) tlas_write_scene_box(sceneBox, sceneCopy, box);   // the root reports to no parent
        });
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// The scratch of a call over `climbed` node slots (binary) or wide nodes: one zeroed block -- the counters and the blocking form's scene
// box (6 floats, zero while the root has not been refitted) -- then the range table and the climb's two words per slot
struct TlasRefitLayout {
    size_t stats, scene, zeroBytes, table, parent, arrive, end;
    TlasRefitLayout(int64_t climbed, int64_t numBlas)
    {
        ScratchCarver c;
        stats = c.take((size_t)64 * kRefitStatSlots);
        scene = c.take(6 * sizeof(float));
        zeroBytes = c.off;
        table = c.take((size_t)numBlas * 16);
        parent = c.take((size_t)climbed * 4);
        arrive = c.take((size_t)climbed * 4);
        end = c.off;
    }
};

// The arguments that ntr_tlas_refit and ntr_tlas_motion_refit share
struct TlasBinaryArgs {
    int32_t numInstances;
    const NtrInstance* d_instances;              // (key 0's)
    int32_t numBlas;
    const NtrBlasRange* blasRanges;
    const void* d_poolNodes;
    int64_t poolNodesBytes;
    void* d_tlasNodes;
    int64_t tlasNodesBytes;
    int32_t rootLink;
    void* d_records;
    int64_t recordsCapacity;
};

// The checks up to the records' capacity.  ownBuffers: the entry point's further buffers are all non-null
inline int tlas_binary_check_extents(const char* fn, const TlasBinaryArgs& a, bool ownBuffers = true)
{
    if (a.numInstances < 1 || (int64_t)a.numInstances - 1 > kMaxNodes || a.numBlas < 1 || !a.d_instances || !ownBuffers || !a.blasRanges ||
        !a.d_poolNodes || !a.d_records || (!a.d_tlasNodes && a.numInstances > 1))
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numInstances <= %lld, numBlas >= 1, non-null buffers)", fn,
                         (long long)kMaxNodes + 1);
    const int n = a.numInstances;
    if (a.tlasNodesBytes != (int64_t)kNodeBytes * (n - 1))
        return set_error(NTR_ERR_INVALID, "%s: tlasNodesBytes must be 64 * (numInstances - 1), the extent ntr_tlas_build reported", fn);
    if (a.rootLink != (n == 1 ? leaf_link(0) : 0))
        return set_error(NTR_ERR_INVALID, "%s: rootLink must be 0, or ~0 for one instance, as ntr_tlas_build reported it", fn);
    if (a.recordsCapacity < (int64_t)kRecordBytes * n) return set_error(NTR_ERR_INVALID, "%s: recordsCapacity below 64 * numInstances", fn);
    return NTR_OK;
}

// The checks from the buffers' alignment on, and the device's range table: per BLAS nodesOffset, triWoopOffset / 16, nodesBytes, 0.
// ownPointers: the entry point's further buffers, or-ed
inline int tlas_binary_range_table(const char* fn, const TlasBinaryArgs& a, uintptr_t ownPointers, std::vector<uint32_t>& table)
{
    if (((uintptr_t)a.d_poolNodes | (uintptr_t)a.d_records | (uintptr_t)a.d_tlasNodes | (uintptr_t)a.d_instances | ownPointers) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", a.poolNodesBytes, kNodeBytes)) return rc;
    table = std::vector<uint32_t>(4 * (size_t)a.numBlas);
    for (int k = 0; k < a.numBlas; k++) {
        if (const int rc = check_blas_range(fn, k, a.blasRanges[k], a.poolNodesBytes)) return rc;
        table[4 * k] = (uint32_t)a.blasRanges[k].nodesOffset;
        table[4 * k + 1] = (uint32_t)(a.blasRanges[k].triWoopOffset / kRowBytes);
        table[4 * k + 2] = (uint32_t)a.blasRanges[k].nodesBytes;
        table[4 * k + 3] = 0u;
    }
    return NTR_OK;
}

}  // namespace ntr
