// tlas_motion_refit_kernels.hip -- on-device refit of a top-level tree to instances that move within the shutter, for gfx950
// (ntr_tlas_motion_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_motion.py (motion_refit), and the header comment of ntr_tlas_motion_refit
// (include/ntrace_amd.h) states the contract.  It is tlas_refit_kernels.hip's refit over two instance arrays -- key 0, the shutter's
// opening, and key 1, its close -- with three changes, and the same two launches:
//   tmr_prepare   one thread per index up to max(N - 1, N): the topology step of bvh_climb.h for node slot i; record i of key-0
//                 instance i (instanced_bvh.h) with word 15 = 1 where the twelve objectToWorld words differ between the keys; and
//                 motion key entry i (128 bytes: key 0's objectToWorld, zeros, key 1's, zeros), for every instance
//   tmr_climb     one thread per child slot: a leaf link ~i forms instance i's world box under key 0 and, where it moves, under key 1
//                 (tlr_world_box of tlas_world_box.h, called twice; its statements are not restated), publishes their integer-order
//                 union into the node and runs the climb of bvh_climb.h
//   tmr_single    N == 1 has no node: record 0, key entry 0 and the scene box in one small launch
// Every corner of the object box moves on a straight line between its two end positions, up to rounding, so the union of the two end
// boxes bounds the sweep; no padding, as everywhere else in the instanced path.
// The arrival protocol and its memory ordering are bvh_climb.h's and are not restated.  A bad part is never followed, as in
// tlas_refit_kernels.hip: a link that names no slot, a leaf link beyond the instances and an instance whose blas index (key 0's) names
// no BLAS are skipped; such an instance keeps its record but its key entry is written all the same (it depends on the transforms only).
// No host read-back unless a result is asked for, and no memset node on the asynchronous path.
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
#include "tlas_world_box.h"

namespace ntr {
namespace {

constexpr int TMR_BLOCK = 256;
enum : unsigned int { TMR_ERR_BLAS = 1u, TMR_ERR_LINK = 2u, TMR_ERR_LEAF = 4u };

// Counters of the blocking form, as tlas_refit_kernels.hip's, and the moving instances
constexpr int TMR_STAT_SLOTS = 256;
struct TmrStats {
    unsigned int innerLinks, leafLinks, err, moving;
    unsigned int pad[12];        // a slot per 64-byte line
};
static_assert(sizeof(TmrStats) == 64, "TmrStats must be 64 bytes");

DeviceScratchPool g_tmrPool;

// objectToWorld of instance i: 48 bytes at the start of a 112-byte struct of a 16-byte aligned array
__device__ __forceinline__ void tmr_load_key(const NtrInstance* __restrict__ inst, int i, uint4 (&m)[3])
{
    const uint4* src = reinterpret_cast<const uint4*>(inst[i].objectToWorld);
    m[0] = src[0]; m[1] = src[1]; m[2] = src[2];
}

__device__ __forceinline__ bool tmr_differs(const uint4 (&a)[3], const uint4 (&b)[3])
{
    unsigned int d = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) d |= (a[k].x ^ b[k].x) | (a[k].y ^ b[k].y) | (a[k].z ^ b[k].z) | (a[k].w ^ b[k].w);
    return d != 0u;
}

// Motion key entry i (instanced_bvh.h), whatever instance i's blas index is.  -> the instance moves
__device__ __forceinline__ bool tmr_write_key(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                              uint4* __restrict__ keys)
{
    uint4 a[3], b[3];
    tmr_load_key(inst0, i, a);
    tmr_load_key(inst1, i, b);
    uint4* e = keys + (kMotionKeyBytes / 16) * (size_t)i;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    e[0] = a[0]; e[1] = a[1]; e[2] = a[2]; e[3] = zero;
    e[4] = b[0]; e[5] = b[1]; e[6] = b[2]; e[7] = zero;
    return tmr_differs(a, b);
}

// Record i of key-0 instance i, whose blas index the caller has checked; range is the table's entry of its BLAS
__device__ __forceinline__ void tmr_write_record(const NtrInstance* __restrict__ inst0, int i, const uint4 range, bool moving,
                                                 uint4* __restrict__ records)
{
    const uint4* inv = reinterpret_cast<const uint4*>(inst0[i].worldToObject);
    uint4* rec = records + 4 * (size_t)i;
    rec[0] = inv[0];
    rec[1] = inv[1];
    rec[2] = inv[2];
    rec[3] = make_uint4(range.x, range.y, range.z, moving ? 1u : 0u);
}

// The swept world box of instance i, whose blas index the caller has checked, from the pool's current node 0 of its BLAS
__device__ __forceinline__ void tmr_instance_box(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int i,
                                                 const uint4 range, const char* __restrict__ poolNodes, float (&wlo)[3], float (&whi)[3])
{
    const float4* nd = (const float4*)(poolNodes + range.x);   // (the host has checked the range against the pool)
    const float4 n0 = nd[0], n1 = nd[1], nz = nd[2];
    uint4 a[3], b[3];
    tmr_load_key(inst0, i, a);
    tmr_load_key(inst1, i, b);
    float m[12];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        m[4 * k] = __uint_as_float(a[k].x); m[4 * k + 1] = __uint_as_float(a[k].y);
        m[4 * k + 2] = __uint_as_float(a[k].z); m[4 * k + 3] = __uint_as_float(a[k].w);
    }
    tlr_world_box(n0, n1, nz, m, wlo, whi);
    if (!tmr_differs(a, b)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        m[4 * k] = __uint_as_float(b[k].x); m[4 * k + 1] = __uint_as_float(b[k].y);
        m[4 * k + 2] = __uint_as_float(b[k].z); m[4 * k + 3] = __uint_as_float(b[k].w);
    }
    float lo1[3], hi1[3];
    tlr_world_box(n0, n1, nz, m, lo1, hi1);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        wlo[q] = ord_min(wlo[q], lo1[q]);
        whi[q] = ord_max(whi[q], hi1[q]);
    }
}

__global__ __launch_bounds__(TMR_BLOCK) void tmr_prepare(int n, int numSlots, const NtrInstance* __restrict__ inst0,
                                                         const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                         const int* __restrict__ nodes, uint4* __restrict__ records, uint4* __restrict__ keys,
                                                         unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                         TmrStats* __restrict__ stats /* or null */)
{
    const int idx = blockIdx.x * TMR_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0, moving = 0;
    if (idx < numSlots) {
        int kind[2];
        topology_slot(idx, numSlots, nodes, parent, arrive, kind);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            inner += kind[k] == LINK_INNER ? 1u : 0u;
            if (kind[k] == LINK_BAD) err |= TMR_ERR_LINK;
            if (kind[k] == LINK_LEAF) {
                leaf += 1u;
                if (leaf_row(nodes[(size_t)idx * kNodeWords + kLinkWord + k]) >= n) err |= TMR_ERR_LEAF;
            }
        }
    }
    if (idx < n) {
        const bool mv = tmr_write_key(inst0, inst1, idx, keys);
        moving = mv ? 1u : 0u;
        const int b = inst0[idx].blas;
        if (b < 0 || b >= numBlas) err |= TMR_ERR_BLAS;
        else tmr_write_record(inst0, idx, table[b], mv, records);
    }
    if (!stats) return;
    stats += blockIdx.x % TMR_STAT_SLOTS;
    // one add per wave and counter
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

__global__ __launch_bounds__(TMR_BLOCK) void tmr_climb(int n, int numSlots, const NtrInstance* __restrict__ inst0,
                                                       const NtrInstance* __restrict__ inst1, int numBlas, const uint4* __restrict__ table,
                                                       const char* __restrict__ poolNodes, int* nodes, const unsigned int* __restrict__ parent,
                                                       unsigned int* __restrict__ arrive, float* sceneBox /* or null */,
                                                       float* sceneCopy /* or null: the blocking form's */)
{
    const unsigned int gid = blockIdx.x * (unsigned int)TMR_BLOCK + threadIdx.x;   // < 2 * numSlots + TMR_BLOCK < 2^26
    const int node = (int)(gid >> 1), k = (int)(gid & 1u);
    if (node >= numSlots) return;
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (link >= 0) return;                       // an inner child arrives with the owner of its node; offset 0 is no child at all
    const int i = leaf_row(link);                // >= 0
    if (i >= n) return;                          // after a bad part the nodes above keep an arrival short and stay as they are
    const int b = inst0[i].blas;
    if (b < 0 || b >= numBlas) return;
    float wlo[3], whi[3];
    tmr_instance_box(inst0, inst1, i, table[b], poolNodes, wlo, whi);
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
            if (nd == 0) {                       // the root reports to no parent
                if (sceneBox) {
                    sceneBox[0] = box[0]; sceneBox[1] = box[2]; sceneBox[2] = box[4];
                    sceneBox[3] = box[1]; sceneBox[4] = box[3]; sceneBox[5] = box[5];
                }
                if (sceneCopy) {
                    sceneCopy[0] = box[0]; sceneCopy[1] = box[2]; sceneCopy[2] = box[4];
                    sceneCopy[3] = box[1]; sceneCopy[4] = box[3]; sceneCopy[5] = box[5];
                }
            }
        });
}

// N == 1: one thread
__global__ __launch_bounds__(64) void tmr_single(const NtrInstance* __restrict__ inst0, const NtrInstance* __restrict__ inst1, int numBlas,
                                                 const uint4* __restrict__ table, const char* __restrict__ poolNodes,
                                                 uint4* __restrict__ records, uint4* __restrict__ keys, float* sceneBox /* or null */,
                                                 float* sceneCopy /* or null */, TmrStats* __restrict__ stats /* or null */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool mv = tmr_write_key(inst0, inst1, 0, keys);
    if (stats) stats->moving = mv ? 1u : 0u;
    const int b = inst0[0].blas;
    if (b < 0 || b >= numBlas) {
        if (stats) stats->err = TMR_ERR_BLAS;
        return;
    }
    const uint4 range = table[b];
    tmr_write_record(inst0, 0, range, mv, records);
    float wlo[3], whi[3];
    tmr_instance_box(inst0, inst1, 0, range, poolNodes, wlo, whi);
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (sceneBox) { sceneBox[q] = wlo[q]; sceneBox[3 + q] = whi[q]; }
        if (sceneCopy) { sceneCopy[q] = wlo[q]; sceneCopy[3 + q] = whi[q]; }
    }
}

struct TmrLayout {
    size_t stats, scene, zeroBytes, table, parent, arrive, end;
    TmrLayout(int64_t slots, int64_t numBlas)
    {
        ScratchCarver c;
        stats = c.take(sizeof(TmrStats) * TMR_STAT_SLOTS);   // one zeroed block: the counters and the blocking form's scene box
        scene = c.take(6 * sizeof(float));
        zeroBytes = c.off;
        table = c.take((size_t)numBlas * 16);
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        end = c.off;
    }
};

// What the device's range table holds, per device (tlas_refit_kernels.hip's rule; this unit's pool has a table of its own)
struct TmrUploaded {
    bool valid = false;
    int slots = 0;
    std::vector<uint32_t> table;
};
TmrUploaded g_tmrUploaded[kMaxDevices];

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_tlas_motion_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1, int32_t numBlas,
                          const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes, void* d_tlasNodes,
                          int64_t tlasNodesBytes, int32_t rootLink, void* d_records, int64_t recordsCapacity, void* d_motionKeys,
                          int64_t motionKeysCapacity, float* d_sceneBox, NtrTlasMotionRefitResult* result, void* stream)
{
    const char* fn = "ntr_tlas_motion_refit";
    if (result) memset(result, 0, sizeof(*result));
    if (numInstances < 1 || (int64_t)numInstances - 1 > kMaxNodes || numBlas < 1 || !d_instances0 || !d_instances1 || !blasRanges ||
        !d_poolNodes || !d_records || !d_motionKeys || (!d_tlasNodes && numInstances > 1))
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numInstances <= %lld, numBlas >= 1, non-null buffers)", fn,
                         (long long)kMaxNodes + 1);
    const int n = numInstances, slots = numInstances - 1;
    if (tlasNodesBytes != (int64_t)kNodeBytes * slots)
        return set_error(NTR_ERR_INVALID, "%s: tlasNodesBytes must be 64 * (numInstances - 1), the extent ntr_tlas_build reported", fn);
    if (rootLink != (n == 1 ? leaf_link(0) : 0))
        return set_error(NTR_ERR_INVALID, "%s: rootLink must be 0, or ~0 for one instance, as ntr_tlas_build reported it", fn);
    if (recordsCapacity < (int64_t)kRecordBytes * n) return set_error(NTR_ERR_INVALID, "%s: recordsCapacity below 64 * numInstances", fn);
    if (motionKeysCapacity < (int64_t)kMotionKeyBytes * n)
        return set_error(NTR_ERR_INVALID, "%s: motionKeysCapacity below 128 * numInstances", fn);
    if (((uintptr_t)d_poolNodes | (uintptr_t)d_records | (uintptr_t)d_tlasNodes | (uintptr_t)d_instances0 | (uintptr_t)d_instances1 |
         (uintptr_t)d_motionKeys) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    std::vector<uint32_t> table(4 * (size_t)numBlas);
    for (int k = 0; k < numBlas; k++) {
        if (const int rc = check_blas_range(fn, k, blasRanges[k], poolNodesBytes)) return rc;
        table[4 * k] = (uint32_t)blasRanges[k].nodesOffset;
        table[4 * k + 1] = (uint32_t)(blasRanges[k].triWoopOffset / kRowBytes);
        table[4 * k + 2] = (uint32_t)blasRanges[k].nodesBytes;
        table[4 * k + 3] = 0u;
    }

    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
    const TmrLayout lay(slots, numBlas);
    TmrUploaded& up = g_tmrUploaded[dev];
    if (g_tmrPool.held() < lay.end) up.valid = false;   // released, never reserved, or about to be regrown
    const bool same = up.valid && up.table == table;
    const bool capturing = stream_is_capturing(s);
    if (capturing && result) return set_error(NTR_ERR_INVALID, "%s: a captured call cannot read a result back (pass result = NULL)", fn);
    if (capturing && !(same && up.slots == slots))
        return set_error(NTR_ERR_INVALID, "%s: a captured call uploads and allocates nothing: the device must hold this range table already "
                         "-- make one uncaptured call with the same ranges and instance count first (and none with others, and no "
                         "ntr_lbvh_release_workspace, between it and the capture)", fn);
    void* base = nullptr;
    if (const int rc = g_tmrPool.reserve(lay.end, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    if (!same) {
        // the host copy is what the upload reads and what the next call compares with: the upload is waited for
        up.valid = false;
        up.table.swap(table);
        NTR_HIP(hipMemcpyAsync(d_table, up.table.data(), up.table.size() * 4, hipMemcpyHostToDevice, s));
        NTR_HIP(hipStreamSynchronize(s));
        up.valid = true;
    }
    if (!capturing) up.slots = slots;
    TmrStats* stats = result ? at<TmrStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    StreamEvents<2> ev(s);
    if (result) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
        NTR_HIP(hipMemsetAsync(at<char>(base, 0), 0, lay.zeroBytes, s));
    }
    if (n == 1) {
        hipLaunchKernelGGL(tmr_single, dim3(1), dim3(64), 0, s, d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table,
                           (const char*)d_poolNodes, (uint4*)d_records, (uint4*)d_motionKeys, d_sceneBox, sceneCopy, stats);
    } else {
        hipLaunchKernelGGL(tmr_prepare, dim3((n + TMR_BLOCK - 1) / TMR_BLOCK), dim3(TMR_BLOCK), 0, s, n, slots, d_instances0, d_instances1,
                           (int)numBlas, (const uint4*)d_table, (const int*)d_tlasNodes, (uint4*)d_records, (uint4*)d_motionKeys, parent, arrive,
                           stats);
        hipLaunchKernelGGL(tmr_climb, dim3((unsigned int)((2ll * slots + TMR_BLOCK - 1) / TMR_BLOCK)), dim3(TMR_BLOCK), 0, s, n, slots,
                           d_instances0, d_instances1, (int)numBlas, (const uint4*)d_table, (const char*)d_poolNodes, (int*)d_tlasNodes,
                           (const unsigned int*)parent, arrive, d_sceneBox, sceneCopy);
    }
    NTR_HIP(hipGetLastError());
    if (!result) return NTR_OK;

    NTR_HIP(ev.record(1));
    std::vector<char> host(lay.zeroBytes);       // the copy is waited for right here
    NTR_HIP(hipMemcpyAsync(host.data(), at<char>(base, 0), lay.zeroBytes, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    uint64_t inner = 0, leafLinks = 0, moving = 0;
    unsigned int err = 0;
    const TmrStats* hs = (const TmrStats*)(host.data() + lay.stats);
    for (int k = 0; k < TMR_STAT_SLOTS; k++) { inner += hs[k].innerLinks; leafLinks += hs[k].leafLinks; moving += hs[k].moving; err |= hs[k].err; }
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    NtrTlasRefitResult& rr = result->refit;
    rr.numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    rr.numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    rr.errBits = (int32_t)err;
    memcpy(rr.sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(rr.sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    rr.seconds = ms * 1e-3f;
    result->numMoving = (int32_t)moving;
    if (err & TMR_ERR_BLAS)
        return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d) (error bits 0x%x); its record, its leaf box and "
                         "the boxes above it were left as they were, everything else was refitted", fn, (int)numBlas, err);
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed top-level tree (error bits 0x%x: 2 a child link that names no slot, 4 a leaf link "
                         "beyond the instances); the boxes above such a place were left as they were, everything else was refitted", fn, err);
    return NTR_OK;
}

int ntr_tlas_motion_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_motion_refit_scratch_bytes", g_tmrPool, bytes); }

}  // extern "C"
