// tlas_refit_kernels.hip -- on-device refit of a top-level tree to moved instances for gfx950 (ntr_tlas_refit).
//
// An EXTENSION: the rule is the numpy spec tests/np_tlas_refit.py, and the header comment of ntr_tlas_refit (include/ntrace_amd.h)
// states the contract.  ntr_tlas_build is a blocking chain of some dozens of launches; a frame whose instances move, or whose BLASes
// were refitted, only needs the records and the boxes again.  Two launches keep the topology and rewrite both:
//   tlr_prepare   one thread per index up to max(N - 1, N): the topology step of bvh_climb.h for node slot i, and record i of
//                 instance i (instanced_bvh.h)
//   tlr_climb     one thread per child slot: a leaf link ~i forms instance i's world box (tlr_world_box), publishes it into the node
//                 and runs the climb of bvh_climb.h with the integer-order union
//   tlr_single    N == 1 has no node: record 0 and the scene box in one small launch
// tlr_world_box (tlas_world_box.h: the wide and the motion refit share it) holds the statements of tl_boxes (tlas_build_kernels.hip),
// which does NOT call it: built over a shared function, tl_boxes came out with other code than before (the operands of twelve additions
// commuted; scripts/kernel_isa_diff.sh), so that file was left as it was.  A change to the world-box rule is made in both
// places; tests/test_tlas_refit_gpu.py demands that the refit of a fresh build changes no byte at every size it runs.
// The arrival protocol and its memory ordering are bvh_climb.h's and are not restated.  A bad part is never followed: a link that names
// no slot, a leaf link beyond the instances and an instance whose blas index names no BLAS are skipped, so their ancestors keep an
// arrival short and stay as they are; everything else is refitted completely.
// What the three top-level refits share on the device, the argument checks and the range table are tlas_refit_parts.h's; the held
// table, the refusals of a captured call and the bracket of the blocking form are refit_launch.h's.  One part is
// deliberately NOT shared: the classification of a node slot's two links in tlr_prepare (and, word for word, in tmr_prepare) -- built
// over a shared function, by reference, by value or over the kinds alone, the kernel came out with other code (other branches around
// the leaf_row test; scripts/kernel_isa_diff.sh), so both kernels keep the text.
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

constexpr int TLR_BLOCK = 256;

// A counter slot of the blocking form (refit_launch.h)
struct TlrStats {
    unsigned int innerLinks, leafLinks, err;
    unsigned int pad[13];        // a slot per 64-byte line
};
static_assert(sizeof(TlrStats) == 64, "TlrStats must be 64 bytes");

DeviceScratchPool g_tlrPool;
RefitHeld g_tlrHeld[kMaxDevices];

// Record i (instanced_bvh.h) of an instance whose blas index the caller has checked; range is the table's entry of its BLAS
__device__ __forceinline__ void tlr_write_record(const NtrInstance* __restrict__ inst, int i, const uint4 range, uint4* __restrict__ records)
{
    const uint4* inv = reinterpret_cast<const uint4*>(inst[i].worldToObject);   // 48 bytes into a 112-byte struct of a 16-byte aligned array
    uint4* rec = records + 4 * (size_t)i;
    rec[0] = inv[0];
    rec[1] = inv[1];
    rec[2] = inv[2];
    rec[3] = make_uint4(range.x, range.y, range.z, 0u);
}

// The world box of instance i, whose blas index b the caller has checked, from the pool's current node 0 of BLAS b
__device__ __forceinline__ void tlr_instance_box(const NtrInstance* __restrict__ inst, int i, const uint4 range, const char* __restrict__ poolNodes,
                                                 float (&wlo)[3], float (&whi)[3])
{
    float4 n0, n1, nz;
    tlas_load_node0(poolNodes, range, n0, n1, nz);
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = inst[i].objectToWorld[k];
    tlr_world_box(n0, n1, nz, m, wlo, whi);
}

__global__ __launch_bounds__(TLR_BLOCK) void tlr_prepare(int n, int numSlots, const NtrInstance* __restrict__ inst, int numBlas,
                                                         const uint4* __restrict__ table, const int* __restrict__ nodes,
                                                         uint4* __restrict__ records, unsigned int* __restrict__ parent,
                                                         unsigned int* __restrict__ arrive, TlrStats* __restrict__ stats /* or null */)
{
    const int idx = blockIdx.x * TLR_BLOCK + threadIdx.x;
    unsigned int inner = 0, leaf = 0, err = 0;
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
        const int b = inst[idx].blas;
        if (b < 0 || b >= numBlas) err |= TLAS_ERR_BLAS;
        else tlr_write_record(inst, idx, table[b], records);
    }
    if (!stats) return;
    stats += blockIdx.x % kRefitStatSlots;
    tlas_fold_counters(stats, inner, leaf, err);
}

__global__ __launch_bounds__(TLR_BLOCK) void tlr_climb(int n, int numSlots, const NtrInstance* __restrict__ inst, int numBlas,
                                                       const uint4* __restrict__ table, const char* __restrict__ poolNodes, int* nodes,
                                                       const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                       float* sceneBox /* or null */, float* sceneCopy /* or null: the blocking form's */)
{
    const unsigned int gid = blockIdx.x * (unsigned int)TLR_BLOCK + threadIdx.x;   // < 2 * numSlots + TLR_BLOCK < 2^26
    const int node = (int)(gid >> 1), k = (int)(gid & 1u);
    if (node >= numSlots) return;
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (link >= 0) return;                       // an inner child arrives with the owner of its node; offset 0 is no child at all
    const int i = leaf_row(link);                // >= 0
    if (i >= n) return;                          // after a bad part the nodes above keep an arrival short and stay as they are
    const int b = inst[i].blas;
    if (b < 0 || b >= numBlas) return;
    float wlo[3], whi[3];
    tlr_instance_box(inst, i, table[b], poolNodes, wlo, whi);
    tlas_leaf_climb(node, k, numSlots, nodes, parent, arrive, wlo, whi, sceneBox, sceneCopy);
}

// N == 1: one thread
__global__ __launch_bounds__(64) void tlr_single(const NtrInstance* __restrict__ inst, int numBlas, const uint4* __restrict__ table,
                                                 const char* __restrict__ poolNodes, uint4* __restrict__ records, float* sceneBox /* or null */,
                                                 float* sceneCopy /* or null */, TlrStats* __restrict__ stats /* or null */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int b = inst[0].blas;
    if (b < 0 || b >= numBlas) {
        if (stats) stats->err = TLAS_ERR_BLAS;
        return;
    }
    const uint4 range = table[b];
    tlr_write_record(inst, 0, range, records);
    float wlo[3], whi[3];
    tlr_instance_box(inst, 0, range, poolNodes, wlo, whi);
    tlas_write_scene_box(sceneBox, sceneCopy, wlo, whi);
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_tlas_refit(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                   const void* d_poolNodes, int64_t poolNodesBytes, void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                   void* d_records, int64_t recordsCapacity, float* d_sceneBox, NtrTlasRefitResult* result, void* stream)
{
    const char* fn = "ntr_tlas_refit";
    if (result) memset(result, 0, sizeof(*result));
    const TlasBinaryArgs args = {numInstances, d_instances, numBlas, blasRanges, d_poolNodes, poolNodesBytes, d_tlasNodes, tlasNodesBytes,
                                 rootLink, d_records, recordsCapacity};
    if (const int rc = tlas_binary_check_extents(fn, args)) return rc;
    const int n = numInstances, slots = numInstances - 1;
    const TlasRefitLayout lay(slots, numBlas);
    RefitTable held = {1, {}, {lay.table, 0}, {slots, 0}};
    if (const int rc = tlas_binary_range_table(fn, args, 0, held.words[0])) return rc;

    hipStream_t s = (hipStream_t)stream;
    void* base = nullptr;
    if (const int rc = refit_hold_table(fn, kRefitRangeWords, g_tlrPool, g_tlrHeld, s, result != nullptr, lay.end, held, &base)) return rc;
    uint4* d_table = at<uint4>(base, lay.table);
    unsigned int *parent = at<unsigned int>(base, lay.parent), *arrive = at<unsigned int>(base, lay.arrive);
    TlrStats* stats = result ? at<TlrStats>(base, lay.stats) : nullptr;
    float* sceneCopy = result ? at<float>(base, lay.scene) : nullptr;

    std::vector<char> host;
    float seconds = 0.0f;
    const int rc = refit_bracket(s, result != nullptr, base, lay.zeroBytes, &host, &seconds, [&] {
        if (n == 1) {
            hipLaunchKernelGGL(tlr_single, dim3(1), dim3(64), 0, s, d_instances, (int)numBlas, (const uint4*)d_table, (const char*)d_poolNodes,
                               (uint4*)d_records, d_sceneBox, sceneCopy, stats);
        } else {
            hipLaunchKernelGGL(tlr_prepare, dim3((n + TLR_BLOCK - 1) / TLR_BLOCK), dim3(TLR_BLOCK), 0, s, n, slots, d_instances, (int)numBlas,
                               (const uint4*)d_table, (const int*)d_tlasNodes, (uint4*)d_records, parent, arrive, stats);
            hipLaunchKernelGGL(tlr_climb, dim3((unsigned int)((2ll * slots + TLR_BLOCK - 1) / TLR_BLOCK)), dim3(TLR_BLOCK), 0, s, n, slots, d_instances,
                               (int)numBlas, (const uint4*)d_table, (const char*)d_poolNodes, (int*)d_tlasNodes, (const unsigned int*)parent, arrive,
                               d_sceneBox, sceneCopy);
        }
    });
    if (rc != NTR_OK || !result) return rc;

    uint64_t inner = 0, leafLinks = 0;
    unsigned int err = 0;
    refit_fold_slots<TlrStats>(host.data() + lay.stats, [&](const TlrStats& v) { inner += v.innerLinks; leafLinks += v.leafLinks; err |= v.err; });
    result->numNodes = n == 1 ? 0 : (int32_t)(1 + inner);
    result->numLeaves = n == 1 ? 1 : (int32_t)leafLinks;
    result->errBits = (int32_t)err;
    memcpy(result->sceneMin, host.data() + lay.scene, 3 * sizeof(float));
    memcpy(result->sceneMax, host.data() + lay.scene + 3 * sizeof(float), 3 * sizeof(float));
    result->seconds = seconds;
    if (err & TLAS_ERR_BLAS)
        return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d) (error bits 0x%x); its record, its leaf box and "
                         "the boxes above it were left as they were, everything else was refitted", fn, (int)numBlas, err);
    if (err)
        return set_error(NTR_ERR_LAYOUT, "%s: malformed top-level tree (error bits 0x%x: 2 a child link that names no slot, 4 a leaf link "
                         "beyond the instances); the boxes above such a place were left as they were, everything else was refitted", fn, err);
    return NTR_OK;
}

int ntr_tlas_refit_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_refit_scratch_bytes", g_tlrPool, bytes); }

}  // extern "C"
