// bvh_optimize_kernels.hip -- on-device treelet restructuring (ntr_bvh_optimize) and SAH cost (ntr_bvh_sah_cost) of a
// BVHLayout_Compact tree for gfx950.
//
// ntr_bvh_optimize is an EXTENSION: the reference has no treelet restructuring.  The rule is the numpy spec tests/np_bvh_optimize.py,
// whose docstring is the normative text (the treelet part of Karras and Aila, HPG 2013, treelet size 7); the header comment of
// ntr_bvh_optimize (include/ntrace_amd.h) restates the contract.  ntr_bvh_sah_cost restates the reference's calcSAHNode
// (emitTreeKernel.cu:1361-1391, host HLBVHBuilder::calcSAHGPU, HLBVHBuilder.cpp:752-770) in strict binary32, as a parallel bottom-up
// pass instead of one thread's recursion.
//
// Shape of a pass of the optimiser:
//   opt_topology      one thread per node slot: the topology step of bvh_climb.h; clears the slot's height and histogram word
//   opt_climb<false>  one thread per child word that is a leaf link: the climb of bvh_climb.h with the payload (height 0, 1 leaf
//                     link); the owner of a node stores its height (1 + max) and leaf links (sum).  Integers only, so arrival order
//                     cannot matter.  The layout is compact_bvh.h's; the arrival protocol is stated in bvh_climb.h and lives only there
//   opt_histogram     one thread per slot with leafLinks >= 7 walks its parent words up to the root (only reached slots root a
//                     treelet) and counts itself under its height
//   opt_scan, opt_scatter  the roots into per-height lists (the scan reads the root's height on the device); then the host reads the
//                     root's report and the histogram back, the one read-back of a pass: it sizes the launches
//   opt_treelets      one launch per height that has roots, one wave64 (one workgroup) per treelet: formation (five dependent 64-byte
//                     record reads), the seven boxes in the ord_enc encoding in LDS, each lane the areas of subsets lane and
//                     lane + 64, the dynamic programme size by size on a 128-entry cost table and a 128-byte choice table, the cost
//                     of the existing topology, and, if the programme's is strictly lower, six records written with vector stores.
//                     Waves of one launch touch disjoint slots; the kernel boundary orders the heights.
// ntr_bvh_sah_cost is opt_topology + opt_climb<true>: a leaf thread counts its triangles to the terminator, the second arrival
// computes the node's value from its two children's; the root's value, height and counts are read back.
// A link outside the extent is never followed (it counts as a leaf link and sets an error bit), so nothing outside the caller's
// buffer is touched; a node reached by more than two arrivals (not a tree) is owned once, so every pass ends on any input.
// The device code of every step but the topology's lives in bvh_optimize_payload.h (the climb and what it carries) and
// bvh_optimize_treelet.h (histogram, scan, scatter, the treelet), which bvh_optimize_batch_kernels.hip runs over the BLASes of a pool
// (DESIGN.md 6v); the kernels here find their slot and call those bodies.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "bvh_optimize_payload.h"
#include "bvh_optimize_treelet.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {
namespace {

DeviceScratchPool g_opPool;

__global__ __launch_bounds__(OP_BLOCK) void opt_topology(int numSlots, const int* __restrict__ nodes, unsigned int* __restrict__ parent,
                                                         unsigned int* __restrict__ arrive, int* __restrict__ height /* or null */,
                                                         unsigned int* __restrict__ hist /* numSlots + 1 words, or null */,
                                                         OpRoot* __restrict__ root)
{
    const int node = blockIdx.x * OP_BLOCK + threadIdx.x;
    if (node > numSlots) return;
    if (hist) hist[node] = 0u;
    if (node == numSlots) return;
    if (height) height[node] = 0;
    int kind[2];
    topology_slot(node, numSlots, nodes, parent, arrive, kind);
    if (kind[0] == LINK_BAD || kind[1] == LINK_BAD) atomicOr(&root->err, OP_ERR_LINK);   // a malformed tree only
}

// The payload, its stores and loads and the climb of a child word are bvh_optimize_payload.h's.
template <bool SAH>
__global__ __launch_bounds__(OP_BLOCK) void opt_climb(int numSlots, const int* __restrict__ nodes, int numRows, const float4* __restrict__ woop,
                                                      const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                      unsigned long long* __restrict__ info, int* __restrict__ height,
                                                      unsigned int* __restrict__ leafLinks, OpRoot* __restrict__ root)
{
    const long long g = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (g >= 2ll * numSlots) return;
    op_climb_child<SAH>((int)(g >> 1), (int)(g & 1), numSlots, nodes, numRows, woop, parent, arrive, info, height, leafLinks, root, nullptr);
}

// qual[slot] = the slot's height if it roots a treelet (reached, leafLinks >= 7), else 0; hist[height] counts them.
__global__ __launch_bounds__(OP_BLOCK) void opt_histogram(int numSlots, const int* __restrict__ nodes, const unsigned int* __restrict__ parent,
                                                          const int* __restrict__ height, const unsigned int* __restrict__ leafLinks,
                                                          int* __restrict__ qual, unsigned int* __restrict__ hist)
{
    const int slot = blockIdx.x * OP_BLOCK + threadIdx.x;
    op_histogram_body(slot < numSlots, slot, numSlots, nodes, parent, height, leafLinks, qual + slot, hist);
}

// cursor[h] = the exclusive scan of hist[0 .. root->height]: one workgroup, which reads the height the climb has just reported, so the
// host needs no read-back between the histogram and the scatter
__global__ __launch_bounds__(OP_BLOCK) void opt_scan(int numSlots, const OpRoot* __restrict__ root, const unsigned int* __restrict__ hist,
                                                     unsigned int* __restrict__ cursor)
{
    op_scan_body(root->done ? min((int)root->height, numSlots) + 1 : 0, hist, cursor);
}

__global__ __launch_bounds__(OP_BLOCK) void opt_scatter(int numSlots, const int* __restrict__ qual, unsigned int* __restrict__ cursor,
                                                        int* __restrict__ list)
{
    op_scatter_body(numSlots, qual, cursor, list);
}

// One wave64 (one workgroup) per treelet (bvh_optimize_treelet.h)
__global__ __launch_bounds__(64) void opt_treelets(int numSlots, int* __restrict__ nodes, const int* __restrict__ roots, int count,
                                                   unsigned int* __restrict__ rewritten)
{
    if ((int)blockIdx.x >= count) return;
    const int R = roots[blockIdx.x];
    if (R < 0 || R >= numSlots) return;
    op_treelet_body(numSlots, nodes, R, rewritten);
}

struct OpLayout {
    size_t root, stats, parent, arrive, info, height, leafLinks, qual, hist, cursor, list, end;
    OpLayout(int64_t slots, bool sah)
    {
        ScratchCarver c;
        root = c.take(sizeof(OpRoot));
        stats = c.take(sizeof(unsigned int) * OP_STAT_SLOTS * OP_MAX_PASSES);
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        info = c.take((size_t)slots * 2 * 8 * (sah ? 3 : 1));
        height = leafLinks = qual = hist = cursor = list = c.off;
        if (!sah) {
            height = c.take((size_t)slots * 4);
            leafLinks = c.take((size_t)slots * 4);
            qual = c.take((size_t)slots * 4);
            hist = c.take((size_t)(slots + 1) * 4);
            cursor = c.take((size_t)(slots + 1) * 4);
            list = c.take((size_t)slots * 4);
        }
        end = c.off;
    }
};

int check_nodes(const char* fn, const void* d_nodes, int64_t nodesBytes)
{
    if (!d_nodes) return set_error(NTR_ERR_INVALID, "%s: null d_nodes", fn);
    return check_nodes_bytes(fn, "nodesBytes", nodesBytes);
}

// opt_topology + opt_climb on stream s, then the root's report read back (blocks)
template <bool SAH>
int run_climb(hipStream_t s, int numSlots, const int* d_nodes, int numRows, const float4* d_woop, char* base, const OpLayout& lay, OpRoot* h)
{
    auto P = [&](size_t o) { return base + o; };
    OpRoot* root = (OpRoot*)P(lay.root);
    NTR_HIP(hipMemsetAsync(root, 0, sizeof(OpRoot), s));
    hipLaunchKernelGGL(opt_topology, dim3((numSlots + 1 + OP_BLOCK - 1) / OP_BLOCK), dim3(OP_BLOCK), 0, s, numSlots, d_nodes,
                       (unsigned int*)P(lay.parent), (unsigned int*)P(lay.arrive), SAH ? (int*)nullptr : (int*)P(lay.height),
                       SAH ? (unsigned int*)nullptr : (unsigned int*)P(lay.hist), root);
    hipLaunchKernelGGL(opt_climb<SAH>, dim3((unsigned int)((2ll * numSlots + OP_BLOCK - 1) / OP_BLOCK)), dim3(OP_BLOCK), 0, s, numSlots, d_nodes,
                       numRows, d_woop, (const unsigned int*)P(lay.parent), (unsigned int*)P(lay.arrive), (unsigned long long*)P(lay.info),
                       (int*)P(lay.height), (unsigned int*)P(lay.leafLinks), root);
    NTR_HIP(hipGetLastError());
    if (!h) return NTR_OK;
    NTR_HIP(hipMemcpyAsync(h, root, sizeof(OpRoot), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_optimize(void* d_nodes, int64_t nodesBytes, int32_t passes, NtrBvhOptimizeResult* result, void* stream)
{
    if (result) memset(result, 0, sizeof(*result));
    {
        const int rc = check_nodes("ntr_bvh_optimize", d_nodes, nodesBytes);
        if (rc != NTR_OK) return rc;
    }
    if (passes < 1 || passes > OP_MAX_PASSES) return set_error(NTR_ERR_INVALID, "ntr_bvh_optimize: passes must be in 1..8");
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "ntr_bvh_optimize: the call reads back per pass and cannot be captured");

    const int numSlots = (int)(nodesBytes / 64);
    const OpLayout lay(numSlots, false);
    void* basev = nullptr;
    {
        const int rc = g_opPool.reserve(lay.end, &basev);
        if (rc != NTR_OK) return rc;
    }
    char* base = (char*)basev;
    auto P = [&](size_t o) { return base + o; };
    unsigned int* d_stats = (unsigned int*)P(lay.stats);
    const dim3 slotGrid((numSlots + OP_BLOCK - 1) / OP_BLOCK);

    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    NTR_HIP(hipMemsetAsync(d_stats, 0, sizeof(unsigned int) * OP_STAT_SLOTS * OP_MAX_PASSES, s));
    NtrBvhOptimizeResult res = NtrBvhOptimizeResult();
    res.passes = passes;
    unsigned int err = 0;
    OpRoot h;
    std::vector<unsigned int> hist;
    for (int pass = 0; pass <= passes; pass++) {   // the last round only measures the height after the last pass
        const bool last = pass == passes;
        {
            const int rc = run_climb<false>(s, numSlots, (const int*)d_nodes, 0, nullptr, base, lay, last ? &h : nullptr);
            if (rc != NTR_OK) return rc;
        }
        if (last) {
            err |= h.err;
            if (!h.done) return set_error(NTR_ERR_LAYOUT, "ntr_bvh_optimize: the child links do not form a tree under slot 0");
            res.heightAfter[pass - 1] = (int32_t)h.height;
            break;
        }
        hipLaunchKernelGGL(opt_histogram, slotGrid, dim3(OP_BLOCK), 0, s, numSlots, (const int*)d_nodes, (const unsigned int*)P(lay.parent),
                           (const int*)P(lay.height), (const unsigned int*)P(lay.leafLinks), (int*)P(lay.qual), (unsigned int*)P(lay.hist));
        hipLaunchKernelGGL(opt_scan, dim3(1), dim3(OP_BLOCK), 0, s, numSlots, (const OpRoot*)P(lay.root), (const unsigned int*)P(lay.hist),
                           (unsigned int*)P(lay.cursor));
        hipLaunchKernelGGL(opt_scatter, slotGrid, dim3(OP_BLOCK), 0, s, numSlots, (const int*)P(lay.qual), (unsigned int*)P(lay.cursor),
                           (int*)P(lay.list));
        NTR_HIP(hipGetLastError());
        // the one read-back of a pass: the root's report and the histogram's first words together, the rest only for a taller tree
        const size_t firstWords = std::min<size_t>((size_t)numSlots + 1, OP_HIST_LDS);
        hist.assign(firstWords, 0u);
        NTR_HIP(hipMemcpyAsync(&h, P(lay.root), sizeof(OpRoot), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipMemcpyAsync(hist.data(), P(lay.hist), sizeof(unsigned int) * firstWords, hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        err |= h.err;
        if (!h.done) return set_error(NTR_ERR_LAYOUT, "ntr_bvh_optimize: the child links do not form a tree under slot 0");
        if (pass > 0) res.heightAfter[pass - 1] = (int32_t)h.height;
        res.heightBefore[pass] = (int32_t)h.height;
        res.numNodes = (int32_t)(h.leafLinks - 1u);
        res.numLeafLinks = (int32_t)h.leafLinks;
        const int H = (int)h.height;             // 1 .. numSlots
        if (H < 1 || H > numSlots) return set_error(NTR_ERR_LAYOUT, "ntr_bvh_optimize: impossible tree height %d", H);
        if ((size_t)H + 1 > firstWords) {
            hist.assign((size_t)H + 1, 0u);
            NTR_HIP(hipMemcpyAsync(hist.data(), P(lay.hist), sizeof(unsigned int) * ((size_t)H + 1), hipMemcpyDeviceToHost, s));
            NTR_HIP(hipStreamSynchronize(s));
        }
        size_t off = 0;
        for (int hgt = 0; hgt <= H; hgt++) {
            const unsigned int cnt = hist[hgt];
            if (off + cnt > (size_t)numSlots) return set_error(NTR_ERR_HIP, "ntr_bvh_optimize: inconsistent height histogram");
            if (cnt && hgt > 0)
                hipLaunchKernelGGL(opt_treelets, dim3(cnt), dim3(64), 0, s, numSlots, (int*)d_nodes, (const int*)P(lay.list) + off, (int)cnt,
                                   d_stats + (size_t)pass * OP_STAT_SLOTS);
            off += cnt;
        }
        NTR_HIP(hipGetLastError());
        res.formed[pass] = (int32_t)off;
    }
    NTR_HIP(ev.record(1));
    unsigned int stats[OP_STAT_SLOTS * OP_MAX_PASSES];
    NTR_HIP(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    for (int pass = 0; pass < passes; pass++)
        for (int i = 0; i < OP_STAT_SLOTS; i++) res.rewritten[pass] += (int32_t)stats[pass * OP_STAT_SLOTS + i];
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    res.seconds = ms * 1e-3f;
    if (result) *result = res;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "ntr_bvh_optimize: malformed tree (a child link outside the node extent); such a link was treated "
                         "as a leaf link and never followed");
    return NTR_OK;
}

int ntr_bvh_optimize_scratch_bytes(int64_t* bytes)
{
    if (!bytes) return set_error(NTR_ERR_INVALID, "ntr_bvh_optimize_scratch_bytes: null");
    *bytes = (int64_t)g_opPool.held();
    return NTR_OK;
}

int ntr_bvh_sah_cost(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes, NtrBvhSahResult* result, void* stream)
{
    if (result) memset(result, 0, sizeof(*result));
    {
        const int rc = check_nodes("ntr_bvh_sah_cost", d_nodes, nodesBytes);
        if (rc != NTR_OK) return rc;
    }
    if (!d_triWoop) return set_error(NTR_ERR_INVALID, "ntr_bvh_sah_cost: null d_triWoop");
    if (triWoopBytes < 16 || (triWoopBytes % 16) != 0 || triWoopBytes / 16 > INT_MAX)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_sah_cost: triWoopBytes must be a positive multiple of 16 (at most 2^31 - 1 rows)");
    if (!result) return set_error(NTR_ERR_INVALID, "ntr_bvh_sah_cost: null result");
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "ntr_bvh_sah_cost: the call reads its result back and cannot be captured");

    const int numSlots = (int)(nodesBytes / 64), numRows = (int)(triWoopBytes / 16);
    const OpLayout lay(numSlots, true);
    void* basev = nullptr;
    {
        const int rc = g_opPool.reserve(lay.end, &basev);
        if (rc != NTR_OK) return rc;
    }
    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    OpRoot h;
    {
        const int rc = run_climb<true>(s, numSlots, (const int*)d_nodes, numRows, (const float4*)d_triWoop, (char*)basev, lay, nullptr);
        if (rc != NTR_OK) return rc;
    }
    NTR_HIP(ev.record(1));
    NTR_HIP(hipMemcpyAsync(&h, (char*)basev + lay.root, sizeof(OpRoot), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    if (!h.done) return set_error(NTR_ERR_LAYOUT, "ntr_bvh_sah_cost: the child links do not form a tree under slot 0");
    result->sahCost = h.sah;
    result->numNodes = (int32_t)h.slots;
    result->numLeaves = (int32_t)h.leaves;
    result->numTris = (int32_t)h.tris;
    result->height = (int32_t)h.height;
    result->seconds = ms * 1e-3f;
    if (h.err)
        return set_error(NTR_ERR_LAYOUT, "ntr_bvh_sah_cost: malformed tree (error 0x%x: 1 child link, 2 leaf row outside the extents); such "
                         "a child counts as 0", h.err);
    return NTR_OK;
}

}  // extern "C"
