// bvh_reorder_kernels.hip -- on-device renumbering of a BVHLayout_Compact tree into the host builder's node and row order for gfx950
// (ntr_bvh_reorder).
//
// The order is the one CudaBVH::createCompact's walk gives (CudaBVH.cpp:594-652): siblings adjacent, a node's direct leaves before
// everything below it, child 1's subtree before child 0's.  The rule is the numpy spec tests/np_bvh_reorder.py, whose docstring is the
// normative text; the header comment of ntr_bvh_reorder (include/ntrace_amd.h) restates the contract.  The pass is out of place: the
// input tree is only read.  The spec's closed form is what is computed here: with I(v) the inner nodes and W(v) the leaf rows below v,
// the walk's counters at the moment v is popped are f(v) = 1 + the sum of df over v's parent chain, g(v) = the sum of dg, where for
// child slot (p, k) of a node p with a inner children and d rows in direct leaves
//   df(p, 1) = a              dg(p, 1) = d
//   df(p, 0) = a + (c1 inner ? I(c1) - 1 : 0)        dg(p, 0) = d + (c1 inner ? W(c1) : 0)
//
// Shape: five launches with kernel boundaries between the phases, one read-back (the totals and the error word) before the copies.
//   ro_topology    a thread per slot: the topology step of bvh_climb.h; clears the slot's srcOf and newLink words
//   ro_climb       a thread per child slot that holds no inner link: measures its leaf (rows ~link + 3j up to the terminator, inside
//                  the extent), publishes {I, W} = {0, rows} and climbs (bvh_climb.h); the second arrival at a node writes the node's
//                  two (df, dg) words, sums and carries {I, W} up; the owner of slot 0 writes the totals
//   ro_place       a thread per slot: walks parent[] to the root (parent_links_back at each step, at most numSlots steps; a slot that
//                  does not get there is unreached and is dropped), adding one 8-byte (df, dg) per ancestor; writes newLink[2v + k]
//                  for both children and srcOf[new slot] for its inner children (slot 0 for itself); counts leaf links and errors
//   ro_copy_nodes  four lanes per destination slot: a 16-byte load from node srcOf[dst] and a 16-byte store each; the lane of words
//                  12-15 substitutes the two links
//   ro_copy_rows   four lanes per leaf link of a reached slot: rows by 16-byte accesses, triIndex words beside them
// The only exchange inside a launch is the arrival protocol of bvh_climb.h with the payload {I, W} as one 8-byte word, published and
// read at agent scope as the refit's boxes are.  Everything else a kernel reads was written by an earlier launch or by nobody.
// Nothing loops without a bound and nobody waits for another workgroup, so the call ends on any input.  A malformed input (a link
// outside the extents, a leaf without a terminator, links that form no tree) is never followed, and no destination outside
// [0, numNodes) x [0, numRows) -- the totals the host has checked against the capacities -- is ever written.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {
namespace {

constexpr int RO_BLOCK = 256;
constexpr int RO_ROW_LANES = 4;              // lanes per leaf link in ro_copy_rows: most leaves are one triangle, four rows
constexpr int RO_STAT_SLOTS = 256;           // ro_place's counters: a workgroup adds to slot blockIdx % 256 (as RfStats)
enum : unsigned int { RO_ERR_LINK = 1u, RO_ERR_ROW = 2u };

struct RoStat {
    unsigned int leaves, err;
    unsigned int pad[14];                    // a slot per 64-byte line
};
struct RoReport {                            // read back once: what the owner of slot 0 reports, then ro_place's counters
    unsigned int done, nodes, rows;          // done stays 0 if the climb never reached slot 0; nodes and rows saturate at 2^32 - 1
    unsigned int pad[13];
    RoStat stat[RO_STAT_SLOTS];
};
static_assert(sizeof(RoStat) == 64 && sizeof(RoReport) == 64 * (1 + RO_STAT_SLOTS), "RoReport is 64-byte records");

DeviceScratchPool g_roPool;

__device__ __forceinline__ unsigned int sat_add(unsigned int a, unsigned int b)
{
    const unsigned long long s = (unsigned long long)a + b;
    return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned int)s;
}
__device__ __forceinline__ unsigned long long pack2(unsigned int lo, unsigned int hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); }

__global__ __launch_bounds__(RO_BLOCK) void ro_topology(int numSlots, const int* __restrict__ nodes, unsigned int* __restrict__ parent,
                                                        unsigned int* __restrict__ arrive, int* __restrict__ srcOf, int2* __restrict__ newLink)
{
    const int node = blockIdx.x * RO_BLOCK + threadIdx.x;
    if (node >= numSlots) return;
    int kind[2];
    topology_slot(node, numSlots, nodes, parent, arrive, kind);
    srcOf[node] = -1;                            // a destination slot nobody claims is left alone
    newLink[node] = make_int2(0, 0);             // ro_copy_rows takes a negative word for a leaf of a reached slot
}

// info[2 * node + k] is child slot (node, k)'s payload: {I, W} of an inner child, {leaf without a terminator ? 1 : 0, rows} of a leaf,
// {0, 0} of a child word 0 or a malformed link.  delta[2 * node + k] = {df, dg} is written by the node's owner.
__global__ __launch_bounds__(RO_BLOCK) void ro_climb(int numSlots, const int* __restrict__ nodes, int numRows, const uint4* __restrict__ woop,
                                                     const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                     unsigned long long* __restrict__ info, unsigned long long* __restrict__ delta,
                                                     RoReport* __restrict__ report)
{
    const long long g = (long long)blockIdx.x * RO_BLOCK + threadIdx.x;
    if (g >= 2ll * numSlots) return;
    const int node = (int)(g >> 1), k = (int)(g & 1);
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (is_inner_link(link, numSlots)) return;   // an inner child arrives with the owner of its node
    unsigned int mineI = 0u, mineW = 0u, sibI = 0u, sibW = 0u;
    unsigned int flag = 0u;
    if (link < 0) {
        long long r = (long long)leaf_row(link);
        while (r < numRows && woop[r].x != kLeafTerm) r += 3;   // only a triangle's first row is tested; at most numRows / 3 steps
        if (r < numRows) {
            mineW = (unsigned int)(r - (long long)leaf_row(link)) + 1u;
        } else {                                 // no terminator inside the extent: emitted as a lone terminator row
            mineW = 1u;
            flag = 1u;
        }
    }
    const auto publish = [&](int n, int ck) {
        __hip_atomic_store(info + 2 * (size_t)n + ck, pack2(mineI, mineW), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const auto acquire = [&](int n, int ck) {
        const unsigned long long v = __hip_atomic_load(info + 2 * (size_t)n + ck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sibI = (unsigned int)v;
        sibW = (unsigned int)(v >> 32);
    };
    const auto merge = [&](int n, int ck) {
        const int2 c = *reinterpret_cast<const int2*>(nodes + (size_t)n * kNodeWords + kLinkWord);   // nobody writes the input tree
        const bool in0 = is_inner_link(c.x, numSlots), in1 = is_inner_link(c.y, numSlots);
        const unsigned int i0 = ck == 0 ? mineI : sibI, w0 = ck == 0 ? mineW : sibW;
        const unsigned int i1 = ck == 0 ? sibI : mineI, w1 = ck == 0 ? sibW : mineW;
        const unsigned int a = (in0 ? 1u : 0u) + (in1 ? 1u : 0u);
        const unsigned int d = sat_add(in0 ? 0u : w0, in1 ? 0u : w1);
        // read by ro_place, a later launch: plain stores
        delta[2 * (size_t)n] = pack2(sat_add(a, in1 ? i1 - 1u : 0u), sat_add(d, in1 ? w1 : 0u));
        delta[2 * (size_t)n + 1] = pack2(a, d);
        mineI = sat_add(1u, sat_add(in0 ? i0 : 0u, in1 ? i1 : 0u));   // a leaf's first word is its flag, not a count
        mineW = sat_add(w0, w1);
        if (n == 0) {                            // the root reports to no parent
            report->nodes = mineI;
            report->rows = mineW;
            report->done = 1u;
        }
    };
    __hip_atomic_store(info + (size_t)g, pack2(flag, mineW), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    climb(node, k, numSlots, nodes, parent, arrive, publish, acquire, merge);
}

__global__ __launch_bounds__(RO_BLOCK) void ro_place(int numSlots, const int* __restrict__ nodes, const unsigned int* __restrict__ parent,
                                                     const unsigned long long* __restrict__ info, const unsigned long long* __restrict__ delta,
                                                     int* __restrict__ srcOf, int2* __restrict__ newLink, RoReport* __restrict__ report)
{
    const int v = blockIdx.x * RO_BLOCK + threadIdx.x;
    unsigned int leaves = 0u, err = 0u;
    if (v < numSlots) {
        unsigned long long f = 1ull, g = 0ull;   // 64-bit sums of saturated 32-bit words: no wrap within numSlots steps
        int n = v, steps = 0;
        for (; n != 0 && steps < numSlots; steps++) {
            const unsigned int p = parent[n];
            if (!parent_links_back(p, n, numSlots, nodes)) break;
            const unsigned long long dl = delta[p];   // p = 2 * parent + k < 2 * numSlots
            f += (unsigned int)dl;
            g += dl >> 32;
            n = (int)(p >> 1);
        }
        if (n == 0) {                            // reached
            const int2 c = *reinterpret_cast<const int2*>(nodes + (size_t)v * kNodeWords + kLinkWord);
            const int link[2] = {c.x, c.y};
            const bool in0 = is_inner_link(c.x, numSlots);
            const unsigned long long d0 = c.x < 0 ? info[2 * (size_t)v] >> 32 : 0ull;
            int out[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (is_inner_link(link[k], numSlots)) {
                    const unsigned long long slot = f + (k == 1 && in0 ? 1ull : 0ull);
                    out[k] = slot < (unsigned long long)kMaxNodes ? inner_link((int)slot) : 0;   // beyond: the host reports an overflow
                    if (slot < (unsigned long long)numSlots) srcOf[slot] = inner_index(link[k]);
                } else if (link[k] < 0) {
                    const unsigned long long row = g + (k == 1 ? d0 : 0ull);
                    out[k] = leaf_link(row <= (unsigned long long)INT_MAX ? (int)row : INT_MAX);
                    leaves++;
                    if ((unsigned int)info[2 * (size_t)v + k]) err |= RO_ERR_ROW;
                } else {
                    out[k] = link[k];            // 0, or a malformed link: copied unchanged
                    if (link[k] != 0) err |= RO_ERR_LINK;
                }
            }
            newLink[v] = make_int2(out[0], out[1]);
            if (v == 0) srcOf[0] = 0;
        }
    }
    RoStat* mine = report->stat + blockIdx.x % RO_STAT_SLOTS;
    leaves = wave_sum_u32(leaves);
    err = wave_or_u32(err);
    if ((threadIdx.x & 63) == 0) {
        if (leaves) atomicAdd(&mine->leaves, leaves);
        if (err) atomicOr(&mine->err, err);
    }
}

__global__ __launch_bounds__(RO_BLOCK) void ro_copy_nodes(int numNodes, int numSlots, const uint4* __restrict__ nodes, const int* __restrict__ srcOf,
                                                          const int2* __restrict__ newLink, uint4* __restrict__ outNodes)
{
    const long long t = (long long)blockIdx.x * RO_BLOCK + threadIdx.x;
    const long long dst = t >> 2;
    const int q = (int)(t & 3);
    if (dst >= numNodes) return;                 // numNodes <= numSlots and <= the output's capacity (the host has checked)
    const int src = srcOf[dst];
    if (src < 0 || src >= numSlots) return;      // not a tree: nobody claimed this slot
    uint4 w = nodes[(size_t)src * 4 + q];
    if (q == 3) {
        const int2 l = newLink[src];
        w.x = (unsigned int)l.x;
        w.y = (unsigned int)l.y;
    }
    outNodes[(size_t)dst * 4 + q] = w;
}

__global__ __launch_bounds__(RO_BLOCK) void ro_copy_rows(int numSlots, const int* __restrict__ nodes, int numRows, const uint4* __restrict__ woop,
                                                         const int* __restrict__ triIndex, const unsigned long long* __restrict__ info,
                                                         const int* __restrict__ newLink /* 2 per slot */, long long outRows,
                                                         uint4* __restrict__ outWoop, int* __restrict__ outTriIndex)
{
    const long long t = (long long)blockIdx.x * RO_BLOCK + threadIdx.x;
    const long long g = t / RO_ROW_LANES;
    const int sub = (int)(t % RO_ROW_LANES);
    if (g >= 2ll * numSlots) return;
    const int nl = newLink[g];
    if (nl >= 0) return;                         // no leaf link of a reached slot
    const int link = nodes[(size_t)(g >> 1) * kNodeWords + kLinkWord + (g & 1)];
    if (link >= 0) return;                       // (a reached slot's newLink is negative only for a leaf link)
    const unsigned long long pay = info[g];
    const long long src = (long long)leaf_row(link), dst = (long long)leaf_row(nl), len = (long long)(pay >> 32);
    if (dst + len > outRows) return;             // not a tree: the totals do not cover this link
    if ((unsigned int)pay) {                     // a leaf without a terminator: a lone terminator row
        if (sub == 0) {
            outWoop[dst] = make_uint4(kLeafTerm, kLeafTerm, kLeafTerm, kLeafTerm);
            outTriIndex[dst] = 0;
        }
        return;
    }
    if (src + len > numRows) return;             // cannot happen: ro_climb measured inside the extent
    for (long long j = sub; j < len; j += RO_ROW_LANES) {
        outWoop[dst + j] = woop[src + j];
        outTriIndex[dst + j] = triIndex[src + j];
    }
}

struct RoLayout {
    size_t report, parent, arrive, info, delta, srcOf, newLink, end;
    explicit RoLayout(int64_t slots)
    {
        ScratchCarver c;
        report = c.take(sizeof(RoReport));
        parent = c.take((size_t)slots * 4);
        arrive = c.take((size_t)slots * 4);
        info = c.take((size_t)slots * 2 * 8);
        delta = c.take((size_t)slots * 2 * 8);
        srcOf = c.take((size_t)slots * 4);
        newLink = c.take((size_t)slots * 8);
        end = c.off;
    }
};

bool ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bn && b0 < a0 + (uintptr_t)an;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_bvh_reorder(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                    int64_t triIndexBytes, void* d_outNodes, int64_t outNodesCapacity, void* d_outTriWoop, int64_t outTriWoopCapacity,
                    int32_t* d_outTriIndex, int64_t outTriIndexCapacity, NtrBvhReorderResult* result, void* stream)
{
    if (result) memset(result, 0, sizeof(*result));
    if (!d_nodes) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_nodes");
    if (const int rc = check_nodes_bytes("ntr_bvh_reorder", "nodesBytes", nodesBytes)) return rc;
    if (!d_triWoop) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_triWoop");
    if (triWoopBytes < 16 || (triWoopBytes % 16) != 0 || triWoopBytes / 16 > INT_MAX)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: triWoopBytes must be a positive multiple of 16 (at most 2^31 - 1 rows)");
    if (!d_triIndex) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_triIndex");
    if (triIndexBytes < 0 || triIndexBytes * 4 < triWoopBytes)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: triIndexBytes must cover one entry per Woop row (triIndexBytes * 4 >= triWoopBytes)");
    if (!d_outNodes) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_outNodes");
    if (!d_outTriWoop) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_outTriWoop");
    if (!d_outTriIndex) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null d_outTriIndex");
    if (outNodesCapacity <= 0) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: outNodesCapacity must be positive");
    if (outTriWoopCapacity <= 0) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: outTriWoopCapacity must be positive");
    if (outTriIndexCapacity <= 0) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: outTriIndexCapacity must be positive");
    if (!result) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: null result");
    {
        const void* in[3] = {d_nodes, d_triWoop, d_triIndex};
        const int64_t inBytes[3] = {nodesBytes, triWoopBytes, triIndexBytes};
        const void* out[3] = {d_outNodes, d_outTriWoop, d_outTriIndex};
        const int64_t outBytes[3] = {outNodesCapacity, outTriWoopCapacity, outTriIndexCapacity};
        static const char* const inName[3] = {"d_nodes", "d_triWoop", "d_triIndex"};
        static const char* const outName[3] = {"d_outNodes", "d_outTriWoop", "d_outTriIndex"};
        for (int o = 0; o < 3; o++) {
            for (int i = 0; i < 3; i++)
                if (ranges_overlap(out[o], outBytes[o], in[i], inBytes[i]))
                    return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: %s overlaps %s (the pass is out of place)", outName[o], inName[i]);
            for (int p = 0; p < o; p++)
                if (ranges_overlap(out[o], outBytes[o], out[p], outBytes[p]))
                    return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: %s overlaps %s", outName[o], outName[p]);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder: the call reads its totals back and cannot be captured");

    const int numSlots = (int)(nodesBytes / 64), numRows = (int)(triWoopBytes / 16);
    const int64_t nodeCap = std::min<int64_t>(outNodesCapacity / kNodeBytes, kMaxNodes);
    const int64_t rowCap = std::min<int64_t>(std::min<int64_t>(outTriWoopCapacity / 16, outTriIndexCapacity / 4), INT_MAX);
    const RoLayout lay(numSlots);
    void* base = nullptr;
    {
        const int rc = g_roPool.reserve(lay.end, &base);
        if (rc != NTR_OK) return rc;
    }
    auto P = [&](size_t o) { return (char*)base + o; };
    RoReport* report = (RoReport*)P(lay.report);
    unsigned int* parent = (unsigned int*)P(lay.parent);
    unsigned int* arrive = (unsigned int*)P(lay.arrive);
    unsigned long long* info = (unsigned long long*)P(lay.info);
    unsigned long long* delta = (unsigned long long*)P(lay.delta);
    int* srcOf = (int*)P(lay.srcOf);
    int2* newLink = (int2*)P(lay.newLink);
    const dim3 slotGrid((numSlots + RO_BLOCK - 1) / RO_BLOCK), block(RO_BLOCK);
    const dim3 linkGrid((unsigned int)((2ll * numSlots + RO_BLOCK - 1) / RO_BLOCK));

    StreamEvents<2> ev(s);
    NTR_HIP(ev.create());
    NTR_HIP(ev.record(0));
    NTR_HIP(hipMemsetAsync(report, 0, sizeof(RoReport), s));
    hipLaunchKernelGGL(ro_topology, slotGrid, block, 0, s, numSlots, (const int*)d_nodes, parent, arrive, srcOf, newLink);
    hipLaunchKernelGGL(ro_climb, linkGrid, block, 0, s, numSlots, (const int*)d_nodes, numRows, (const uint4*)d_triWoop,
                       (const unsigned int*)parent, arrive, info, delta, report);
    hipLaunchKernelGGL(ro_place, slotGrid, block, 0, s, numSlots, (const int*)d_nodes, (const unsigned int*)parent,
                       (const unsigned long long*)info, (const unsigned long long*)delta, srcOf, newLink, report);
    NTR_HIP(hipGetLastError());
    static RoReport h;                       // one caller per device at a time, and the copy is waited for right here
    static std::mutex hMu;
    std::lock_guard<std::mutex> lk(hMu);
    NTR_HIP(hipMemcpyAsync(&h, report, sizeof(RoReport), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    if (!h.done) return set_error(NTR_ERR_LAYOUT, "ntr_bvh_reorder: the child links do not form a tree under slot 0; nothing was written");
    unsigned int leaves = 0, err = 0;
    for (const RoStat& v : h.stat) { leaves += v.leaves; err |= v.err; }
    if ((int64_t)h.nodes > (int64_t)numSlots)
        return set_error(NTR_ERR_LAYOUT, "ntr_bvh_reorder: a node slot is named by more than one link; nothing was written");
    result->numNodes = (int32_t)h.nodes;
    result->numLeaves = (int32_t)std::min<unsigned int>(leaves, (unsigned int)INT_MAX);
    result->numRows = (int32_t)std::min<unsigned int>(h.rows, (unsigned int)INT_MAX);
    result->numDroppedSlots = numSlots - (int32_t)h.nodes;
    result->nodesBytes = (int64_t)h.nodes * kNodeBytes;
    result->triWoopBytes = (int64_t)h.rows * 16;
    result->triIndexBytes = (int64_t)h.rows * 4;
    if ((int64_t)h.nodes > nodeCap || (int64_t)h.rows > rowCap)
        return set_error(NTR_ERR_OVERFLOW, "ntr_bvh_reorder: the tree has %u nodes and %u rows; the output buffers hold %lld nodes and %lld "
                         "rows (at most %lld nodes, 2^31 - 1 rows); nothing was written", h.nodes, h.rows, (long long)nodeCap, (long long)rowCap,
                         (long long)kMaxNodes);
    const long long nodeLanes = 4ll * h.nodes, rowLanes = 2ll * numSlots * RO_ROW_LANES;
    hipLaunchKernelGGL(ro_copy_nodes, dim3((unsigned int)((nodeLanes + RO_BLOCK - 1) / RO_BLOCK)), block, 0, s, (int)h.nodes, numSlots,
                       (const uint4*)d_nodes, (const int*)srcOf, (const int2*)newLink, (uint4*)d_outNodes);
    hipLaunchKernelGGL(ro_copy_rows, dim3((unsigned int)((rowLanes + RO_BLOCK - 1) / RO_BLOCK)), block, 0, s, numSlots, (const int*)d_nodes,
                       numRows, (const uint4*)d_triWoop, d_triIndex, (const unsigned long long*)info, (const int*)newLink, (long long)h.rows,
                       (uint4*)d_outTriWoop, d_outTriIndex);
    NTR_HIP(hipGetLastError());
    NTR_HIP(ev.record(1));
    float ms = 0.0f;
    NTR_HIP(ev.elapsed(0, 1, &ms));
    result->seconds = ms * 1e-3f;
    if (err)
        return set_error(NTR_ERR_LAYOUT, "ntr_bvh_reorder: malformed tree (error 0x%x: 1 child link outside the node extent, copied "
                         "unchanged; 2 leaf without a terminator inside the extent, emitted as a lone terminator row)", err);
    return NTR_OK;
}

int ntr_bvh_reorder_scratch_bytes(int64_t* bytes)
{
    if (!bytes) return set_error(NTR_ERR_INVALID, "ntr_bvh_reorder_scratch_bytes: null");
    *bytes = (int64_t)g_roPool.held();
    return NTR_OK;
}

}  // extern "C"
