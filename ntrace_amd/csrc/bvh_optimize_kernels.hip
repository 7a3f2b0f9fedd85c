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
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ntr_internal.h"
#include "bvh_climb.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {
namespace {

constexpr int OP_BLOCK = 256;
constexpr int OP_N = 7;                      // treelet size
constexpr int OP_FULL = (1 << OP_N) - 1;
constexpr int OP_MAX_PASSES = 8;
constexpr int OP_STAT_SLOTS = 64;            // the rewritten-treelet counters of a pass: a workgroup adds to slot blockIdx % 64
constexpr int OP_HIST_LDS = 1024;            // heights below this are counted in LDS first
enum : unsigned int { OP_ERR_LINK = 1u, OP_ERR_ROW = 2u };

struct OpRoot {                              // what the owner of slot 0 reports; `done` stays 0 if the climb never got there
    unsigned int done, height, leafLinks, slots, leaves, tris, err;
    float sah;
    unsigned int pad[8];
};
static_assert(sizeof(OpRoot) == 64, "OpRoot must be 64 bytes");

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

// What a child reports to its node.  SAH: three 8-byte words (value | height, leaves | triangles, slots); else one (height | leaf links).
template <bool SAH>
struct OpInfo {
    unsigned int height, leafLinks, slots, leaves, tris;
    float value;
};
template <bool SAH>
__device__ __forceinline__ void op_publish(unsigned long long* info, size_t child, const OpInfo<SAH>& v)
{
    if (SAH) {
        unsigned long long* p = info + 3 * child;
        __hip_atomic_store(p, (unsigned long long)__float_as_uint(v.value) | ((unsigned long long)v.height << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 1, (unsigned long long)v.leaves | ((unsigned long long)v.tris << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 2, (unsigned long long)v.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __hip_atomic_store(info + child, (unsigned long long)v.height | ((unsigned long long)v.leafLinks << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <bool SAH>
__device__ __forceinline__ void op_acquire(const unsigned long long* info, size_t child, OpInfo<SAH>& v)
{
    v = OpInfo<SAH>();
    if (SAH) {
        const unsigned long long* p = info + 3 * child;
        const unsigned long long a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long c = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.value = __uint_as_float((unsigned int)a); v.height = (unsigned int)(a >> 32);
        v.leaves = (unsigned int)b; v.tris = (unsigned int)(b >> 32);
        v.slots = (unsigned int)c;
    } else {
        const unsigned long long a = __hip_atomic_load(info + child, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v.height = (unsigned int)a; v.leafLinks = (unsigned int)(a >> 32);
    }
}

// fminf / fmaxf of calcSAHNode pinned: the other operand for a NaN, else by the total order -0 < +0
__device__ __forceinline__ float op_fmin(float a, float b) { return a != a ? b : (b != b ? a : ord_min(a, b)); }
__device__ __forceinline__ float op_fmax(float a, float b) { return a != a ? b : (b != b ? a : ord_max(a, b)); }
// 2 * ((dx*dy + dy*dz) + dz*dx), left to right (emitTreeKernel.cu:1374-1376); this file is compiled without contraction
__device__ __forceinline__ float op_sah_area(float xi, float xa, float yi, float ya, float zi, float za)
{
    const float dx = xa - xi, dy = ya - yi, dz = za - zi;
    return 2.0f * ((dx * dy + dy * dz) + dz * dx);
}

template <bool SAH>
__global__ __launch_bounds__(OP_BLOCK) void opt_climb(int numSlots, const int* __restrict__ nodes, int numRows, const float4* __restrict__ woop,
                                                      const unsigned int* __restrict__ parent, unsigned int* __restrict__ arrive,
                                                      unsigned long long* __restrict__ info, int* __restrict__ height,
                                                      unsigned int* __restrict__ leafLinks, OpRoot* __restrict__ root)
{
    const long long g = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
    if (g >= 2ll * numSlots) return;
    int node = (int)(g >> 1), k = (int)(g & 1);
    const int link = nodes[(size_t)node * kNodeWords + kLinkWord + k];
    if (is_inner_link(link, numSlots)) return;   // an inner child arrives with the owner of its node
    OpInfo<SAH> mine = OpInfo<SAH>();
    mine.leafLinks = 1u;
    if (SAH && link < 0) {
        mine.leaves = 1u;
        long long r = (long long)leaf_row(link);
        while (r < numRows && __float_as_uint(woop[r].x) != kLeafTerm) {   // calcLeafs (emitTreeKernel.cu:1351-1359), inside the extent
            mine.tris++;
            r += 3;
        }
        if (r >= numRows) atomicOr(&root->err, OP_ERR_ROW);
        mine.value = (float)mine.tris;
    }
    OpInfo<SAH> sib;
    const auto publish = [&](int n, int ck) { op_publish<SAH>(info, 2 * (size_t)n + ck, mine); };
    const auto acquire = [&](int n, int ck) { op_acquire<SAH>(info, 2 * (size_t)n + ck, sib); };
    const auto merge = [&](int n, int ck) {
        OpInfo<SAH> up = OpInfo<SAH>();
        up.height = 1u + max(mine.height, sib.height);
        up.leafLinks = mine.leafLinks + sib.leafLinks;
        if (SAH) {
            up.slots = 1u + mine.slots + sib.slots;
            up.leaves = mine.leaves + sib.leaves;
            up.tris = mine.tris + sib.tris;
            const float* nf = reinterpret_cast<const float*>(nodes + (size_t)n * kNodeWords);
            const float4 n0 = *reinterpret_cast<const float4*>(nf), n1 = *reinterpret_cast<const float4*>(nf + 4),
                         n2 = *reinterpret_cast<const float4*>(nf + 8);
            const float pa = op_sah_area(op_fmin(n0.x, n1.x), op_fmax(n0.y, n1.y), op_fmin(n0.z, n1.z), op_fmax(n0.w, n1.w),
                                         op_fmin(n2.x, n2.z), op_fmax(n2.y, n2.w));
            const float pl = op_sah_area(n0.x, n0.y, n0.z, n0.w, n2.x, n2.y);
            const float pr = op_sah_area(n1.x, n1.y, n1.z, n1.w, n2.z, n2.w);
            const float l = ck == 0 ? mine.value : sib.value, r = ck == 0 ? sib.value : mine.value;
            up.value = (1.0f + (pl / pa) * l) + (pr / pa) * r;
        } else {
            height[n] = (int)up.height;
            leafLinks[n] = up.leafLinks;
        }
        if (n == 0) {                         // the root reports to no parent
            root->height = up.height; root->leafLinks = up.leafLinks; root->slots = up.slots; root->leaves = up.leaves;
            root->tris = up.tris; root->sah = up.value; root->done = 1u;
        }
        mine = up;
    };
    publish(node, k);
    climb(node, k, numSlots, nodes, parent, arrive, publish, acquire, merge);
}

// qual[slot] = the slot's height if it roots a treelet (reached, leafLinks >= 7), else 0; hist[height] counts them.
__global__ __launch_bounds__(OP_BLOCK) void opt_histogram(int numSlots, const int* __restrict__ nodes, const unsigned int* __restrict__ parent,
                                                          const int* __restrict__ height, const unsigned int* __restrict__ leafLinks,
                                                          int* __restrict__ qual, unsigned int* __restrict__ hist)
{
    __shared__ unsigned int sh[OP_HIST_LDS];
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK) sh[i] = 0u;
    __syncthreads();
    const int slot = blockIdx.x * OP_BLOCK + threadIdx.x;
    if (slot < numSlots) {
        const int h = height[slot];              // 0: nobody owned this slot in the climb
        int q = 0;
        if (h > 0 && leafLinks[slot] >= (unsigned int)OP_N) {
            int n = slot;
            for (int steps = 0; n != 0 && steps < numSlots; steps++) {
                const unsigned int p = parent[n];
                if (!parent_links_back(p, n, numSlots, nodes)) break;
                n = (int)(p >> 1);
            }
            if (n == 0) q = h;
        }
        qual[slot] = q;
        if (q > 0) {
            if (q < OP_HIST_LDS) atomicAdd(&sh[q], 1u); else atomicAdd(&hist[q], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK)
        if (sh[i]) atomicAdd(&hist[i], sh[i]);
}

// cursor[h] = the exclusive scan of hist[0 .. root->height]: one workgroup, which reads the height the climb has just reported, so the
// host needs no read-back between the histogram and the scatter
__global__ __launch_bounds__(OP_BLOCK) void opt_scan(int numSlots, const OpRoot* __restrict__ root, const unsigned int* __restrict__ hist,
                                                     unsigned int* __restrict__ cursor)
{
    const int nb = root->done ? min((int)root->height, numSlots) + 1 : 0;
    unsigned int carry = 0u;
    for (int base = 0; base < nb; base += OP_BLOCK) {   // uniform
        const int i = base + threadIdx.x;
        unsigned int chunk;
        const unsigned int ex = block_exclusive_scan<OP_BLOCK>(i < nb ? hist[i] : 0u, &chunk);
        if (i < nb) cursor[i] = carry + ex;
        carry += chunk;
    }
}

// The roots into their heights' lists; the order inside a list is immaterial (its treelets are disjoint).  A workgroup ranks its
// roots per height in LDS and reserves one range per height: one global add per workgroup and height instead of one per root, which
// all land on the same few words (53 us instead of a few on the 49 k-node tree).
__global__ __launch_bounds__(OP_BLOCK) void opt_scatter(int numSlots, const int* __restrict__ qual, unsigned int* __restrict__ cursor,
                                                        int* __restrict__ list)
{
    __shared__ unsigned int sCount[OP_HIST_LDS], sBase[OP_HIST_LDS];
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK) sCount[i] = 0u;
    __syncthreads();
    const int slot = blockIdx.x * OP_BLOCK + threadIdx.x;
    const int q = slot < numSlots ? qual[slot] : 0;
    unsigned int rank = 0u;
    if (q > 0 && q < OP_HIST_LDS) rank = atomicAdd(&sCount[q], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK)
        if (sCount[i]) sBase[i] = atomicAdd(&cursor[i], sCount[i]);
    __syncthreads();
    if (q > 0) {
        const unsigned int at = q < OP_HIST_LDS ? sBase[q] + rank : atomicAdd(&cursor[q], 1u);
        if (at < (unsigned int)numSlots) list[at] = slot;
    }
}

__device__ __forceinline__ float op_area(const unsigned int (&b)[6])   // rule 4
{
    const float dx = ord_dec(b[1]) - ord_dec(b[0]), dy = ord_dec(b[3]) - ord_dec(b[2]), dz = ord_dec(b[5]) - ord_dec(b[4]);
    return (dx * dy + dy * dz) + dz * dx;
}

// One wave64 (one workgroup) per treelet; every branch around a barrier is uniform.
__global__ __launch_bounds__(64) void opt_treelets(int numSlots, int* __restrict__ nodes, const int* __restrict__ roots, int count,
                                                   unsigned int* __restrict__ rewritten)
{
    __shared__ unsigned int sBox[OP_N][6];       // the entries' boxes, ord_enc words, lo.x hi.x lo.y hi.y lo.z hi.z
    __shared__ int sLink[OP_N];
    __shared__ float sArea[OP_FULL + 1], sCost[OP_FULL + 1], sOrig[OP_FULL + 1];
    __shared__ unsigned char sChoice[OP_FULL + 1];
    __shared__ int sSorted[OP_N - 2];            // the internal slots other than the root, ascending
    __shared__ int sSub[OP_N - 1];               // the entries of the new inner node with preorder index i
    if ((int)blockIdx.x >= count) return;
    const int lane = threadIdx.x;
    const int R = roots[blockIdx.x];
    if (R < 0 || R >= numSlots) return;

    // ---- formation (rule 3): lane j < 6 keeps the entry masks of internal node j (node 0 = R), lane e < n entry e's link and area
    unsigned int m0 = lane == 0 ? 1u : 0u, m1 = lane == 0 ? 2u : 0u;
    int mySlot = R;                              // lane j: the slot of internal node j + 1
    int pos0 = 0, pos1 = 1, from = R;
    for (int n = 2;; n++) {
        if (lane < 12) {
            const int w = lane;
            sBox[box_word_child(w) ? pos1 : pos0][box_word_comp(w)] = ord_enc(__int_as_float(nodes[(size_t)from * kNodeWords + w]));
        } else if (lane < 14) {
            sLink[lane == kLinkWord ? pos0 : pos1] = nodes[(size_t)from * kNodeWords + lane];
        }
        __syncthreads();
        if (n == OP_N) break;
        int myLink = 0;
        float myArea = 0.0f;
        if (lane < n) {
            myLink = sLink[lane];
            unsigned int b[6];
#pragma unroll
            for (int j = 0; j < 6; j++) b[j] = sBox[lane][j];
            myArea = op_area(b);
        }
        const unsigned long long inner = __ballot(lane < n && is_inner_link(myLink, numSlots));
        if (!inner) return;                      // cannot happen with leafLinks >= 7 in a tree; uniform
        int cand = __ffsll((long long)inner) - 1;
        float best = __shfl(myArea, cand);
        for (int e = cand + 1; e < n; e++) {
            const float a = __shfl(myArea, e);
            if (((inner >> e) & 1ull) && a > best) { best = a; cand = e; }
        }
        from = inner_index(__shfl(myLink, cand));
        pos0 = cand;
        pos1 = n;
        const unsigned int bit = 1u << cand, fresh = 1u << n;
        if (lane < n - 1) {
            if (m0 & bit) m0 |= fresh;
            if (m1 & bit) m1 |= fresh;
        } else if (lane == n - 1) {
            m0 = bit;
            m1 = fresh;
        }
        if (lane == n - 2) mySlot = from;
        __syncthreads();                         // everybody has read the entries before the next record overwrites one
    }

    // the five internal slots in ascending order (distinct in a tree; the table starts as R so that no word of it is ever undefined)
    if (lane < OP_N - 2) sSorted[lane] = R;
    __syncthreads();
    {
        int rank = 0;
        for (int j = 0; j < OP_N - 2; j++) {
            const int other = __shfl(mySlot, j);
            if (other < mySlot) rank++;
        }
        if (lane < OP_N - 2) sSorted[rank] = mySlot;
    }

    // ---- rule 4: the areas of subsets lane and lane + 64; rule 5's single entries
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int s = lane + 64 * half;
        unsigned int b[6] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
        for (int e = 0; e < OP_N; e++) {
            if ((s >> e) & 1) {
#pragma unroll
                for (int j = 0; j < 6; j += 2) {
                    b[j] = min(b[j], sBox[e][j]);
                    b[j + 1] = max(b[j + 1], sBox[e][j + 1]);
                }
            }
        }
        sArea[s] = s ? op_area(b) : 0.0f;
        sCost[s] = 0.0f;
        sOrig[s] = 0.0f;
        sChoice[s] = 0;
    }
    __syncthreads();

    // ---- rule 5: subsets of size k; a lane's subsets lane and lane + 64 differ by one in size, so it has at most one per round
    const int pc = __popc((unsigned int)lane);
    for (int k = 2; k <= OP_N; k++) {
        const int s = pc == k ? lane : (pc == k - 1 ? lane + 64 : 0);
        if (s) {
            const int low = s & -s, rest = s ^ low;
            float best = INFINITY;
            int bp = low;
            for (int q = 0; q != rest; q = (q - rest) & rest) {   // the subsets of rest in ascending order, rest itself left out
                const float v = sCost[low | q] + sCost[rest ^ q];
                if (v < best) { best = v; bp = low | q; }
            }
            sCost[s] = sArea[s] + best;
            sChoice[s] = (unsigned char)bp;
        }
        __syncthreads();
    }

    // ---- rule 6: the existing topology's cost, children before parents (a child is formed after its parent)
    for (int i = OP_N - 2; i >= 0; i--) {
        if (lane == i) sOrig[m0 | m1] = sArea[m0 | m1] + (sOrig[m0] + sOrig[m1]);
        __syncthreads();
    }
    if (!(sCost[OP_FULL] < sOrig[OP_FULL])) return;   // uniform: nothing of this treelet changes

    // ---- rule 7
    if (lane == 0) {
        sSub[0] = OP_FULL;
        for (int i = 0; i < OP_N - 1; i++) {
            const int s = sSub[i], p = sChoice[s], o = s ^ p;
            const int np = __popc((unsigned int)p);
            if (np > 1 && i + 1 < OP_N - 1) sSub[i + 1] = p;
            if (__popc((unsigned int)o) > 1 && i + np < OP_N - 1) sSub[i + np] = o;   // i + 1 + (np - 1)
        }
        atomicAdd(&rewritten[blockIdx.x % OP_STAT_SLOTS], 1u);
    }
    __syncthreads();
    for (int item = lane; item < 16 * (OP_N - 1); item += 64) {
        const int i = item >> 4, w = item & 15;
        if (w == 15) continue;                   // the fourth link word stays
        const int s = sSub[i] & OP_FULL, p = sChoice[s], o = s ^ p;
        const int slot = i == 0 ? R : sSorted[i - 1];
        int word = 0;                            // w == 14: the split word, which no kernel reads
        if (w < 12) {
            const int q = box_word_child(w) ? o : p, j = box_word_comp(w);
            unsigned int v = (j & 1) ? 0u : 0xFFFFFFFFu;
            for (int e = 0; e < OP_N; e++)
                if ((q >> e) & 1) v = (j & 1) ? max(v, sBox[e][j]) : min(v, sBox[e][j]);
            word = __float_as_int(ord_dec(v));
        } else if (w < 14) {
            const int q = w == 12 ? p : o;
            const int np = __popc((unsigned int)p);
            if (__popc((unsigned int)q) <= 1) {
                word = sLink[__ffs(q | (1 << (OP_N - 1))) - 1];
            } else {
                const int idx = w == 12 ? i + 1 : i + np;
                word = inner_link(sSorted[min(max(idx, 1), OP_N - 2) - 1]);
            }
        }
        nodes[(size_t)slot * kNodeWords + w] = word;
    }
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
