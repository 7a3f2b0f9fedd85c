// bvh_optimize_treelet.h -- the treelet side of the optimiser (tests/np_bvh_optimize.py), stated once for the single-tree
// unit (bvh_optimize_kernels.hip) and the pool unit (bvh_optimize_batch_kernels.hip): which slots root a treelet and under which
// height, the scan and the scatter of those roots into per-height lists, and the restructuring of one treelet by one wave64.  Every
// body is the whole of a kernel but for how the kernel finds its slot and its tree, so a workgroup calls each at most once and every
// thread of the workgroup calls it (the bodies hold barriers).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "bvh_climb.h"
#include "device_prims.h"

namespace ntr {
namespace {   // a unit's own copy: the kernels' names keep the unit's anonymous namespace

constexpr int OP_BLOCK = 256;
constexpr int OP_N = 7;                      // treelet size
constexpr int OP_FULL = (1 << OP_N) - 1;
constexpr int OP_MAX_PASSES = 8;
constexpr int OP_STAT_SLOTS = 64;            // the rewritten-treelet counters of a pass: a workgroup adds to slot blockIdx % 64
constexpr int OP_HIST_LDS = 1024;            // heights below this are counted in LDS first

// *qual = the slot's height if it roots a treelet (reached, leafLinks >= 7), else 0; hist[height] counts them.  `live`: the thread has
// a slot whose tree takes part; slot, numSlots and the arrays are that tree's own, hist is the launch's.
__device__ __forceinline__ void op_histogram_body(bool live, int slot, int numSlots, const int* nodes,
                                                  const unsigned int* parent, const int* height,
                                                  const unsigned int* leafLinks, int* qual,
                                                  unsigned int* hist)
{
    __shared__ unsigned int sh[OP_HIST_LDS];
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK) sh[i] = 0u;
    __syncthreads();
    if (live) {
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
        *qual = q;
        if (q > 0) {
            if (q < OP_HIST_LDS) atomicAdd(&sh[q], 1u); else atomicAdd(&hist[q], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OP_HIST_LDS; i += OP_BLOCK)
        if (sh[i]) atomicAdd(&hist[i], sh[i]);
}

// cursor[h] = the exclusive scan of hist[0 .. nb): one workgroup
__device__ __forceinline__ void op_scan_body(int nb, const unsigned int* hist, unsigned int* cursor)
{
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
// all land on the same few words (53 us instead of a few on the 49 k-node tree).  numSlots: the slots the launch covers, the length
// of qual and of list; a slot is listed under the index qual is read at.
__device__ __forceinline__ void op_scatter_body(int numSlots, const int* qual, unsigned int* cursor,
                                                int* list)
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

// One wave64 (one workgroup) restructures the treelet rooted at slot R (0 <= R < numSlots) of the tree `nodes`; every branch around a
// barrier is uniform.  A link is followed only where it names a slot of this tree.  rewritten: the pass's OP_STAT_SLOTS counters.
__device__ __forceinline__ void op_treelet_body(int numSlots, int* nodes, int R, unsigned int* rewritten)
{
    __shared__ unsigned int sBox[OP_N][6];       // the entries' boxes, ord_enc words, lo.x hi.x lo.y hi.y lo.z hi.z
    __shared__ int sLink[OP_N];
    __shared__ float sArea[OP_FULL + 1], sCost[OP_FULL + 1], sOrig[OP_FULL + 1];
    __shared__ unsigned char sChoice[OP_FULL + 1];
    __shared__ int sSorted[OP_N - 2];            // the internal slots other than the root, ascending
    __shared__ int sSub[OP_N - 1];               // the entries of the new inner node with preorder index i
    const int lane = threadIdx.x;

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

}  // namespace
}  // namespace ntr
