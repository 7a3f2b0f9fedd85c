// bvh_ploc_batch_kernels.hip -- many PLOC builds in one pass for gfx950 (ntr_ploc_build_batch): every mesh of a batch becomes a bottom-level
// tree (BLAS) of one pool (instanced_bvh.h), each byte for byte what ntr_ploc_build writes for that mesh at pool + offset.  EXTENSION: the
// reference has neither PLOC nor instancing; the rule is the numpy spec tests/np_ploc_batch.py (np_bvh_ploc.build per mesh,
// np_instanced.make_pool over the results), which the build equals byte for byte.
// All meshes' clusters live in ONE list, mesh after mesh: a cluster carries (box, link, height, mesh), a mesh the start and the length of its
// segment of the list.  Every round of every mesh runs in the same launches; a mesh that has reached one cluster keeps that cluster in the
// list and takes no further part.
//   before the rounds  pb_codes: one thread per triangle slot (slot = the mesh's first slot + the triangle's index within the mesh; two
//                        meshes may name the same triangles): finds its mesh, checks the vertex indices, takes the LBVH's Morton code over
//                        ITS MESH's box and counts the digits of all sort passes; thread m also starts mesh m's segment.  One read-back
//                      sort: radix_sort.h's one-sweep passes over the 30-bit code, then over the mesh index (LSD, stable: within a mesh
//                        np_hlbvh.morton_sorted's order, ties by triangle id; meshes in mesh order)
//                      pb_leaves: one thread per sorted slot: its cluster, its leaf's three Woop rows, terminator row and triIndex entries
//                        at the mesh's row base; a one-triangle mesh gets ntr_ploc_build's one-triangle node and rows and a cluster of
//                        height 1 that never merges
//   per round          pb_search: as pl_search -- tile plus halo in LDS -- but a lane's candidates are i +- k inside its segment, k and the
//                        parity bit taken from the position relative to the segment's start (pl_nearest, ploc_rounds.h)
//                      pb_mark + pb_sums: the mutual test, the scan of (survivors, merging pairs) over the whole list and one item more, so
//                        that the scan can be read at a segment's end
//                      pb_update: a thread per mesh reads the scan at its segment's two ends: its pairs m, its next start and length; counts
//                        the round, takes the height when two clusters become one, adds the meshes still open to the state record
//                      pb_scatter: a pair of mesh k writes node slot (n_k - 1 - m_k) + r of ITS node range, r its rank among the segment's
//                        pairs, and links 64 * slot; the survivors go to the other cluster buffer, compacted
// The host launches rounds in groups of four and reads the 32-byte record once per group until no mesh is open (as ploc_rounds).  There is
// no tail launch: with many meshes the list never becomes short, and the last rounds are a few tiles.  A round that merges nothing in an
// open mesh, a list position or a node slot outside its mesh's range set an error bit and end the call with NTR_ERR_LAYOUT.
// Distances keep the spec's order of operations (__fmul_rn / __fadd_rn, and the library is compiled without contraction).
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "level_build.h"
#include "ploc_rounds.h"
#include "radix_sort.h"

namespace ntr {
namespace {

constexpr int PB_TILE = NTR_PLOC_TILE;   // clusters of a workgroup of the round kernels, one per thread
constexpr int PB_BLOCK = 256;            // per-slot and per-mesh kernels
constexpr int PB_ITEMS = 8;              // keys per thread of a sort tile
constexpr int PB_CODE_PASSES = 4;        // 30-bit codes
constexpr int PB_MAX_PASSES = PB_CODE_PASSES + 3;   // + the mesh index: at most 20 bits
constexpr int PB_MAX_MESHES = 1 << 20;
constexpr int kRoundsPerRead = 4;
constexpr int kErrWord = 8;              // of the sort's misc words: [0..6] tickets, [8] the chained scans' error flag
static_assert(PB_TILE == 1024, "one cluster per thread of a 1024-thread workgroup");
static_assert(PB_MAX_PASSES <= kErrWord && PB_MAX_PASSES <= OS_MAX_PASSES, "a ticket per pass");

struct PbMesh {             // device table, one per mesh
    int firstTri, numTris;  // triangles [firstTri, +numTris) of the shared index array
    int start;              // first slot (and first list position before the rounds): the running sum of numTris
    int nodeBase, rowBase;  // nodesOffset / 64, triWoopOffset / 16
    float lo[3], step[3];   // the Morton grid: sceneMin, (sceneMax - sceneMin) / 1024 (taken on the host, as ntr_lbvh_build does)
    int pad;
};
static_assert(sizeof(PbMesh) == 48, "three 16-byte rows");

struct PbState {            // halves [k & 1] are read by round k, [(k & 1) ^ 1] written
    int n[2];               // list length
    int open[2];            // meshes with more than one cluster
    int cur[2];             // which cluster buffer holds the list
    unsigned int err;       // bit 0: vertex index out of range, bit 2: a node slot or a list position outside its mesh's range, bit 3: a
                            // round without a merge in an open mesh, bit 4: the sorted order does not keep the meshes apart (none of
                            // the last three is expected; the bits keep PlState's meaning)
    int pad;
};
static_assert(sizeof(PbState) == 32, "one 32-byte record (read_totals)");

struct PbBuf {              // a list of clusters: box component c of cluster i at box[c * cap + i] (lo.x lo.y lo.z hi.x hi.y hi.z)
    float* box;
    int* link;
    int* height;
    int* mesh;
};
struct PbBufs { PbBuf b[2]; };

struct PbSegs {             // per mesh: its segment of the list, double buffered like PbState; what a round's kernels hand each other
    int* start[2];
    int* len[2];
    int* pairBase;          // pairs of the list before the segment's start, this round (pb_update -> pb_scatter)
    int* rounds;            // rounds the mesh took part in
    int* height;            // its last cluster's height, once it has one cluster
};

// the scan of (survivors, pairs) before list position i (i == n: the totals)
__device__ __forceinline__ U2 pb_scan_at(const U2* __restrict__ local, const U2* __restrict__ blockSums, int i)
{
    return local[i] + blockSums[i / PB_TILE];
}

// emitTreeKernel.cu:647-653
__device__ __forceinline__ unsigned int pb_spread(unsigned int v)
{
    v &= 0x3ffu;
    v = (v ^ (v << 16)) & 0xff0000ffu;
    v = (v ^ (v << 8)) & 0x0300f00fu;
    v = (v ^ (v << 4)) & 0x030c30c3u;
    return (v ^ (v << 2)) & 0x09249249u;
}

// ---- before the rounds --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB_BLOCK) void pb_codes(int n, int numMeshes, const PbMesh* __restrict__ meshes, const int* __restrict__ tri,
                                                     int numVerts, const float* __restrict__ pos, unsigned int* __restrict__ keys,
                                                     int* __restrict__ meshOf, int passes, unsigned int* __restrict__ hist /* [passes][256], zeroed */,
                                                     PbSegs seg, PbState* __restrict__ st)
{
    __shared__ unsigned int s_hist[PB_MAX_PASSES][256];
    for (int k = threadIdx.x; k < PB_MAX_PASSES * 256; k += PB_BLOCK) (&s_hist[0][0])[k] = 0u;
    __syncthreads();
    const int q = blockIdx.x * PB_BLOCK + threadIdx.x;
    if (q < numMeshes) {   // (numMeshes <= n: every mesh has a triangle)
        seg.start[0][q] = meshes[q].start;
        seg.len[0][q] = meshes[q].numTris;
        seg.rounds[q] = 0;
        seg.height[q] = meshes[q].numTris == 1 ? 1 : 0;
    }
    if (q < n) {
        int a = 0, b = numMeshes - 1;   // the last mesh whose first slot is at or before q
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (meshes[mid].start <= q) a = mid;
            else b = mid - 1;
        }
        const PbMesh m = meshes[a];
        const int t = q - m.start;
        int i0, i1, i2;
        unsigned int key = 0u;
        if (t < 0 || t >= m.numTris) {
            atomicOr(&st->err, 4u);
        } else if (!tri_indices_checked(tri + 3 * (size_t)m.firstTri, numVerts, t, i0, i1, i2)) {
            atomicOr(&st->err, 1u);
        } else {
            // lbvh_morton_hist_kernel's code (lbvh_kernels.hip), over the mesh's own grid
            unsigned int cell[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float va = pos[3 * (size_t)i0 + c], vb = pos[3 * (size_t)i1 + c], vc = pos[3 * (size_t)i2 + c];
                const float mn = fminf(va, fminf(vb, vc)), mx = fmaxf(va, fmaxf(vb, vc));
                const float mid = mn + (mx - mn) / 2.0f;
                const int v = (int)floorf((mid - m.lo[c]) / m.step[c]);
                cell[c] = (unsigned int)min(max(v, 0), 1023);
            }
            key = pb_spread(cell[0]) | (pb_spread(cell[1]) << 1) | (pb_spread(cell[2]) << 2);
        }
        keys[q] = key;
        meshOf[q] = a;
#pragma unroll
        for (int p = 0; p < PB_MAX_PASSES; p++)
            if (p < passes) atomicAdd(&s_hist[p][((p < PB_CODE_PASSES ? key >> (8 * p) : (unsigned int)a >> (8 * (p - PB_CODE_PASSES)))) & 255u], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < passes * 256; k += PB_BLOCK) {
        const unsigned int v = (&s_hist[0][0])[k];
        if (v) atomicAdd(&hist[k], v);
    }
}

__global__ __launch_bounds__(PB_BLOCK) void pb_leaves(int n, int numMeshes, const PbMesh* __restrict__ meshes, const int* __restrict__ tri,
                                                      int numVerts, const float* __restrict__ pos, const int* __restrict__ sorted,
                                                      const int* __restrict__ meshOf, PbBuf out, int cap, int* __restrict__ nodes,
                                                      uint4* __restrict__ woop, int* __restrict__ triIndex, PbState* __restrict__ st)
{
    const int p = blockIdx.x * PB_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int q = sorted[p];
    if (q < 0 || q >= n) { atomicOr(&st->err, 16u); return; }
    const int k = meshOf[q];
    if (k < 0 || k >= numMeshes) { atomicOr(&st->err, 16u); return; }
    const PbMesh m = meshes[k];
    const int lp = p - m.start, t = q - m.start;   // the leaf's position in its mesh's order, the triangle's index within its mesh
    if (lp < 0 || lp >= m.numTris || t < 0 || t >= m.numTris) { atomicOr(&st->err, 16u); return; }
    const int* mtri = tri + 3 * (size_t)m.firstTri;
    float lo[3], hi[3];
    if (!tri_box_checked(mtri, numVerts, pos, t, lo, hi)) { atomicOr(&st->err, 1u); return; }   // pb_codes has passed
#pragma unroll
    for (int c = 0; c < 3; c++) {
        out.box[(size_t)c * cap + p] = lo[c];
        out.box[(size_t)(3 + c) * cap + p] = hi[c];
    }
    out.mesh[p] = k;
    float4 r0, r1, r2;
    woop_rows(mtri, pos, t, r0, r1, r2);
    long long row;
    if (m.numTris == 1) {
        // an empty child 0 (a terminator row only) and the triangle in child 1: pl_single's node and rows
        const float b0[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
        const float b1[6] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
        pl_write_node(nodes, m.nodeBase, b0, leaf_link(0), b1, leaf_link(1));
        write_leaf_terminator(woop, triIndex, m.rowBase);
        write_leaf_terminator(woop, triIndex, (long long)m.rowBase + 4);
        row = (long long)m.rowBase + 1;
        out.link[p] = 0;      // the one node of the mesh; no round reads it
        out.height[p] = 1;
    } else {
        row = (long long)m.rowBase + 4ll * lp;
        write_leaf_terminator(woop, triIndex, row + 3);
        out.link[p] = leaf_link(4 * lp);
        out.height[p] = 0;
    }
    float4* w = (float4*)woop;
    w[row] = r0; w[row + 1] = r1; w[row + 2] = r2;
    triIndex[row] = t; triIndex[row + 1] = 0; triIndex[row + 2] = 0;
}

// ---- a round --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB_TILE) void pb_search(int k, PbState* __restrict__ st, PbBufs bufs, int cap, int radius, int numMeshes,
                                                     PbSegs seg, int* __restrict__ nn)
{
    constexpr int STRIDE = PB_TILE + 2 * kPlocMaxRadius;
    __shared__ float s_box[6 * STRIDE];
    const int p = k & 1;
    const int n = st->n[p];
    const int base = blockIdx.x * PB_TILE;
    if (st->open[p] <= 0 || base >= n) return;
    const PbBuf in = bufs.b[st->cur[p]];
    for (int l = threadIdx.x; l < PB_TILE + 2 * radius; l += PB_TILE) {
        const int g = base - radius + l;
        if (g >= 0 && g < n) {
#pragma unroll
            for (int c = 0; c < 6; c++) s_box[c * STRIDE + l] = in.box[(size_t)c * cap + g];
        }
    }
    __syncthreads();
    const int i = base + threadIdx.x;
    if (i >= n) return;
    const int m = in.mesh[i];
    if (m < 0 || m >= numMeshes) { atomicOr(&st->err, 4u); nn[i] = -1; return; }
    const int s0 = seg.start[p][m], len = seg.len[p][m];
    const int rel = i - s0;
    // (a segment lies inside the list, so every column pl_nearest reads -- rel +- k inside [0, len) -- has been staged)
    if (rel < 0 || rel >= len || s0 < 0 || s0 + len > n) { atomicOr(&st->err, 4u); nn[i] = -1; return; }
    const int best = pl_nearest(s_box, STRIDE, threadIdx.x + radius, rel, len, radius);
    nn[i] = best < 0 ? -1 : s0 + best;
}

// items 0 .. n: item n counts nothing and receives the totals
__global__ __launch_bounds__(PB_TILE) void pb_mark(int k, const PbState* __restrict__ st, const int* __restrict__ nn, U2* __restrict__ local,
                                                   U2* __restrict__ blockSums)
{
    const int p = k & 1;
    const int n = st->n[p];
    if (st->open[p] <= 0 || blockIdx.x * PB_TILE > n) return;
    const int i = blockIdx.x * PB_TILE + threadIdx.x;
    U2 v{0u, 0u};
    if (i < n) {
        const int j = nn[i];
        const bool mutual = j >= 0 && j < n && nn[j] == i;
        v.x = (mutual && i > j) ? 0u : 1u;
        v.y = (mutual && i < j) ? 1u : 0u;
    }
    scan_local_store<PB_TILE>(v, i <= n, (size_t)i, local, blockSums, (int)blockIdx.x);
}

// one workgroup: the block sums' exclusive scan in place, and the other half of the record (pb_update adds the open meshes)
__global__ __launch_bounds__(PB_TILE) void pb_sums(int k, PbState* __restrict__ st, U2* __restrict__ blockSums)
{
    const int p = k & 1, q = p ^ 1;
    const int n = st->n[p];
    const bool active = st->open[p] > 0;
    U2 carry{0u, 0u};
    if (active) {
        const int nb = n / PB_TILE + 1;
        for (int base = 0; base < nb; base += PB_TILE) {
            const int i = base + threadIdx.x;
            const U2 v = i < nb ? blockSums[i] : U2{0u, 0u};
            U2 chunk;
            const U2 ex = block_exclusive_scan<PB_TILE>(v, &chunk);
            if (i < nb) blockSums[i] = carry + ex;
            carry = carry + chunk;
        }
    }
    if (threadIdx.x == 0) {
        if (active && (carry.y == 0u || carry.x + carry.y != (unsigned int)n)) atomicOr(&st->err, 8u);
        st->n[q] = active ? n - (int)carry.y : n;
        st->open[q] = 0;
        st->cur[q] = st->cur[p] ^ (active ? 1 : 0);
    }
}

__global__ __launch_bounds__(PB_BLOCK) void pb_update(int k, PbState* __restrict__ st, int numMeshes, PbBufs bufs, PbSegs seg,
                                                      const U2* __restrict__ local, const U2* __restrict__ blockSums)
{
    const int p = k & 1, q = p ^ 1;
    if (st->open[p] <= 0) return;   // the same in every thread
    const int n = st->n[p];
    const int m = blockIdx.x * PB_BLOCK + threadIdx.x;
    bool open = false;
    if (m < numMeshes) {
        const int s0 = seg.start[p][m], len = seg.len[p][m];
        if (s0 < 0 || len < 1 || s0 + len > n) {
            atomicOr(&st->err, 4u);
        } else {
            const U2 a = pb_scan_at(local, blockSums, s0), b = pb_scan_at(local, blockSums, s0 + len);
            const int pairs = (int)(b.y - a.y), next = len - pairs;
            if ((int)(b.x - a.x) != next || next < 1) atomicOr(&st->err, 4u);
            if (len > 1) {
                if (pairs == 0) atomicOr(&st->err, 8u);
                seg.rounds[m]++;
                if (next == 1) {   // two clusters become one
                    const PbBuf in = bufs.b[st->cur[p]];
                    seg.height[m] = 1 + max(in.height[s0], in.height[s0 + len - 1]);
                }
            }
            seg.start[q][m] = (int)a.x;
            seg.len[q][m] = next;
            seg.pairBase[m] = (int)a.y;
            open = next > 1;
        }
    }
    const int cnt = __syncthreads_count(open ? 1 : 0);
    if (threadIdx.x == 0 && cnt) atomicAdd(&st->open[q], cnt);
}

__global__ __launch_bounds__(PB_TILE) void pb_scatter(int k, PbState* __restrict__ st, PbBufs bufs, int cap, int numMeshes, PbSegs seg,
                                                      const PbMesh* __restrict__ meshes, const int* __restrict__ nn,
                                                      const U2* __restrict__ local, const U2* __restrict__ blockSums, int* __restrict__ nodes)
{
    const int p = k & 1, q = p ^ 1;
    const int n = st->n[p];
    const int i = blockIdx.x * PB_TILE + threadIdx.x;
    if (st->open[p] <= 0 || i >= n) return;
    const PbBuf in = bufs.b[st->cur[p]], out = bufs.b[st->cur[p] ^ 1];
    const int j = nn[i];
    const bool mutual = j >= 0 && j < n && nn[j] == i;
    if (mutual && i > j) return;
    const U2 e = local[i] + blockSums[blockIdx.x];
    const int m = in.mesh[i];
    if (m < 0 || m >= numMeshes) { atomicOr(&st->err, 4u); return; }
    const int len = seg.len[p][m], nextStart = seg.start[q][m], nextLen = seg.len[q][m];
    const int dst = (int)e.x;
    if (dst < nextStart || dst >= nextStart + nextLen || dst >= cap) { atomicOr(&st->err, 4u); return; }
    float a[6];
#pragma unroll
    for (int c = 0; c < 6; c++) a[c] = in.box[(size_t)c * cap + i];
    int link = in.link[i], height = in.height[i];
    if (mutual) {
        const int pairs = len - nextLen;
        const int slot = (len - 1 - pairs) + ((int)e.y - seg.pairBase[m]);   // of the mesh's own node range
        if (slot < 0 || slot >= meshes[m].numTris - 1 || in.mesh[j] != m) { atomicOr(&st->err, 4u); return; }
        float b[6];
#pragma unroll
        for (int c = 0; c < 6; c++) b[c] = in.box[(size_t)c * cap + j];
        pl_write_node(nodes, meshes[m].nodeBase + slot, a, link, b, in.link[j]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            a[c] = ord_min(a[c], b[c]);
            a[3 + c] = ord_max(a[3 + c], b[3 + c]);
        }
        link = inner_link(slot);
        height = 1 + max(height, in.height[j]);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) out.box[(size_t)c * cap + dst] = a[c];
    out.link[dst] = link;
    out.height[dst] = height;
    out.mesh[dst] = m;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct PbLayout {
    size_t keys[2], idx[2], meshOf, zero, zeroBytes, hist, misc, tileState, meshes, state, nn, local, blockSums, box[2], link[2], height[2],
        mesh[2], segStart[2], segLen[2], pairBase, perMesh /* rounds then height: one read-back */, off;
    int tiles;
    PbLayout(int64_t n, int64_t numMeshes)
    {
        ScratchCarver cv;
        tiles = (int)((n + OS_THREADS * PB_ITEMS - 1) / (OS_THREADS * PB_ITEMS));
        for (int k = 0; k < 2; k++) { keys[k] = cv.take((size_t)n * 4); idx[k] = cv.take((size_t)n * 4); }
        meshOf = cv.take((size_t)n * 4);
        // one zeroed block: the digit histograms, tickets and error flag, the tile state of the chained scans
        zero = hist = cv.take(PB_MAX_PASSES * 256 * 4);
        misc = cv.take(64);
        tileState = cv.take((size_t)tiles * 256 * 8);
        zeroBytes = cv.off - zero;
        meshes = cv.take((size_t)numMeshes * sizeof(PbMesh));
        state = cv.take(sizeof(PbState));
        nn = cv.take((size_t)n * 4);
        local = cv.take((size_t)(n + 1) * sizeof(U2));
        blockSums = cv.take((size_t)(n / PB_TILE + 2) * sizeof(U2));
        for (int k = 0; k < 2; k++) {
            box[k] = cv.take((size_t)n * 24);
            link[k] = cv.take((size_t)n * 4);
            height[k] = cv.take((size_t)n * 4);
            mesh[k] = cv.take((size_t)n * 4);
            segStart[k] = cv.take((size_t)numMeshes * 4);
            segLen[k] = cv.take((size_t)numMeshes * 4);
        }
        pairBase = cv.take((size_t)numMeshes * 4);
        perMesh = cv.take((size_t)numMeshes * 8);
        off = cv.off;
    }
};

DeviceScratchPool g_pbPool;

// The pool's layout: every mesh's range, the extents.  The checks that need the meshes' sizes only
int pb_plan(const char* fn, int32_t numMeshes, const NtrPlocBatchMesh* meshes, NtrBlasRange* ranges, int64_t* numTris, int64_t* nodesBytes,
            int64_t* rowsOut)
{
    if (numMeshes < 1 || numMeshes > PB_MAX_MESHES || !meshes)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numMeshes <= %d, a non-null mesh array)", fn, PB_MAX_MESHES);
    int64_t tris = 0, nodes = 0, rows = 0;
    for (int k = 0; k < numMeshes; k++) {
        const int64_t n = meshes[k].numTris;
        if (n < 1) return set_error(NTR_ERR_INVALID, "%s: mesh %d: numTris %lld < 1", fn, k, (long long)n);
        tris += n;
    }
    if (tris >= (1ll << 28)) return set_error(NTR_ERR_INVALID, "%s: %lld triangles in all; at most 2^28 - 1", fn, (long long)tris);
    for (int k = 0; k < numMeshes; k++) {
        const int64_t n = meshes[k].numTris;
        const int64_t nd = std::max<int64_t>(n - 1, 1), rw = n == 1 ? 5 : 4 * n;
        if (nd > kMaxNodes)
            return set_error(NTR_ERR_OVERFLOW, "%s: mesh %d: %lld triangles make %lld inner nodes, more than the %lld that BVHLayout_Compact's "
                             "32-bit child offsets address", fn, k, (long long)n, (long long)nd, (long long)kMaxNodes);
        if (ranges) ranges[k] = NtrBlasRange{nodes * kNodeBytes, nd * kNodeBytes, rows * kRowBytes, rw * kRowBytes};
        nodes += nd;
        rows += rw;
    }
    if (nodes * kNodeBytes > kPoolMaxBytes || rows * kRowBytes > kPoolMaxBytes)
        return set_error(NTR_ERR_OVERFLOW, "%s: the pool would take %lld node bytes and %lld triWoop bytes; a pool buffer holds at most 0x%llx",
                         fn, (long long)(nodes * kNodeBytes), (long long)(rows * kRowBytes), (unsigned long long)kPoolMaxBytes);
    *numTris = tris;
    *nodesBytes = nodes * kNodeBytes;
    *rowsOut = rows;
    return NTR_OK;
}

int pb_build(int numMeshes, const NtrPlocBatchMesh* meshes, int n, const int32_t* d_tri, int32_t numVerts, const float* d_pos, int radius,
             void* d_nodes, void* d_woop, int32_t* d_idx, const NtrBlasRange* ranges, NtrPlocBatchMeshResult* meshResults,
             NtrPlocBatchResult* res, hipStream_t s, std::chrono::steady_clock::time_point wall0 /* the call's start */)
{
    const char* fn = "ntr_ploc_build_batch";
    const PbLayout lay((int64_t)n, (int64_t)numMeshes);
    void* base = nullptr;
    if (const int rc = first_block(g_pbPool, lay.off, &base)) return rc;
    PbState* st = at<PbState>(base, lay.state);
    PbMesh* d_meshes = at<PbMesh>(base, lay.meshes);
    PbBufs bufs;
    PbSegs seg;
    for (int k = 0; k < 2; k++) {
        bufs.b[k] = PbBuf{at<float>(base, lay.box[k]), at<int>(base, lay.link[k]), at<int>(base, lay.height[k]), at<int>(base, lay.mesh[k])};
        seg.start[k] = at<int>(base, lay.segStart[k]);
        seg.len[k] = at<int>(base, lay.segLen[k]);
    }
    seg.pairBase = at<int>(base, lay.pairBase);
    seg.rounds = at<int>(base, lay.perMesh);
    seg.height = seg.rounds + numMeshes;

    // the device's table, and the meshes that have rounds to run
    std::vector<PbMesh> table((size_t)numMeshes);   // (lives until the read-back below has drained the stream)
    int open = 0, start = 0;
    for (int k = 0; k < numMeshes; k++) {
        PbMesh& m = table[k];
        m.firstTri = meshes[k].firstTri;
        m.numTris = meshes[k].numTris;
        m.start = start;
        m.nodeBase = (int)(ranges[k].nodesOffset / kNodeBytes);
        m.rowBase = (int)(ranges[k].triWoopOffset / kRowBytes);
        for (int a = 0; a < 3; a++) {
            m.lo[a] = meshes[k].sceneMin[a];
            m.step[a] = (meshes[k].sceneMax[a] - meshes[k].sceneMin[a]) / 1024.0f;
        }
        m.pad = 0;
        start += m.numTris;
        open += m.numTris > 1;
    }
    int meshBits = 0;
    while (meshBits < 32 && ((int64_t)numMeshes - 1) >> meshBits) meshBits++;
    const int passes = PB_CODE_PASSES + (meshBits + 7) / 8;

    StreamEvents<5> ev(s);
    (void)ev.create();
    ev.mark(0);
    PbState h;
    memset(&h, 0, sizeof(h));
    h.n[0] = n;
    h.open[0] = open;
    NTR_HIP(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemcpyAsync(d_meshes, table.data(), table.size() * sizeof(PbMesh), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemsetAsync(at<char>(base, lay.zero), 0, lay.zeroBytes, s));
    unsigned int* hist = at<unsigned int>(base, lay.hist);
    unsigned int* misc = at<unsigned int>(base, lay.misc);
    unsigned long long* tileState = at<unsigned long long>(base, lay.tileState);
    unsigned int *kIn = at<unsigned int>(base, lay.keys[0]), *kOut = at<unsigned int>(base, lay.keys[1]);
    int *vIn = at<int>(base, lay.idx[0]), *vOut = at<int>(base, lay.idx[1]);
    int* meshOf = at<int>(base, lay.meshOf);
    const int nbN = (n + PB_BLOCK - 1) / PB_BLOCK;
    pb_codes<<<nbN, PB_BLOCK, 0, s>>>(n, numMeshes, d_meshes, d_tri, numVerts, d_pos, kIn, meshOf, passes, hist, seg, st);
    NTR_HIP(hipGetLastError());
    if (const int rc = read_totals(&h, st, s)) return rc;
    if (h.err & 1u) return set_error(NTR_ERR_INVALID, "%s: vertex index out of range", fn);
    if (h.err) return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x before the sort", fn, h.err);
    ev.mark(1);

    for (int p = 0; p < passes; p++) {
        if (p == PB_CODE_PASSES)   // the first pass over the mesh index fetches it by slot; it moves with the slot from here on
            onesweep_launch<PB_ITEMS, 2, false>(s, lay.tiles, n, (const unsigned int*)meshOf, (const int*)vIn, kOut, vOut, 1, 0, p, hist + 256 * p,
                                                tileState, misc + p, misc + kErrWord);
        else
            onesweep_launch<PB_ITEMS, 0, false>(s, lay.tiles, n, (const unsigned int*)kIn, p == 0 ? (const int*)nullptr : (const int*)vIn, kOut, vOut,
                                                1, p < PB_CODE_PASSES ? 8 * p : 8 * (p - PB_CODE_PASSES), p, hist + 256 * p, tileState, misc + p,
                                                misc + kErrWord);
        std::swap(kIn, kOut);
        std::swap(vIn, vOut);
    }
    NTR_HIP(hipGetLastError());
    ev.mark(2);
    pb_leaves<<<nbN, PB_BLOCK, 0, s>>>(n, numMeshes, d_meshes, d_tri, numVerts, d_pos, vIn, meshOf, bufs.b[0], n, (int*)d_nodes, (uint4*)d_woop,
                                       d_idx, st);
    NTR_HIP(hipGetLastError());
    ev.mark(3);

    int* nn = at<int>(base, lay.nn);
    U2 *local = at<U2>(base, lay.local), *blockSums = at<U2>(base, lay.blockSums);
    const int nbM = (numMeshes + PB_BLOCK - 1) / PB_BLOCK;
    int k = 0, len = n;   // rounds launched; the list length the host knows
    while (open > 0) {
        const int nb = len / PB_TILE + 1;   // tiles of len + 1 items
        for (int r = 0; r < kRoundsPerRead; r++, k++) {
            pb_search<<<nb, PB_TILE, 0, s>>>(k, st, bufs, n, radius, numMeshes, seg, nn);
            pb_mark<<<nb, PB_TILE, 0, s>>>(k, st, nn, local, blockSums);
            pb_sums<<<1, PB_TILE, 0, s>>>(k, st, blockSums);
            pb_update<<<nbM, PB_BLOCK, 0, s>>>(k, st, numMeshes, bufs, seg, local, blockSums);
            pb_scatter<<<nb, PB_TILE, 0, s>>>(k, st, bufs, n, numMeshes, seg, d_meshes, nn, local, blockSums, (int*)d_nodes);
        }
        NTR_HIP(hipGetLastError());
        if (const int rc = read_totals(&h, st, s)) return rc;
        const int now = h.n[k & 1];
        if (h.err || now < numMeshes || now >= len || h.open[k & 1] < 0 || h.open[k & 1] > open)
            return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x, %d clusters after %d, %d meshes open after %d", fn, h.err,
                             now, len, h.open[k & 1], open);
        len = now;
        open = h.open[k & 1];
    }
    ev.mark(4);
    std::vector<int> perMesh(2 * (size_t)numMeshes);
    unsigned int sortBad = 0;
    NTR_HIP(hipMemcpyAsync(perMesh.data(), seg.rounds, perMesh.size() * 4, hipMemcpyDeviceToHost, s));
    NTR_HIP(hipMemcpyAsync(&sortBad, misc + kErrWord, 4, hipMemcpyDeviceToHost, s));
    if (const int rc = read_totals(&h, st, s)) return rc;
    if (sortBad) return set_error(NTR_ERR_HIP, "%s: a chained scan timed out waiting for a predecessor tile (status %u)", fn, sortBad);
    if (h.err & 1u) return set_error(NTR_ERR_INVALID, "%s: vertex index out of range", fn);
    if (h.err || len != numMeshes)
        return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x, %d clusters left of %d meshes", fn, h.err, len, numMeshes);

    int maxRounds = 0, maxHeight = 0, tooHigh = -1;
    for (int m = 0; m < numMeshes; m++) {
        const int nt = meshes[m].numTris, rounds = perMesh[m], height = perMesh[(size_t)numMeshes + m];
        if (meshResults) meshResults[m] = NtrPlocBatchMeshResult{nt == 1 ? 1 : nt - 1, nt == 1 ? 2 : nt, rounds, height};
        maxRounds = std::max(maxRounds, rounds);
        maxHeight = std::max(maxHeight, height);
        if (height > kPlocMaxHeight && tooHigh < 0) tooHigh = m;
    }
    if (tooHigh >= 0)
        return set_error(NTR_ERR_OVERFLOW, "%s: mesh %d: the tree's height %d exceeds the %d entries of the reference CPU tracer's stack; the "
                         "pool is not to be traced", fn, tooHigh, perMesh[(size_t)numMeshes + tooHigh], kPlocMaxHeight);
    const NtrBlasRange& last = ranges[numMeshes - 1];
    res->numMeshes = numMeshes;
    res->numRounds = maxRounds;
    res->maxHeight = maxHeight;
    res->numTris = n;
    res->nodesBytes = last.nodesOffset + last.nodesBytes;
    res->triWoopBytes = last.triWoopOffset + last.triWoopBytes;
    res->triIndexBytes = res->triWoopBytes / 4;
    res->checkMs = ev.ms(0, 1);
    res->sortMs = ev.ms(1, 2);
    res->emitMs = ev.ms(2, 3);
    res->roundsMs = ev.ms(3, 4);
    res->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_ploc_batch_capacity(int32_t numMeshes, const NtrPlocBatchMesh* meshes, NtrBlasRange* ranges, int64_t* nodesBytes,
                            int64_t* triWoopBytes, int64_t* triIndexBytes)
{
    int64_t tris, nb, rows;
    if (const int rc = pb_plan("ntr_ploc_batch_capacity", numMeshes, meshes, ranges, &tris, &nb, &rows)) return rc;
    if (nodesBytes) *nodesBytes = nb;
    if (triWoopBytes) *triWoopBytes = rows * kRowBytes;
    if (triIndexBytes) *triIndexBytes = rows * 4;
    return NTR_OK;
}

int ntr_ploc_build_batch(int32_t numMeshes, const NtrPlocBatchMesh* meshes, int32_t numTrisTotal, const int32_t* d_triVtxIndex,
                         int32_t numVerts, const float* d_vtxPos, int32_t radius, void* d_poolNodes, int64_t nodesCapacity,
                         void* d_poolTriWoop, int64_t triWoopCapacity, int32_t* d_poolTriIndex, int64_t triIndexCapacity, NtrBlasRange* ranges,
                         NtrPlocBatchMeshResult* meshResults, NtrPlocBatchResult* result, void* stream)
{
    const char* fn = "ntr_ploc_build_batch";
    const auto wall0 = std::chrono::steady_clock::now();   // the checks and the layout below walk every mesh: part of the call's time
    if (!result) return set_error(NTR_ERR_INVALID, "%s: null result", fn);
    memset(result, 0, sizeof(*result));
    if (numTrisTotal < 1 || numVerts < 1 || !d_triVtxIndex || !d_vtxPos || !d_poolNodes || !d_poolTriWoop || !d_poolTriIndex || !ranges)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (numTrisTotal >= 1, numVerts >= 1, non-null buffers and ranges)", fn);
    if (radius < 1 || radius > kPlocMaxRadius) return set_error(NTR_ERR_INVALID, "%s: radius %d outside 1..%d", fn, (int)radius, kPlocMaxRadius);
    int64_t tris, nodesBytes, rows;
    if (const int rc = pb_plan(fn, numMeshes, meshes, ranges, &tris, &nodesBytes, &rows)) return rc;
    for (int k = 0; k < numMeshes; k++) {
        const NtrPlocBatchMesh& m = meshes[k];
        if (m.firstTri < 0 || (int64_t)m.firstTri + m.numTris > numTrisTotal)
            return set_error(NTR_ERR_INVALID, "%s: mesh %d: triangles [%d, +%d) lie outside [0, %d)", fn, k, (int)m.firstTri, (int)m.numTris,
                             (int)numTrisTotal);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(m.sceneMin[a]) || !std::isfinite(m.sceneMax[a]) || m.sceneMin[a] > m.sceneMax[a])
                return set_error(NTR_ERR_INVALID, "%s: mesh %d: the box must be finite with min <= max on every axis", fn, k);
    }
    if (nodesCapacity < nodesBytes || triWoopCapacity < rows * kRowBytes || triIndexCapacity < rows * 4)
        return set_error(NTR_ERR_INVALID, "%s: pool buffers smaller than ntr_ploc_batch_capacity()", fn);
    if (((uintptr_t)d_poolNodes | (uintptr_t)d_poolTriWoop) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the pool's nodes and triWoop must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads back per four rounds and cannot be captured", fn);
    return finish_build(pb_build(numMeshes, meshes, (int)tris, d_triVtxIndex, numVerts, d_vtxPos, radius, d_poolNodes, d_poolTriWoop,
                                 d_poolTriIndex, ranges, meshResults, result, s, wall0), result, s);
}

int ntr_ploc_batch_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_ploc_batch_scratch_bytes", g_pbPool, bytes); }

}  // extern "C"
