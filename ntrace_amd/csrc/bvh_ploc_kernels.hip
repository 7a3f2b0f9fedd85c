// bvh_ploc_kernels.hip -- on-device PLOC build for gfx950 (ntr_ploc_build): parallel locally-ordered clustering (Meister and Bittner
// 2018) over the LBVH's Morton order.  EXTENSION: the reference has no PLOC; the rule is the numpy spec tests/np_bvh_ploc.py, which the
// build equals byte for byte.
//   before the rounds  pl_check: every vertex index (the LBVH's Morton kernel reads the mesh unchecked), one read-back
//                      lbvh_sort_codes (lbvh_kernels.hip): the LBVH's own codes and stable sort, same launches
//                      pl_leaves: one cluster per triangle in sorted order (box by ord_min / ord_max, link ~(4p), height 0), its
//                        terminator row and its leaf row; emit_leaf_rows (device_prims.h): the Woop rows and triIndex entries
//   per round          pl_search: a workgroup stages its tile's boxes plus a halo of R clusters on either side in LDS, [component][cluster],
//                        so that the lanes of a wave read consecutive words; each lane evaluates its 2R unions from there and keeps
//                        the least key (d, k, b)
//                      pl_mark + pl_sums: the mutual test, a scan of (survivors, merging pairs), the next round's list length
//                      pl_scatter: the merged clusters' node records, the compacted list into the other cluster buffer
//   tail               pl_tail: once the list has at most NTR_PLOC_TAIL clusters one workgroup runs all remaining rounds out of LDS in
//                        one launch: same rule, same bytes
// Every kernel of a round reads the list length from a 32-byte device record (PlState), so the host launches kRoundsPerRead rounds
// with grids sized by the last length it knows and reads the record back once per such group; a round that finds the list already at
// or below the tail length does nothing.  The record's fields are double buffered by the parity of the launch counter: a round reads
// one half and writes the other.  No result depends on how often the host reads.
// Distances keep the spec's order of operations (__fmul_rn / __fadd_rn, and the library is compiled without contraction).
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "ntr_internal.h"
#include "level_build.h"
#include "ploc_rounds.h"

namespace ntr {
namespace {

constexpr int PL_TILE = NTR_PLOC_TILE;   // clusters of a workgroup of the round kernels, one per thread
constexpr int PL_TAIL = NTR_PLOC_TAIL;   // the tail workgroup's threads, one cluster each
constexpr int PL_MAX_RADIUS = kPlocMaxRadius;
constexpr int PL_BLOCK = 256;            // per-triangle kernels
constexpr int kRoundsPerRead = 4;
constexpr int kMaxHeight = kPlocMaxHeight;
static_assert(PL_TILE == 1024 && PL_TAIL <= 1024 && PL_TAIL >= 2, "one cluster per thread of a 1024-thread workgroup");

// ---- before the rounds --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_BLOCK) void pl_check(int n, const int* __restrict__ tri, int numVerts, PlState* __restrict__ st)
{
    const int t = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (t >= n) return;
    int i0, i1, i2;
    if (!tri_indices_checked(tri, numVerts, t, i0, i1, i2)) atomicOr(&st->err, 1u);
}

__global__ __launch_bounds__(PL_BLOCK) void pl_leaves(int n, const int* __restrict__ tri, int numVerts, const float* __restrict__ pos,
                                                      const int* __restrict__ sorted, PlBuf out, int cap, int* __restrict__ leafRow,
                                                      uint4* __restrict__ woop, int* __restrict__ triIndex, PlState* __restrict__ st)
{
    const int p = blockIdx.x * PL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int t = sorted[p];
    float lo[3], hi[3];
    if (t < 0 || t >= n || !tri_box_checked(tri, numVerts, pos, t, lo, hi)) { atomicOr(&st->err, 1u); return; }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        out.box[(size_t)c * cap + p] = lo[c];
        out.box[(size_t)(3 + c) * cap + p] = hi[c];
    }
    out.link[p] = leaf_link(4 * p);
    out.height[p] = 0;
    leafRow[t] = 4 * p;
    write_leaf_terminator(woop, triIndex, 4ll * p + 3);
}

// N == 1: an empty child 0 (a terminator row only) and the triangle in child 1, the rows of ntr_persistent_bvh_build's one-triangle tree
__global__ void pl_single(const int* __restrict__ tri, int numVerts, const float* __restrict__ pos, int* __restrict__ nodes,
                          uint4* __restrict__ woop, int* __restrict__ triIndex, int* __restrict__ leafRow)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float b0[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}, b1[6];
    if (!tri_box_checked(tri, numVerts, pos, 0, b1, b1 + 3)) return;   // pl_check has passed
    pl_write_node(nodes, 0, b0, leaf_link(0), b1, leaf_link(1));
    write_leaf_terminator(woop, triIndex, 0);
    write_leaf_terminator(woop, triIndex, 4);
    leafRow[0] = 1;
}

// ---- a round --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_TILE) void pl_search(int k, const PlState* __restrict__ st, PlBufs bufs, int cap, int radius,
                                                     int* __restrict__ nn)
{
    constexpr int STRIDE = PL_TILE + 2 * PL_MAX_RADIUS;
    __shared__ float s_box[6 * STRIDE];
    const int n = st->n[k & 1];
    const int base = blockIdx.x * PL_TILE;
    if (n <= PL_TAIL || base >= n) return;
    const float* box = bufs.b[st->cur[k & 1]].box;
    for (int l = threadIdx.x; l < PL_TILE + 2 * radius; l += PL_TILE) {
        const int g = base - radius + l;
        if (g >= 0 && g < n) {
#pragma unroll
            for (int c = 0; c < 6; c++) s_box[c * STRIDE + l] = box[(size_t)c * cap + g];
        }
    }
    __syncthreads();
    const int i = base + threadIdx.x;
    if (i < n) nn[i] = pl_nearest(s_box, STRIDE, threadIdx.x + radius, i, n, radius);
}

__global__ __launch_bounds__(PL_TILE) void pl_mark(int k, const PlState* __restrict__ st, const int* __restrict__ nn, U2* __restrict__ local,
                                                   U2* __restrict__ blockSums)
{
    const int n = st->n[k & 1];
    if (n <= PL_TAIL || blockIdx.x * PL_TILE >= n) return;
    const int i = blockIdx.x * PL_TILE + threadIdx.x;
    U2 v{0u, 0u};
    if (i < n) {
        const int j = nn[i];
        const bool mutual = j >= 0 && j < n && nn[j] == i;
        v.x = (mutual && i > j) ? 0u : 1u;
        v.y = (mutual && i < j) ? 1u : 0u;
    }
    scan_local_store<PL_TILE>(v, i < n, (size_t)i, local, blockSums, (int)blockIdx.x);
}

// one workgroup: the block sums' exclusive scan in place, and the other half of the record
__global__ __launch_bounds__(PL_TILE) void pl_sums(int k, PlState* __restrict__ st, U2* __restrict__ blockSums)
{
    const int p = k & 1, q = p ^ 1;
    const int n = st->n[p];
    const bool active = n > PL_TAIL;
    U2 carry{0u, 0u};
    if (active) {
        const int nb = (n + PL_TILE - 1) / PL_TILE;
        for (int base = 0; base < nb; base += PL_TILE) {
            const int i = base + threadIdx.x;
            const U2 v = i < nb ? blockSums[i] : U2{0u, 0u};
            U2 chunk;
            const U2 ex = block_exclusive_scan<PL_TILE>(v, &chunk);
            if (i < nb) blockSums[i] = carry + ex;
            carry = carry + chunk;
        }
    }
    if (threadIdx.x == 0) {
        if (active && carry.y == 0u) atomicOr(&st->err, 8u);
        st->n[q] = active ? n - (int)carry.y : n;
        st->rounds[q] = st->rounds[p] + (active ? 1 : 0);
        st->cur[q] = st->cur[p] ^ (active ? 1 : 0);
    }
}

__global__ __launch_bounds__(PL_TILE) void pl_scatter(int k, PlState* __restrict__ st, PlBufs bufs, int cap, const int* __restrict__ nn,
                                                      const U2* __restrict__ local, const U2* __restrict__ blockSums, int* __restrict__ nodes,
                                                      int nodeCap)
{
    const int p = k & 1;
    const int n = st->n[p];
    const int i = blockIdx.x * PL_TILE + threadIdx.x;
    if (n <= PL_TAIL || i >= n) return;
    const int m = n - st->n[p ^ 1];
    const PlBuf in = bufs.b[st->cur[p]], out = bufs.b[st->cur[p] ^ 1];
    const int j = nn[i];
    const bool mutual = j >= 0 && j < n && nn[j] == i;
    if (mutual && i > j) return;
    const U2 e = local[i] + blockSums[blockIdx.x];
    const int dst = (int)e.x;
    if (dst < 0 || dst >= n - m) { atomicOr(&st->err, 4u); return; }
    float a[6];
#pragma unroll
    for (int c = 0; c < 6; c++) a[c] = in.box[(size_t)c * cap + i];
    int link = in.link[i], height = in.height[i];
    if (mutual) {
        const int slot = (n - 1 - m) + (int)e.y;
        if (slot < 0 || slot >= nodeCap) { atomicOr(&st->err, 4u); return; }
        float b[6];
#pragma unroll
        for (int c = 0; c < 6; c++) b[c] = in.box[(size_t)c * cap + j];
        pl_write_node(nodes, slot, a, link, b, in.link[j]);
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
}

// ---- the tail: every remaining round in one workgroup, the list in LDS -------------------------------------------------------------
__global__ __launch_bounds__(PL_TAIL) void pl_tail(int k, PlState* __restrict__ st, PlBufs bufs, int cap, int radius, int* __restrict__ nodes,
                                                   int nodeCap)
{
    __shared__ float s_box[6 * PL_TAIL];
    __shared__ int s_link[PL_TAIL], s_height[PL_TAIL], s_nn[PL_TAIL];
    const int p = k & 1;
    int n = st->n[p];
    if (n > PL_TAIL) return;   // not handed over (the host reports it)
    const int i = threadIdx.x;
    {
        const PlBuf in = bufs.b[st->cur[p]];
        if (i < n) {
#pragma unroll
            for (int c = 0; c < 6; c++) s_box[c * PL_TAIL + i] = in.box[(size_t)c * cap + i];
            s_link[i] = in.link[i];
            s_height[i] = in.height[i];
        }
    }
    __syncthreads();
    int rounds = 0;
    unsigned int err = 0u;
    while (n > 1) {
        if (i < n) s_nn[i] = pl_nearest(s_box, PL_TAIL, i, i, n, radius);
        __syncthreads();
        int j = -1;
        bool mutual = false;
        if (i < n) {
            j = s_nn[i];
            mutual = j >= 0 && j < n && s_nn[j] == i;
        }
        const bool survives = i < n && !(mutual && i > j), merges = mutual && i < j;
        U2 total;
        const U2 e = block_exclusive_scan<PL_TAIL>(U2{survives ? 1u : 0u, merges ? 1u : 0u}, &total);
        const int m = (int)total.y;
        if (m == 0) { err = 8u; break; }   // the same in every thread
        float a[6];
        int link = 0, height = 0;
        if (survives) {
#pragma unroll
            for (int c = 0; c < 6; c++) a[c] = s_box[c * PL_TAIL + i];
            link = s_link[i];
            height = s_height[i];
            if (merges) {
                const int slot = (n - 1 - m) + (int)e.y;
                float b[6];
#pragma unroll
                for (int c = 0; c < 6; c++) b[c] = s_box[c * PL_TAIL + j];
                if (slot < 0 || slot >= nodeCap) err = 4u;
                else pl_write_node(nodes, slot, a, link, b, s_link[j]);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    a[c] = ord_min(a[c], b[c]);
                    a[3 + c] = ord_max(a[3 + c], b[3 + c]);
                }
                link = inner_link(slot);
                height = 1 + max(height, s_height[j]);
            }
        }
        __syncthreads();   // every read of the old list is done
        if (survives) {
            const int dst = (int)e.x;
#pragma unroll
            for (int c = 0; c < 6; c++) s_box[c * PL_TAIL + dst] = a[c];
            s_link[dst] = link;
            s_height[dst] = height;
        }
        __syncthreads();
        n -= m;
        rounds++;
    }
    if (err) atomicOr(&st->err, err);
    if (i == 0) {
        st->n[p ^ 1] = n;
        st->rounds[p ^ 1] = st->rounds[p] + rounds;
        st->cur[p ^ 1] = st->cur[p];
        st->height = s_height[0];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct PlLayout {
    size_t sort, leafRow, off;
    PlRoundsLayout rounds;
    explicit PlLayout(int64_t n)
    {
        ScratchCarver cv;
        sort = cv.take(n >= 2 ? lbvh_sort_scratch_bytes((int)n) : 0);
        rounds.carve(cv, n);
        leafRow = cv.take((size_t)n * 4);
        off = cv.off;
    }
};

DeviceScratchPool g_plPool;

int pl_build(int n, const int32_t* d_tri, int32_t numVerts, const float* d_pos, const float* sceneMin, const float* sceneMax, int radius,
             void* d_nodes, int64_t nodeCap, void* d_woop, int64_t rowCap, int32_t* d_idx, NtrPlocResult* res, hipStream_t s)
{
    const char* fn = "ntr_ploc_build";
    const auto wall0 = std::chrono::steady_clock::now();
    const PlLayout lay((int64_t)n);
    void* base = nullptr;
    if (const int rc = first_block(g_plPool, lay.off, &base)) return rc;
    PlState* st = at<PlState>(base, lay.rounds.state);
    int* leafRow = at<int>(base, lay.leafRow);
    const PlBufs bufs = pl_bufs(base, lay.rounds);

    StreamEvents<6> ev(s);
    (void)ev.create();
    ev.mark(0);
    PlState h;
    memset(&h, 0, sizeof(h));
    h.n[0] = n;
    NTR_HIP(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    const int nbN = (n + PL_BLOCK - 1) / PL_BLOCK;
    pl_check<<<nbN, PL_BLOCK, 0, s>>>(n, d_tri, numVerts, st);
    NTR_HIP(hipGetLastError());
    if (const int rc = read_totals(&h, st, s)) return rc;
    if (h.err & 1u) return set_error(NTR_ERR_INVALID, "%s: vertex index out of range", fn);
    ev.mark(1);

    const unsigned int* sortErr = nullptr;
    int tailClusters = 0;
    if (n == 1) {
        ev.mark(2);
        pl_single<<<1, 64, 0, s>>>(d_tri, numVerts, d_pos, (int*)d_nodes, (uint4*)d_woop, d_idx, leafRow);
        emit_leaf_rows<PL_BLOCK><<<1, PL_BLOCK, 0, s>>>(1, d_tri, d_pos, (const unsigned char*)nullptr, leafRow, (int)rowCap, (float4*)d_woop, d_idx,
                                                        &st->err, 2u);
        NTR_HIP(hipGetLastError());
        ev.mark(3);
        ev.mark(4);
        ev.mark(5);
        if (const int rc = read_totals(&h, st, s)) return rc;
        if (h.err) return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x", fn, h.err);
        h.height = 1;
    } else {
        const unsigned int* keys = nullptr;
        const int* sorted = nullptr;
        if (const int rc = lbvh_sort_codes(n, d_tri, d_pos, sceneMin, sceneMax, at<char>(base, lay.sort), s, &keys, &sorted, &sortErr)) return rc;
        ev.mark(2);
        pl_leaves<<<nbN, PL_BLOCK, 0, s>>>(n, d_tri, numVerts, d_pos, sorted, bufs.b[0], n, leafRow, (uint4*)d_woop, d_idx, st);
        emit_leaf_rows<PL_BLOCK><<<nbN, PL_BLOCK, 0, s>>>(n, d_tri, d_pos, (const unsigned char*)nullptr, leafRow, (int)rowCap, (float4*)d_woop, d_idx,
                                                          &st->err, 2u);
        NTR_HIP(hipGetLastError());
        ev.mark(3);

        int k = 0, len = n;   // launch groups so far; the list length the host knows
        if (const int rc = ploc_rounds(fn, base, lay.rounds, n, radius, d_nodes, (int)nodeCap, s, &k, &len)) return rc;
        ev.mark(4);
        tailClusters = len;
        if (const int rc = ploc_tail(base, lay.rounds, n, radius, d_nodes, (int)nodeCap, s, &k)) return rc;
        ev.mark(5);
        unsigned int sortBad = 0;
        NTR_HIP(hipMemcpyAsync(&sortBad, sortErr, 4, hipMemcpyDeviceToHost, s));
        if (const int rc = read_totals(&h, st, s)) return rc;
        if (sortBad) return set_error(NTR_ERR_HIP, "%s: a chained scan timed out waiting for a predecessor tile (status %u)", fn, sortBad);
        if (h.err & 1u) return set_error(NTR_ERR_INVALID, "%s: vertex index out of range", fn);
        if (h.err || h.n[k & 1] != 1)
            return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x, %d clusters left", fn, h.err, h.n[k & 1]);
        h.rounds[0] = h.rounds[k & 1];
    }
    if (h.height > kMaxHeight)
        return set_error(NTR_ERR_OVERFLOW, "%s: the tree's height %d exceeds the %d entries of the reference CPU tracer's stack; the buffers "
                         "are not to be traced", fn, h.height, kMaxHeight);
    const int64_t rows = n == 1 ? 5 : 4ll * n;
    res->numNodes = n == 1 ? 1 : n - 1;
    res->numLeaves = n == 1 ? 2 : n;
    res->numRounds = n == 1 ? 0 : h.rounds[0];
    res->height = h.height;
    res->tailClusters = tailClusters;
    res->nodesBytes = (int64_t)res->numNodes * kNodeBytes;
    res->triWoopBytes = rows * kRowBytes;
    res->triIndexBytes = rows * 4;
    res->mortonMs = ev.ms(0, 1);
    res->sortMs = ev.ms(1, 2);
    res->emitMs = ev.ms(2, 3);
    res->roundsMs = ev.ms(3, 4);
    res->tailMs = ev.ms(4, 5);
    res->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace

// ---- the rounds, for this file's pl_build and for ntr_tlas_build (ploc_rounds.h) ----------------------------------------------------
int ploc_rounds(const char* fn, void* base, const PlRoundsLayout& lay, int cap, int radius, void* d_nodes, int nodeCap, hipStream_t s,
                int* kp, int* lenp)
{
    PlState* st = at<PlState>(base, lay.state);
    int* nn = at<int>(base, lay.nn);
    U2 *local = at<U2>(base, lay.local), *blockSums = at<U2>(base, lay.blockSums);
    const PlBufs bufs = pl_bufs(base, lay);
    PlState h;
    int k = *kp, len = *lenp;
    while (len > PL_TAIL) {
        const int nb = (len + PL_TILE - 1) / PL_TILE;
        for (int r = 0; r < kRoundsPerRead; r++, k++) {
            pl_search<<<nb, PL_TILE, 0, s>>>(k, st, bufs, cap, radius, nn);
            pl_mark<<<nb, PL_TILE, 0, s>>>(k, st, nn, local, blockSums);
            pl_sums<<<1, PL_TILE, 0, s>>>(k, st, blockSums);
            pl_scatter<<<nb, PL_TILE, 0, s>>>(k, st, bufs, cap, nn, local, blockSums, (int*)d_nodes, nodeCap);
        }
        NTR_HIP(hipGetLastError());
        if (const int rc = read_totals(&h, st, s)) return rc;
        const int now = h.n[k & 1];
        if (h.err || now < 1 || now >= len)
            return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x, %d clusters after %d of round %d", fn, h.err, now, len,
                             h.rounds[k & 1]);
        len = now;
    }
    *kp = k;
    *lenp = len;
    return NTR_OK;
}

int ploc_tail(void* base, const PlRoundsLayout& lay, int cap, int radius, void* d_nodes, int nodeCap, hipStream_t s, int* k)
{
    pl_tail<<<1, PL_TAIL, 0, s>>>(*k, at<PlState>(base, lay.state), pl_bufs(base, lay), cap, radius, (int*)d_nodes, nodeCap);
    ++*k;
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_ploc_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos, const float sceneMin[3],
                   const float sceneMax[3], int32_t radius, void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                   int32_t* d_triIndex, int64_t triIndexCapacity, NtrPlocResult* result, void* stream)
{
    const char* fn = "ntr_ploc_build";
    if (!result) return set_error(NTR_ERR_INVALID, "%s: null result", fn);
    memset(result, 0, sizeof(*result));
    if (const int rc = check_build_geometry(fn, numTris, numVerts, d_triVtxIndex, d_vtxPos, sceneMin && sceneMax, ", a scene box")) return rc;
    if (radius < 1 || radius > PL_MAX_RADIUS) return set_error(NTR_ERR_INVALID, "%s: radius %d outside 1..%d", fn, (int)radius, PL_MAX_RADIUS);
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(sceneMin[a]) || !std::isfinite(sceneMax[a]) || sceneMin[a] > sceneMax[a])
            return set_error(NTR_ERR_INVALID, "%s: the scene box must be finite with min <= max on every axis", fn);
    int64_t nodeCap, rowCap;
    if (const int rc = check_build_outputs(fn, numTris, d_nodes, nodesCapacity, d_triWoop, triWoopCapacity, d_triIndex, triIndexCapacity,
                                           &nodeCap, &rowCap))
        return rc;
    if ((int64_t)numTris - 1 > kMaxNodes)
        return set_error(NTR_ERR_OVERFLOW, "%s: %lld triangles make %lld inner nodes, more than the %lld that BVHLayout_Compact's 32-bit "
                         "child offsets address", fn, (long long)numTris, (long long)numTris - 1, (long long)kMaxNodes);
    hipStream_t s = (hipStream_t)stream;
    return finish_build(pl_build(numTris, d_triVtxIndex, numVerts, d_vtxPos, sceneMin, sceneMax, radius, d_nodes, nodeCap, d_triWoop, rowCap,
                                 d_triIndex, result, s), result, s);
}

int ntr_ploc_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_ploc_scratch_bytes", g_plPool, bytes); }

}  // extern "C"
