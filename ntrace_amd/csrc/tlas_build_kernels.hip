// tlas_build_kernels.hip -- on-device build of a top-level tree over instances for gfx950 (ntr_tlas_build), and the host's
// ntr_instance_invert.  EXTENSION: the reference has no instancing; the rule is the numpy spec tests/np_instanced.py, which the build
// equals bit for bit.  instanced_bvh.h states the pool, the record and the limits.
//   tl_boxes      one thread per instance: checks its BLAS index against the range table, reads node 0 of its BLAS, forms the world box
//                 (eight corners through objectToWorld, min / max in the total order), writes record i and folds the box into the
//                 scene box (device_prims.h's six words merged by integer max, one atomic set per wave)
//   tl_codes      the LBVH's Morton code of every world box over that scene box, and the sort's digit histograms
//   sort          radix_sort.h: four one-sweep passes over the 30-bit codes (stable; values start as the instance index)
//   tl_clusters   the cluster list in sorted order: (world box, link ~i, height 0)
//   rounds        the PLOC rounds themselves (ploc_rounds.h: bvh_ploc_kernels.hip's kernels and loop), then its tail
// Arithmetic keeps the spec's order of operations; the library is compiled without contraction.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "ntr_internal.h"
#include "instance_math.h"
#include "instanced_bvh.h"
#include "level_build.h"
#include "ploc_rounds.h"
#include "radix_sort.h"

namespace ntr {
namespace {

constexpr int TL_BLOCK = 256;
constexpr int TL_ITEMS = 8;      // keys per thread of a sort tile: a frame's instances are thousands, not millions
constexpr int TL_PASSES = 4;     // 30-bit codes
static_assert(TL_BLOCK % 64 == 0, "whole waves fold the scene box");

// xform's component (np_instanced.py): r = 0; r += a0 * x; r += a1 * y; r += a2 * z; r += a3 * w
__device__ __forceinline__ float tl_dot4(const float* a, float x, float y, float z, float w)
{
    float r = 0.0f;
    r += a[0] * x;
    r += a[1] * y;
    r += a[2] * z;
    r += a[3] * w;
    return r;
}

__global__ __launch_bounds__(TL_BLOCK) void tl_boxes(int n, const NtrInstance* __restrict__ inst, int numBlas, const uint4* __restrict__ table,
                                                     const char* __restrict__ poolNodes, float* __restrict__ instBox,
                                                     uint4* __restrict__ records, unsigned int* __restrict__ scene, PlState* __restrict__ st)
{
    const int i = blockIdx.x * TL_BLOCK + threadIdx.x;
    unsigned int w[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // the empty box: lanes without an instance fold nothing in
    if (i < n) {
        const int b = inst[i].blas;
        if (b < 0 || b >= numBlas) {
            atomicOr(&st->err, 1u);
        } else {
            const uint4 range = table[b];   // nodesOffset, row offset, nodesBytes, 0 (the host has checked it against the pool)
            const float4* nd = (const float4*)(poolNodes + range.x);
            const float4 n0 = nd[0], n1 = nd[1], nz = nd[2];
            // the object box: the union of node 0's child boxes (an empty child, (FLT_MAX, -FLT_MAX), drops out by itself)
            const float lo[3] = {ord_min(n0.x, n1.x), ord_min(n0.z, n1.z), ord_min(nz.x, nz.z)};
            const float hi[3] = {ord_max(n0.y, n1.y), ord_max(n0.w, n1.w), ord_max(nz.y, nz.w)};
            float m[12], inv[12];
#pragma unroll
            for (int k = 0; k < 12; k++) { m[k] = inst[i].objectToWorld[k]; inv[k] = inst[i].worldToObject[k]; }
            float wlo[3], whi[3];
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const float x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    const float p = tl_dot4(m + 4 * r, x, y, z, 1.0f);
                    wlo[r] = c == 0 ? p : ord_min(wlo[r], p);
                    whi[r] = c == 0 ? p : ord_max(whi[r], p);
                }
            }
#pragma unroll
            for (int r = 0; r < 3; r++) {
                instBox[(size_t)r * n + i] = wlo[r];
                instBox[(size_t)(3 + r) * n + i] = whi[r];
            }
            uint4* rec = records + 4 * (size_t)i;
            rec[0] = make_uint4(__float_as_uint(inv[0]), __float_as_uint(inv[1]), __float_as_uint(inv[2]), __float_as_uint(inv[3]));
            rec[1] = make_uint4(__float_as_uint(inv[4]), __float_as_uint(inv[5]), __float_as_uint(inv[6]), __float_as_uint(inv[7]));
            rec[2] = make_uint4(__float_as_uint(inv[8]), __float_as_uint(inv[9]), __float_as_uint(inv[10]), __float_as_uint(inv[11]));
            rec[3] = make_uint4(range.x, range.y, range.z, 0u);
            box_words(make_float4(wlo[0], wlo[1], wlo[2], 0.0f), make_float4(whi[0], whi[1], whi[2], 0.0f), w);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) w[k] = wave_max_u32(w[k]);
    if ((threadIdx.x & 63) == 0 && (w[3] | w[4] | w[5]) != 0u) atomic_max_box(scene, w);   // (ord_enc is never 0 for a float: 0 is "no member")
}

// emitTreeKernel.cu:647-653
__device__ __forceinline__ unsigned int tl_spread(unsigned int v)
{
    v &= 0x3ffu;
    v = (v ^ (v << 16)) & 0xff0000ffu;
    v = (v ^ (v << 8)) & 0x0300f00fu;
    v = (v ^ (v << 4)) & 0x030c30c3u;
    return (v ^ (v << 2)) & 0x09249249u;
}

__global__ __launch_bounds__(TL_BLOCK) void tl_codes(int n, const float* __restrict__ instBox, const unsigned int* __restrict__ scene,
                                                     unsigned int* __restrict__ keys, unsigned int* __restrict__ hist /* [TL_PASSES][256], zeroed */)
{
    __shared__ unsigned int s_hist[TL_PASSES][256];
    for (int k = threadIdx.x; k < TL_PASSES * 256; k += TL_BLOCK) (&s_hist[0][0])[k] = 0u;
    __syncthreads();
    const int i = blockIdx.x * TL_BLOCK + threadIdx.x;
    if (i < n) {
        unsigned int sw[6];
#pragma unroll
        for (int k = 0; k < 6; k++) sw[k] = scene[k];
        float mn[3], mx[3];
        words_box(1, sw, 0.0f, false, mn, mx);
        unsigned int cell[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float step = (mx[a] - mn[a]) / 1024.0f;
            const float lo = instBox[(size_t)a * n + i], hi = instBox[(size_t)(3 + a) * n + i];
            const float mid = lo + (hi - lo) / 2.0f;
            const float q = (mid - mn[a]) / step;
            cell[a] = !(q >= 0.0f) ? 0u : (q >= 1024.0f ? 1023u : (unsigned int)floorf(q));
        }
        const unsigned int key = tl_spread(cell[0]) | (tl_spread(cell[1]) << 1) | (tl_spread(cell[2]) << 2);
        keys[i] = key;
#pragma unroll
        for (int p = 0; p < TL_PASSES; p++) atomicAdd(&s_hist[p][(key >> (8 * p)) & 255u], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TL_PASSES * 256; k += TL_BLOCK) {
        const unsigned int v = (&s_hist[0][0])[k];
        if (v) atomicAdd(&hist[k], v);
    }
}

__global__ __launch_bounds__(TL_BLOCK) void tl_clusters(int n, const int* __restrict__ sorted, const float* __restrict__ instBox, PlBuf out,
                                                        int cap, PlState* __restrict__ st)
{
    const int p = blockIdx.x * TL_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int i = sorted[p];
    if (i < 0 || i >= n) { atomicOr(&st->err, 4u); return; }
#pragma unroll
    for (int c = 0; c < 6; c++) out.box[(size_t)c * cap + p] = instBox[(size_t)c * n + i];
    out.link[p] = leaf_link(i);
    out.height[p] = 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct TlLayout {
    size_t keys[2], idx[2], zero, zeroBytes, hist, misc, tileState, scene, table, instBox, off;
    int tiles;
    PlRoundsLayout rounds;
    TlLayout(int64_t n, int64_t numBlas)
    {
        ScratchCarver cv;
        tiles = (int)((n + OS_THREADS * TL_ITEMS - 1) / (OS_THREADS * TL_ITEMS));
        for (int k = 0; k < 2; k++) { keys[k] = cv.take((size_t)n * 4); idx[k] = cv.take((size_t)n * 4); }
        // one zeroed block: the scene box's words, the digit histograms, tickets and error flag, the tile state of the chained scans
        zero = scene = cv.take(256);
        hist = cv.take(TL_PASSES * 256 * 4);
        misc = cv.take(64);
        tileState = cv.take((size_t)tiles * 256 * 8);
        zeroBytes = cv.off - zero;
        table = cv.take((size_t)numBlas * 16);
        instBox = cv.take((size_t)n * 24);
        rounds.carve(cv, n);
        off = cv.off;
    }
};

DeviceScratchPool g_tlPool;

int tl_build(int n, const NtrInstance* d_inst, int numBlas, const NtrBlasRange* ranges, const void* d_poolNodes, int radius, void* d_nodes,
             void* d_records, NtrTlasResult* res, hipStream_t s)
{
    const char* fn = "ntr_tlas_build";
    const auto wall0 = std::chrono::steady_clock::now();
    const TlLayout lay((int64_t)n, (int64_t)numBlas);
    void* base = nullptr;
    if (const int rc = first_block(g_tlPool, lay.off, &base)) return rc;
    PlState* st = at<PlState>(base, lay.rounds.state);
    unsigned int* scene = at<unsigned int>(base, lay.scene);
    float* instBox = at<float>(base, lay.instBox);
    const PlBufs bufs = pl_bufs(base, lay.rounds);

    StreamEvents<6> ev(s);
    (void)ev.create();
    ev.mark(0);
    PlState h;
    memset(&h, 0, sizeof(h));
    h.n[0] = n;
    NTR_HIP(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    NTR_HIP(hipMemsetAsync(at<char>(base, lay.zero), 0, lay.zeroBytes, s));
    std::vector<uint32_t> table(4 * (size_t)numBlas);   // (lives until the read-back below has drained the stream)
    for (int k = 0; k < numBlas; k++) {
        table[4 * k] = (uint32_t)ranges[k].nodesOffset;
        table[4 * k + 1] = (uint32_t)(ranges[k].triWoopOffset / kRowBytes);
        table[4 * k + 2] = (uint32_t)ranges[k].nodesBytes;
        table[4 * k + 3] = 0u;
    }
    NTR_HIP(hipMemcpyAsync(at<char>(base, lay.table), table.data(), table.size() * 4, hipMemcpyHostToDevice, s));
    const int nbN = (n + TL_BLOCK - 1) / TL_BLOCK;
    tl_boxes<<<nbN, TL_BLOCK, 0, s>>>(n, d_inst, numBlas, at<uint4>(base, lay.table), (const char*)d_poolNodes, instBox, (uint4*)d_records,
                                      scene, st);
    NTR_HIP(hipGetLastError());
    unsigned int sw[6];
    NTR_HIP(hipMemcpyAsync(sw, scene, sizeof(sw), hipMemcpyDeviceToHost, s));
    if (const int rc = read_totals(&h, st, s)) return rc;
    if (h.err & 1u) return set_error(NTR_ERR_INVALID, "%s: an instance's blas index lies outside [0, %d)", fn, numBlas);
    ev.mark(1);

    int tailClusters = 0;
    if (n == 1) {
        for (int k = 2; k < 6; k++) ev.mark(k);
        NTR_HIP(hipStreamSynchronize(s));
        h.height = 0;
    } else {
        unsigned int* hist = at<unsigned int>(base, lay.hist);
        unsigned int* misc = at<unsigned int>(base, lay.misc);   // [0..3] tickets, [4] the chained scans' error flag
        unsigned long long* tileState = at<unsigned long long>(base, lay.tileState);
        unsigned int *kIn = at<unsigned int>(base, lay.keys[0]), *kOut = at<unsigned int>(base, lay.keys[1]);
        int *vIn = at<int>(base, lay.idx[0]), *vOut = at<int>(base, lay.idx[1]);
        tl_codes<<<nbN, TL_BLOCK, 0, s>>>(n, instBox, scene, kIn, hist);
        for (int p = 0; p < TL_PASSES; p++) {
            onesweep_launch<TL_ITEMS, 0, false>(s, lay.tiles, n, (const unsigned int*)kIn, p == 0 ? (const int*)nullptr : (const int*)vIn, kOut, vOut,
                                                1, 8 * p, p, hist + 256 * p, tileState, misc + p, misc + 4);
            std::swap(kIn, kOut);
            std::swap(vIn, vOut);
        }
        NTR_HIP(hipGetLastError());
        ev.mark(2);
        tl_clusters<<<nbN, TL_BLOCK, 0, s>>>(n, vIn, instBox, bufs.b[0], n, st);   // (an even number of passes: the order is back in idx[0])
        NTR_HIP(hipGetLastError());
        ev.mark(3);
        int k = 0, len = n;
        if (const int rc = ploc_rounds(fn, base, lay.rounds, n, radius, d_nodes, n - 1, s, &k, &len)) return rc;
        ev.mark(4);
        tailClusters = len;
        if (const int rc = ploc_tail(base, lay.rounds, n, radius, d_nodes, n - 1, s, &k)) return rc;
        ev.mark(5);
        unsigned int sortBad = 0;
        NTR_HIP(hipMemcpyAsync(&sortBad, misc + 4, 4, hipMemcpyDeviceToHost, s));
        if (const int rc = read_totals(&h, st, s)) return rc;
        if (sortBad) return set_error(NTR_ERR_HIP, "%s: a chained scan timed out waiting for a predecessor tile (status %u)", fn, sortBad);
        if (h.err || h.n[k & 1] != 1)
            return set_error(NTR_ERR_LAYOUT, "%s: internal check failed: error 0x%x, %d clusters left", fn, h.err, h.n[k & 1]);
        h.rounds[0] = h.rounds[k & 1];
    }
    if (h.height > kPlocMaxHeight)
        return set_error(NTR_ERR_OVERFLOW, "%s: the top-level tree's height %d exceeds %d; the buffers are not to be traced", fn, h.height,
                         kPlocMaxHeight);
    res->rootLink = n == 1 ? leaf_link(0) : 0;
    res->numNodes = n - 1;
    res->numRounds = n == 1 ? 0 : h.rounds[0];
    res->height = h.height;
    res->tailClusters = tailClusters;
    res->nodesBytes = (int64_t)(n - 1) * kNodeBytes;
    res->recordsBytes = (int64_t)n * kRecordBytes;
    for (int a = 0; a < 3; a++) {
        res->sceneMin[a] = ord_dec(~sw[a]);
        res->sceneMax[a] = ord_dec(sw[3 + a]);
    }
    res->boxesMs = ev.ms(0, 1);
    res->sortMs = ev.ms(1, 2);
    res->clustersMs = ev.ms(2, 3);
    res->roundsMs = ev.ms(3, 4);
    res->tailMs = ev.ms(4, 5);
    res->seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - wall0).count();
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_instance_invert(const float objectToWorld[12], float worldToObject[12])
{
    const char* fn = "ntr_instance_invert";
    if (!objectToWorld || !worldToObject) return set_error(NTR_ERR_INVALID, "%s: null", fn);
    // binary64, every product rounded before the sum that uses it (the library is compiled without contraction); np_instanced.invert
    if (!instance_invert(objectToWorld, worldToObject))
        return set_error(NTR_ERR_INVALID, "%s: the transform's determinant is zero or not finite", fn);
    return NTR_OK;
}

int ntr_tlas_capacity(int32_t numInstances, int64_t* nodesBytes, int64_t* recordsBytes)
{
    if (numInstances < 1) return set_error(NTR_ERR_INVALID, "ntr_tlas_capacity: numInstances < 1");
    if (nodesBytes) *nodesBytes = std::max<int64_t>((int64_t)numInstances - 1, 1) * kNodeBytes;
    if (recordsBytes) *recordsBytes = (int64_t)numInstances * kRecordBytes;
    return NTR_OK;
}

int ntr_tlas_build(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                   const void* d_poolNodes, int64_t poolNodesBytes, int32_t radius, void* d_tlasNodes, int64_t tlasNodesCapacity,
                   void* d_records, int64_t recordsCapacity, NtrTlasResult* result, void* stream)
{
    const char* fn = "ntr_tlas_build";
    if (!result) return set_error(NTR_ERR_INVALID, "%s: null result", fn);
    memset(result, 0, sizeof(*result));
    if (numInstances < 1 || (int64_t)numInstances - 1 > kMaxNodes || numBlas < 1 || !d_instances || !blasRanges || !d_poolNodes ||
        !d_tlasNodes || !d_records)
        return set_error(NTR_ERR_INVALID, "%s: bad arguments (1 <= numInstances <= %lld, numBlas >= 1, non-null buffers)", fn,
                         (long long)kMaxNodes + 1);
    if (radius < 1 || radius > kPlocMaxRadius) return set_error(NTR_ERR_INVALID, "%s: radius %d outside 1..%d", fn, (int)radius, kPlocMaxRadius);
    int64_t needN, needR;
    ntr_tlas_capacity(numInstances, &needN, &needR);
    if (tlasNodesCapacity < needN || recordsCapacity < needR)
        return set_error(NTR_ERR_INVALID, "%s: output buffers smaller than ntr_tlas_capacity()", fn);
    if (((uintptr_t)d_poolNodes | (uintptr_t)d_records | (uintptr_t)d_tlasNodes) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: the buffers must be 16-byte aligned", fn);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    for (int k = 0; k < numBlas; k++)
        if (const int rc = check_blas_range(fn, k, blasRanges[k], poolNodesBytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return finish_build(tl_build(numInstances, d_instances, numBlas, blasRanges, d_poolNodes, radius, d_tlasNodes, d_records, result, s),
                        result, s);
}

int ntr_tlas_scratch_bytes(int64_t* bytes) { return pool_bytes("ntr_tlas_scratch_bytes", g_tlPool, bytes); }

}  // extern "C"
