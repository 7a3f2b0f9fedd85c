// selftest_prims_kernels.hip -- device self tests of the shared device toolkit, run on inputs the caller chooses: the one-sweep radix pass
// (radix_sort.h) in exactly the instantiations its five users launch, the three-launch scan and scan_block_sums, the order-preserving
// float encoding with ord_min / ord_max, the six-word box merged by integer max, the wave folds and wave_grouped_atomic (device_prims.h).
// The production templates run as they stand; the kernels here only feed them and store what they return.
// ntr_selftest_onesweep / ntr_selftest_scan / ntr_selftest_scan_block_sums / ntr_selftest_float_order / ntr_selftest_box_words in the C-ABI
// (argument checks: ntr_api.cpp; tests/test_device_prims_gpu.py against the numpy references of tests/np_device_prims.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_prims.h"
#include "device_scratch.h"
#include "ntr_internal.h"
#include "radix_sort.h"

namespace ntr {

static_assert(kSelftestMaxPassNumber == OS_MAX_PASSES - 1, "ntr_api.cpp refuses the pass numbers the tile state's status bits cannot hold");

struct SelftestPasses {
    int count;
    int shift[kSelftestMaxPasses], pass[kSelftestMaxPasses];
};

// The digit histograms of every pass of the list in one read of the keys, as the users' key kernels take them.  FETCH: the key word of
// element i is keys[vals[i] * stride] (MODE 2); a value outside [0, n) is not followed and raises bit 1 of *err.
template <bool FETCH>
__global__ __launch_bounds__(256) void selftest_digit_hist_kernel(int n, const unsigned int* __restrict__ keys, const int* __restrict__ vals, int stride,
                                                                  SelftestPasses passes, unsigned int* __restrict__ hist, unsigned int* __restrict__ err)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned int k;
    if (FETCH) {
        const int v = vals[i];
        if (v < 0 || v >= n) { atomicOr(err, 1u); return; }
        k = keys[(size_t)v * stride];
    } else
        k = keys[i];
    for (int p = 0; p < passes.count; p++) atomicAdd(&hist[p * 256 + ((k >> passes.shift[p]) & 255)], 1u);
}

// ---- scan -------------------------------------------------------------------------------------------------------------------------
template <int THREADS, class V>
__global__ __launch_bounds__(THREADS) void selftest_scan_local_kernel(int n, const V* __restrict__ in, V* __restrict__ local, V* __restrict__ blockSums)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const bool valid = i < (size_t)n;
    scan_local_store<THREADS>(valid ? in[i] : V{}, valid, i, local, blockSums, (int)blockIdx.x);
}
template <int THREADS, class V>
__global__ __launch_bounds__(THREADS) void selftest_scan_add_kernel(int n, V* __restrict__ local, const V* __restrict__ blockEx)
{
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < (size_t)n) local[i] = blockEx[blockIdx.x] + local[i];
}

// ---- float order ------------------------------------------------------------------------------------------------------------------
// single[i][6]: ord_enc, ord_dec(ord_enc), ord_enc_int, ord_dec_int(ord_enc_int), ord_to_int(ord_enc), ord_from_int(ord_to_int(ord_enc));
// pairs[i * n + j][2]: ord_min(w[i], w[j]), ord_max(w[i], w[j]) -- every ordered pair, so both orders of the operands
__global__ __launch_bounds__(256) void selftest_float_order_kernel(int n, const unsigned int* __restrict__ words, unsigned int* __restrict__ single,
                                                                   unsigned int* __restrict__ pairs)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < (size_t)n) {
        const float f = __uint_as_float(words[idx]);
        const unsigned int e = ord_enc(f);
        const int ei = ord_enc_int(f);
        unsigned int* o = single + idx * 6;
        o[0] = e;
        o[1] = __float_as_uint(ord_dec(e));
        o[2] = (unsigned int)ei;
        o[3] = __float_as_uint(ord_dec_int(ei));
        o[4] = (unsigned int)ord_to_int(e);
        o[5] = ord_from_int(ord_to_int(e));
    }
    if (idx < (size_t)n * n) {
        const float a = __uint_as_float(words[idx / n]), b = __uint_as_float(words[idx % n]);
        pairs[idx * 2] = __float_as_uint(ord_min(a, b));
        pairs[idx * 2 + 1] = __float_as_uint(ord_max(a, b));
    }
}

// ---- boxes and wave folds ---------------------------------------------------------------------------------------------------------
constexpr int kBoxOutWords = 26;   // per merge path and group: words [0..5], members [6], corners as merged [7..12], grown [13..18], of no members [19..24], area [25]

// Lane i merges box i into group group[i] (-1: none), once by atomic_max_box and once word by word through wave_grouped_atomic, as the
// sweep builder's child boxes are merged; and folds its lane words.  m is a multiple of 64: every wave is full.  A group outside
// [-1, groups) is not followed and raises bit 1 of *err.
__global__ __launch_bounds__(256) void selftest_box_merge_kernel(int m, const float* __restrict__ boxes, const int* __restrict__ group, int groups,
                                                                 const unsigned int* __restrict__ lane32, const unsigned long long* __restrict__ lane64,
                                                                 unsigned int* plainWords, unsigned int* groupedWords, unsigned int* members,
                                                                 unsigned int* __restrict__ folds, unsigned int* err)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < m;
    int g = live ? group[i] : -1;
    if (g < -1 || g >= groups) { atomicOr(err, 1u); g = -1; }
    float4 lo = {0.0f, 0.0f, 0.0f, 0.0f}, hi = lo;
    if (live) {
        const float* b = boxes + (size_t)i * 6;
        lo.x = b[0]; lo.y = b[1]; lo.z = b[2];
        hi.x = b[3]; hi.y = b[4]; hi.z = b[5];
    }
    unsigned int w[6];
    box_words(lo, hi, w);
    if (g >= 0) {
        atomic_max_box(plainWords + (size_t)g * 6, w);
        atomicAdd(&members[g], 1u);
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
        wave_grouped_atomic(g, w[k], wave_max_u32, [&](int c, unsigned int v) { atomicMax(&groupedWords[(size_t)c * 6 + k], v); });
    if (!live) return;   // (whole waves: m is a multiple of 64)
    const unsigned int a = lane32[i];
    const unsigned long long q = wave_min_u64(lane64[i]);
    unsigned int* o = folds + (size_t)i * 6;
    o[0] = wave_min_u32(a);
    o[1] = wave_max_u32(a);
    o[2] = wave_sum_u32(a);
    o[3] = wave_or_u32(a);
    o[4] = (unsigned int)q;
    o[5] = (unsigned int)(q >> 32);
}

__global__ __launch_bounds__(256) void selftest_box_decode_kernel(int groups, float eps, const unsigned int* __restrict__ plainWords,
                                                                  const unsigned int* __restrict__ groupedWords, const unsigned int* __restrict__ members,
                                                                  unsigned int* __restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * groups) return;
    const int g = t % groups;
    const unsigned int* w = (t < groups ? plainWords : groupedWords) + (size_t)g * 6;
    unsigned int* o = out + (size_t)t * kBoxOutWords;
    const int count = (int)members[g];
    float lo[3], hi[3];
    for (int k = 0; k < 6; k++) o[k] = w[k];
    o[6] = members[g];
    words_box(count, w, eps, false, lo, hi);
    for (int k = 0; k < 3; k++) { o[7 + k] = __float_as_uint(lo[k]); o[10 + k] = __float_as_uint(hi[k]); }
    words_box(count, w, eps, true, lo, hi);
    for (int k = 0; k < 3; k++) { o[13 + k] = __float_as_uint(lo[k]); o[16 + k] = __float_as_uint(hi[k]); }
    words_box(0, w, eps, true, lo, hi);
    for (int k = 0; k < 3; k++) { o[19 + k] = __float_as_uint(lo[k]); o[22 + k] = __float_as_uint(hi[k]); }
    o[25] = __float_as_uint(words_area(w));
}

}  // namespace ntr

using namespace ntr;

namespace {
// Grow-only scratch of the self tests (device_scratch.h): every sort runs on the same tile-state words, cleared afresh per call.
ntr::DeviceScratchPool g_selftestScratch;

// One pass of one production instantiation.  Unforced, onesweep_launch decides between the ticket and the resident path as it does for
// its users; forced, the kernel gets the ticket whatever the grid size.  (The ticket is never withheld from a grid that may not fit.)
template <int ITEMS, int MODE, bool SKIP>
void os_pass(hipStream_t s, bool forceTicket, int tiles, int n, const unsigned int* kIn, const int* vIn, unsigned int* kOut, int* vOut, int stride,
             int shift, int pass, const unsigned int* hist, unsigned long long* state, unsigned int* ticket, unsigned int* err)
{
    if (forceTicket)
        hipLaunchKernelGGL((onesweep_pass_kernel<ITEMS, MODE, SKIP>), dim3(tiles), dim3(OS_THREADS), 0, s, n, kIn, vIn, kOut, vOut, stride, shift, pass,
                           hist, state, ticket, err);
    else
        onesweep_launch<ITEMS, MODE, SKIP>(s, tiles, n, kIn, vIn, kOut, vOut, stride, shift, pass, hist, state, ticket, err);
}

// MODE 2: the first pass fetches the key word through the values, the others run in MODE 0 on the dense pairs, as both users chain them.
template <int ITEMS, int MODE, bool SKIP>
int os_sort(hipStream_t s, int n, const unsigned int* d_keys, int stride, const int* d_vals, const SelftestPasses& pl, bool forceTicket,
            unsigned int* d_keysOut, int* d_valsOut, uint32_t* errWord)
{
    constexpr int TILE = OS_THREADS * ITEMS;
    const int tiles = (n + TILE - 1) / TILE;
    const size_t histWords = (size_t)kSelftestMaxPasses * 256, miscWords = 32, stateWords = (size_t)tiles * 256 * 2;
    ScratchCarver cv;
    const size_t oZero = cv.take((histWords + miscWords + stateWords) * 4);
    const size_t oKA = cv.take((size_t)n * 4), oKB = cv.take((size_t)n * 4), oVA = cv.take((size_t)n * 4), oVB = cv.take((size_t)n * 4);
    void* base = nullptr;
    if (const int rc = g_selftestScratch.reserve(cv.off, &base)) return rc;
    char* ws = (char*)base;
    unsigned int* hist = (unsigned int*)(ws + oZero);
    unsigned int* misc = hist + histWords;   // [0 .. kSelftestMaxPasses) tickets, [31] the error word
    unsigned long long* state = (unsigned long long*)(misc + miscWords);
    unsigned int* kBuf[2] = {(unsigned int*)(ws + oKA), (unsigned int*)(ws + oKB)};
    int* vBuf[2] = {(int*)(ws + oVA), (int*)(ws + oVB)};
    NTR_HIP(hipMemsetAsync(ws + oZero, 0, (histWords + miscWords + stateWords) * 4, s));
    if (MODE == 2)
        hipLaunchKernelGGL(selftest_digit_hist_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, n, d_keys, d_vals, stride, pl, hist, misc + 31);
    else
        hipLaunchKernelGGL(selftest_digit_hist_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, n, d_keys, d_vals, stride, pl, hist, misc + 31);
    NTR_HIP(hipGetLastError());
    unsigned int e = 0;
    if (MODE == 2) {   // no pass follows a value the histogram kernel refused
        NTR_HIP(hipMemcpyAsync(&e, misc + 31, sizeof(e), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        if (e) return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: a value outside [0, n)");
    }
    const unsigned int* kIn = d_keys;
    const int* vIn = d_vals;
    for (int p = 0; p < pl.count; p++) {
        unsigned int* kOut = kBuf[p & 1];
        int* vOut = vBuf[p & 1];
        if (p == 0)
            os_pass<ITEMS, MODE, SKIP>(s, forceTicket, tiles, n, kIn, vIn, kOut, vOut, stride, pl.shift[p], pl.pass[p], hist + p * 256, state, misc + p, misc + 31);
        else
            os_pass<ITEMS, 0, SKIP>(s, forceTicket, tiles, n, kIn, vIn, kOut, vOut, 1, pl.shift[p], pl.pass[p], hist + p * 256, state, misc + p, misc + 31);
        kIn = kOut;
        vIn = vOut;
    }
    NTR_HIP(hipGetLastError());
    NTR_HIP(hipMemcpyAsync(d_keysOut, kIn, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    NTR_HIP(hipMemcpyAsync(d_valsOut, vIn, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    NTR_HIP(hipMemcpyAsync(&e, misc + 31, sizeof(e), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    *errWord = e;
    return NTR_OK;
}

template <int THREADS, class V>
int scan_run(hipStream_t s, int n, const V* d_in, V* d_prefix, void* total)
{
    const int nb = (n + THREADS - 1) / THREADS;
    V* d_blocks = nullptr;   // [nb] block sums, then the total
    if (const int rc = device_malloc((void**)&d_blocks, ((size_t)nb + 1) * sizeof(V), "ntr_selftest_scan")) return rc;
    hipLaunchKernelGGL((selftest_scan_local_kernel<THREADS, V>), dim3(nb), dim3(THREADS), 0, s, n, d_in, d_prefix, d_blocks);
    hipLaunchKernelGGL((scan_block_sums<THREADS, V>), dim3(1), dim3(THREADS), 0, s, nb, (const V*)d_blocks, d_blocks, d_blocks + nb);
    hipLaunchKernelGGL((selftest_scan_add_kernel<THREADS, V>), dim3(nb), dim3(THREADS), 0, s, n, d_prefix, (const V*)d_blocks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(total, d_blocks + nb, sizeof(V), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_blocks);
    if (e != hipSuccess) return hip_fail(e, "ntr_selftest_scan");
    return NTR_OK;
}

template <int THREADS, class V>
int block_sums_run(hipStream_t s, int nb, const V* d_in, V* d_out, void* total)
{
    V* d_total = nullptr;
    if (total)
        if (const int rc = device_malloc((void**)&d_total, sizeof(V), "ntr_selftest_scan_block_sums")) return rc;
    hipLaunchKernelGGL((scan_block_sums<THREADS, V>), dim3(1), dim3(THREADS), 0, s, nb, d_in, d_out, d_total);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && total) e = hipMemcpyAsync(total, d_total, sizeof(V), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (d_total) (void)hipFree(d_total);
    if (e != hipSuccess) return hip_fail(e, "ntr_selftest_scan_block_sums");
    return NTR_OK;
}

template <class V>
int scan_by_threads(hipStream_t s, int threads, int n, const void* d_in, void* d_prefix, void* total)
{
    return threads == 256 ? scan_run<256, V>(s, n, (const V*)d_in, (V*)d_prefix, total) : scan_run<1024, V>(s, n, (const V*)d_in, (V*)d_prefix, total);
}
template <class V>
int block_sums_by_threads(hipStream_t s, int threads, int nb, const void* d_in, void* d_out, void* total)
{
    return threads == 256 ? block_sums_run<256, V>(s, nb, (const V*)d_in, (V*)d_out, total) : block_sums_run<1024, V>(s, nb, (const V*)d_in, (V*)d_out, total);
}
}  // namespace

namespace ntr {

// The instantiations the users launch (OS_LOOK is 1 at every call site; MODE 1 has no caller):
//   <8 | 16 | 24 | 32, 0, false>  lbvh_kernels.hip (8: also sah_build_, tlas_build_, bvh_ploc_batch_kernels.hip)
//   <8, 2, false>                 bvh_ploc_batch_kernels.hip, followed by <8, 0, false>
//   <8, 2, true>, <8, 0, true>    rayops_kernels.hip
bool selftest_onesweep_offered(int items, int mode, int skipTrivial)
{
    if (skipTrivial != 0 && skipTrivial != 1) return false;
    if (mode == 0) return skipTrivial ? items == 8 : (items == 8 || items == 16 || items == 24 || items == 32);
    return mode == 2 && items == 8;
}

int selftest_onesweep_run(int items, int mode, int skipTrivial, int n, const uint32_t* d_keys, int stride, const int32_t* d_vals, int numPasses,
                          const int32_t* passes, int forceTicket, uint32_t* d_keysOut, int32_t* d_valsOut, uint32_t* errWord, hipStream_t s)
{
    SelftestPasses pl;
    pl.count = numPasses;
    for (int p = 0; p < kSelftestMaxPasses; p++) {
        pl.shift[p] = p < numPasses ? passes[2 * p] : 0;
        pl.pass[p] = p < numPasses ? passes[2 * p + 1] : 0;
    }
    const bool ft = forceTicket != 0;
#define NTR_ST_SORT(I, M, S) return os_sort<I, M, S>(s, n, d_keys, stride, d_vals, pl, ft, d_keysOut, d_valsOut, errWord)
    if (mode == 2) {
        if (skipTrivial) NTR_ST_SORT(8, 2, true);
        NTR_ST_SORT(8, 2, false);
    }
    if (skipTrivial) NTR_ST_SORT(8, 0, true);
    if (items == 32) NTR_ST_SORT(32, 0, false);
    if (items == 24) NTR_ST_SORT(24, 0, false);
    if (items == 16) NTR_ST_SORT(16, 0, false);
    NTR_ST_SORT(8, 0, false);
#undef NTR_ST_SORT
}

int selftest_scan_run(int type, int threads, int n, const void* d_in, void* d_prefix, void* total, hipStream_t s)
{
    switch (type) {
    case NTR_SCAN_U32: return scan_by_threads<unsigned int>(s, threads, n, d_in, d_prefix, total);
    case NTR_SCAN_I32: return scan_by_threads<int>(s, threads, n, d_in, d_prefix, total);
    case NTR_SCAN_U64: return scan_by_threads<unsigned long long>(s, threads, n, d_in, d_prefix, total);
    default: return scan_by_threads<U4>(s, threads, n, d_in, d_prefix, total);
    }
}

int selftest_block_sums_run(int type, int threads, int nb, const void* d_in, void* d_out, void* total, hipStream_t s)
{
    switch (type) {
    case NTR_SCAN_U32: return block_sums_by_threads<unsigned int>(s, threads, nb, d_in, d_out, total);
    case NTR_SCAN_I32: return block_sums_by_threads<int>(s, threads, nb, d_in, d_out, total);
    case NTR_SCAN_U64: return block_sums_by_threads<unsigned long long>(s, threads, nb, d_in, d_out, total);
    default: return block_sums_by_threads<U4>(s, threads, nb, d_in, d_out, total);
    }
}

int selftest_float_order_run(int n, const uint32_t* d_words, uint32_t* d_single, uint32_t* d_pairs, hipStream_t s)
{
    const size_t items = (size_t)n * n;
    hipLaunchKernelGGL(selftest_float_order_kernel, dim3((unsigned int)((items + 255) / 256)), dim3(256), 0, s, n, d_words, d_single, d_pairs);
    NTR_HIP(hipGetLastError());
    NTR_HIP(hipStreamSynchronize(s));
    return NTR_OK;
}

int selftest_box_words_run(int m, const float* d_boxes, const int32_t* d_group, int groups, float eps, const uint32_t* d_lane32,
                           const uint64_t* d_lane64, uint32_t* d_groupsOut, uint32_t* d_foldsOut, hipStream_t s)
{
    // plain words, grouped words (6 per group each), members, the error word: all zero, the empty box
    const size_t words = (size_t)groups * 13 + 1;
    unsigned int* d_w = nullptr;
    if (const int rc = device_malloc((void**)&d_w, words * 4, "ntr_selftest_box_words")) return rc;
    unsigned int *plain = d_w, *grouped = d_w + (size_t)groups * 6, *members = d_w + (size_t)groups * 12, *err = members + groups;
    hipError_t e = hipMemsetAsync(d_w, 0, words * 4, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(selftest_box_merge_kernel, dim3((m + 255) / 256), dim3(256), 0, s, m, d_boxes, d_group, groups, d_lane32,
                           (const unsigned long long*)d_lane64, plain, grouped, members, d_foldsOut, err);
        hipLaunchKernelGGL(selftest_box_decode_kernel, dim3((2 * groups + 255) / 256), dim3(256), 0, s, groups, eps, (const unsigned int*)plain,
                           (const unsigned int*)grouped, (const unsigned int*)members, d_groupsOut);
        e = hipGetLastError();
    }
    unsigned int bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, err, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_w);
    if (e != hipSuccess) return hip_fail(e, "ntr_selftest_box_words");
    if (bad) return set_error(NTR_ERR_INVALID, "ntr_selftest_box_words: a group outside [-1, groups)");
    return NTR_OK;
}

}  // namespace ntr
