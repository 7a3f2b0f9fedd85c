// ntr_internal.h -- helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "ntrace_amd.h"

namespace ntr {
constexpr int kMaxDevices = 64;   // device indices the per-device state of the library covers

int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char* what);

// Tunables (environment overrides for sweeps), read once at first use -- see ntr_api.cpp.
struct Tunables {
    int chunk, fetchThreshold, leafSwitchBelow, blocksPerCU, blocksPerCUIncoherent, blocksPerCUDivergent, poolHeads, octant, unified, flatFetch, uniformPrologue, certainSteps, certainDescent, splitSlice, wholeWave, prefetchAfter, minipool, minipoolThreshold, minipoolWide;
    int autoHint, autoHintMinRays, persistentHints, route, predict, predictPersistent, predictDepth, predictMinRays, predictMinNodes;
    int schedRefreshEvery, schedClasses;
    int lbvhSplit, lbvhAggLds, lbvhAggStaged, lbvhSortItems;
};
Tunables tunables();

// true when `s` is being captured into a HIP graph: scratch handed to such a launch must stay valid for the
// lifetime of the graph, so it is taken from never-recycled storage.
bool stream_is_capturing(hipStream_t s);

// lbvh_kernels.hip: Morton codes and their stable sort exactly as ntr_lbvh_build makes them (the HLBVH builder's first phase)
size_t lbvh_sort_scratch_bytes(int n);
int lbvh_sort_codes(int n, const int32_t* d_tri, const float* d_pos, const float sceneMin[3], const float sceneMax[3], void* scratch,
                    hipStream_t s, const unsigned int** keys, const int** idx, const unsigned int** errWord);

// selftest_prims_kernels.hip: the device self tests of radix_sort.h and device_prims.h; their arguments are checked in ntr_api.cpp
constexpr int kSelftestMaxPasses = 16;   // passes of one ntr_selftest_onesweep call
constexpr int kSelftestMaxPassNumber = 125;   // OS_MAX_PASSES - 1 (radix_sort.h; asserted where both are seen)
bool selftest_onesweep_offered(int items, int mode, int skipTrivial);
int selftest_onesweep_run(int items, int mode, int skipTrivial, int n, const uint32_t* d_keys, int stride, const int32_t* d_vals, int numPasses,
                          const int32_t* passes, int forceTicket, uint32_t* d_keysOut, int32_t* d_valsOut, uint32_t* errWord, hipStream_t s);
int selftest_scan_run(int type, int threads, int n, const void* d_in, void* d_prefix, void* total, hipStream_t s);
int selftest_block_sums_run(int type, int threads, int nb, const void* d_in, void* d_out, void* total, hipStream_t s);
int selftest_float_order_run(int n, const uint32_t* d_words, uint32_t* d_single, uint32_t* d_pairs, hipStream_t s);
int selftest_box_words_run(int m, const float* d_boxes, const int32_t* d_group, int groups, float eps, const uint32_t* d_lane32,
                           const uint64_t* d_lane64, uint32_t* d_groupsOut, uint32_t* d_foldsOut, hipStream_t s);
}  // namespace ntr

// sched_state.cpp: (re)build the top-of-tree box table cached for this node buffer (dispatch-order prediction)
extern "C" int ntr_top_table_refresh(const void* d_nodes, int64_t nodesBytes, void* stream);

#define NTR_HIP(call)                                            \
    do {                                                         \
        hipError_t _e = (call);                                  \
        if (_e != hipSuccess) return ::ntr::hip_fail(_e, #call); \
    } while (0)
