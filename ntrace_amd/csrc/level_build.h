// level_build.h -- what the level-synchronous device builders (bvh_build_, sah_build_, kdtree_build_kernels.hip) share of their level
// loop: per level each decides per task, scans the tasks (U4), emits nodes, links and child tasks, scans the references, partitions
// them stably into the other buffer, reads one 32-byte record back and books the level.  The kernels, their launches and their order
// stay in the builders' files; here is what those loops have in common, stated once:
//   device  the binned builders' 32 planes and the position of a plane
//   host    the per-level record (LevelTotals, read_totals); the bookkeeping (LevelState); typed scratch pointers (at); the BVH entry
//           points' result, failure path and scratch query
#pragma once
#include "compact_bvh.h"
#include "device_prims.h"
#include "device_scratch.h"

namespace ntr {

// ---- the binned builders' planes (SPLIT_TYPE 5, PLANE_COUNT 32) ---------------------------------------------------------------
constexpr int kPlanes = 32;
constexpr int kPlanesPerAxis = (kPlanes + 2) / 3;   // 11: x and y get 11 planes, z gets 10; plane k is plane k % 11 of axis k / 11
constexpr float kPlaneEps = 1e-8f;                  // rt_common.cuh:37
__host__ __device__ constexpr int planes_on_axis(int a) { return a < 2 ? kPlanesPerAxis : kPlanes - 2 * kPlanesPerAxis; }

namespace {   // one copy per translation unit
// rpos = (float)(1 + k) / (float)(planesPerAxis + 1) (rt_common.cu:1013), folded by the compiler with IEEE rounding
__constant__ float kRpos[kPlanesPerAxis] = {1.0f / 12.0f, 2.0f / 12.0f, 3.0f / 12.0f, 4.0f / 12.0f, 5.0f / 12.0f, 6.0f / 12.0f,
                                            7.0f / 12.0f, 8.0f / 12.0f, 9.0f / 12.0f, 10.0f / 12.0f, 11.0f / 12.0f};
}  // namespace
// findPlaneAABB (rt_common.cu:1007-1030): pos = mn + (mx - mn) * rpos, two roundings
__device__ __forceinline__ float plane_pos(float mn, float mx, int j) { return mn + (mx - mn) * kRpos[j]; }

// ---- host: the per-level read-back ----------------------------------------------------------------------------------------------
struct LevelTotals {    // the head of every builder's 32-byte record; each adds three words of its own
    U4 t;               // x: inner nodes of the level, y: rows (kd-tree: index entries) of its leaves; z, w: the builder's own
    unsigned int err;   // bit 0: vertex index out of range, bit 1: a partition rank outside its child, bit 2: an output row or node
                        // beyond the caller's capacity (neither of the last two is expected)
};
template <class Totals>
inline int read_totals(Totals* host, const Totals* dev, hipStream_t s)   // all that was queued on s before has completed on return
{
    static_assert(sizeof(Totals) == 32, "one 32-byte record per level");
    NTR_HIP(hipMemcpyAsync(host, dev, sizeof(Totals), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    return NTR_OK;
}

// ---- host: the level loop's bookkeeping -------------------------------------------------------------------------------------------
struct LevelState {
    int64_t T = 1, innerBase = 0, rowBase = 0;   // tasks of this level; inner nodes and leaf rows (kd-tree: index entries) before it
    int level = 0, cur = 0;                      // after the loop `level` is the number of levels; cur: which double buffer is read
    int32_t numLeaves = 0, maxDepth = 0;
    int nxt() const { return cur ^ 1; }
    // Compact's bound on the nodes; checked before the error word: the emit kernels write no node beyond it and flag the level instead
    int check_nodes(const char* fn, int64_t inner) const
    {
        return innerBase + inner > kMaxNodes ? node_overflow_error(fn, level, innerBase + inner) : (int)NTR_OK;
    }
    void advance(int64_t inner, int64_t rows)   // the level made `inner` nodes and `rows` rows: on to the nodes' 2 * inner children
    {
        numLeaves += (int32_t)(T - inner);
        if (inner) maxDepth = level + 1;
        innerBase += inner;
        rowBase += rows;
        T = 2 * inner;
        cur = nxt();
        level++;
    }
};

// ---- host: scratch and entry points -----------------------------------------------------------------------------------------------
// The array at byte offset `off` of the scratch block.  `base` changes when a pool regrows: resolve after that, not before.
template <class T>
inline T* at(void* base, size_t off) { return (T*)((char*)base + off); }
// A build's first block: whatever an earlier build left in the pool is not carried over
inline int first_block(DeviceScratchPool& pool, size_t bytes, void** base)
{
    return pool.regrow(bytes, base, [](void*, void*) { return (int)NTR_OK; });
}

// A Compact-BVH build's counts and exact byte extents (NtrPersistentBvhResult, NtrSahDeviceResult)
template <class Result>
inline void fill_bvh_result(Result* res, const LevelState& lv)
{
    res->numNodes = (int32_t)lv.innerBase;
    res->numLeaves = lv.numLeaves;
    res->numLevels = lv.level;
    res->maxDepth = lv.maxDepth;
    res->nodesBytes = lv.innerBase * kNodeBytes;
    res->triWoopBytes = lv.rowBase * kRowBytes;
    res->triIndexBytes = lv.rowBase * 4;
}
template <class Result>
inline int finish_build(int rc, Result* res, hipStream_t s)   // a failed build leaves an idle stream and a zeroed result
{
    if (rc != NTR_OK) {
        (void)hipStreamSynchronize(s);
        *res = Result{};
    }
    return rc;
}
inline int pool_bytes(const char* fn, DeviceScratchPool& pool, int64_t* bytes)   // the *_scratch_bytes entry points
{
    if (!bytes) return set_error(NTR_ERR_INVALID, "%s: null", fn);
    *bytes = (int64_t)pool.held();
    return NTR_OK;
}

}  // namespace ntr
