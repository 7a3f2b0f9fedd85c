// trace_instanced_kernels.hip -- the two-level trace for gfx950 (ntr_trace_instanced): a top-level tree over instances, each a Compact
// tree of a pool plus a transform (instanced_bvh.h).  EXTENSION: the reference has no instancing; the rule is the numpy spec
// tests/np_instanced.py, which the kernel equals in all four result words and the instance id.
// One kernel, 64-thread workgroups, one ray per lane: a unified-step loop built from trace_lane.h.  Per iteration every live lane fetches
// the 64 bytes it needs -- a top-level node, an instance record, a BLAS node at nodesOffset + node, or a triangle and the word after it
// at row offset + row -- and takes the step they allow:
//   inner node (either level)   inner_advance<false, 8>, unchanged
//   triangle                    triangle_step, through unified_advance, unchanged
//   entering an instance        (top level, link ~i) push the exit marker, transform the ray by record i, go on at the BLAS's node 0
//   leaving an instance         (the exit marker was popped) reload the world ray from d_rays -- one 32-byte load, rare against the
//                               steps, for six registers less -- and pop again
// Arithmetic is the GENERIC path only: a transformed ray need not lie in the FAST ranges, and the pool has no validate flags.
// Fetches go through four wave-uniform range-checked descriptors (fetch64_four_buffers: the shape of fetch64_two_buffers): whatever a
// link or an offset holds, a lane reads zeros and never faults.  Per lane beyond the single-level loop: nodesOffset, the row offset
// and the instance index, which also says which level the lane is on (-1: the top level).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
#include "trace_lane.h"

namespace ntr {
namespace {

struct InstancedParams {
    int32_t numRays, anyHit;
    const NtrRay* rays;
    NtrRayResult* results;
    int32_t* instanceIDs;
    const void *tlas, *records, *poolNodes, *poolWoop;
    uint32_t tlasBytes, recordsBytes, poolNodesBytes, poolWoopBytes;   // descriptor ranges (out-of-range loads return 0)
    const int32_t* triIndex;
    int32_t rootLink, numInstances;
    unsigned int* status;   // sticky error bits
};

// Lanes of mask k fetch 64 B at byte offset `ofs` of buffer k (range-checked: beyond the extent a load returns 0 and touches no memory),
// all into the same registers; a buffer whose mask is empty is skipped by a scalar branch; the other lanes keep what a..d held.
#define NTR_FETCH64_GROUP(R, M, L)                                          \
    "s_and_b64 exec, %[sav], %[" M "]\n\t"                                  \
    "s_cbranch_execz .Lcs_fetch" L "%=\n\t"                                 \
    "buffer_load_dwordx4 %[a], %[ofs], %[" R "], 0 offen\n\t"               \
    "buffer_load_dwordx4 %[b], %[ofs], %[" R "], 0 offen offset:16\n\t"     \
    "buffer_load_dwordx4 %[c], %[ofs], %[" R "], 0 offen offset:32\n\t"     \
    "buffer_load_dwordx4 %[d], %[ofs], %[" R "], 0 offen offset:48\n\t"     \
    ".Lcs_fetch" L "%=:\n\t"
__device__ __forceinline__ void fetch64_four_buffers(u32x4 r0, u32x4 r1, u32x4 r2, u32x4 r3, int ofs, unsigned long long m0,
                                                     unsigned long long m1, unsigned long long m2, unsigned long long m3, float4& a, float4& b,
                                                     float4& c, float4& d)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 NTR_FETCH64_GROUP("r0", "m0", "a")
                 NTR_FETCH64_GROUP("r1", "m1", "b")
                 NTR_FETCH64_GROUP("r2", "m2", "c")
                 NTR_FETCH64_GROUP("r3", "m3", "d")
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [r0] "s"(r0), [r1] "s"(r1), [r2] "s"(r2), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd);
}
#undef NTR_FETCH64_GROUP

__global__ __launch_bounds__(64) void trace_instanced(InstancedParams p)
{
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;
    const float4* rays4 = reinterpret_cast<const float4*>(p.rays);
    const u32x4 rTlas = rsrc_words(p.tlas, p.tlasBytes), rRec = rsrc_words(p.records, p.recordsBytes),
                rNodes = rsrc_words(p.poolNodes, p.poolNodesBytes), rWoop = rsrc_words(p.poolWoop, p.poolWoopBytes);
    const bool anyHit = p.anyHit != 0;

    RayRegs r;   // the current form: the world ray on the top level, the object ray inside an instance
    {
        const float4 o = rays4[(valid ? rayIdx : 0) * 2 + 0], d = rays4[(valid ? rayIdx : 0) * 2 + 1];
        r.ox = o.x; r.oy = o.y; r.oz = o.z; r.tmin = o.w;
        r.dx = d.x; r.dy = d.y; r.dz = d.z; r.tmax = d.w;
        r.rx = r.ry = r.rz = 0.0f;   // (the FAST path's reciprocals: unused)
    }
    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[0][lane];
    stack_reset(st);

    int hitAddr = -1, hitInst = -1;   // the hit's row in the pool's triWoop and its instance
    float hitU = 0.0f, hitV = 0.0f;
    int inst = -1;                    // >= 0: inside that instance
    unsigned int nodesOffset = 0u, rowOffset = 0u;
    // a degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal
    int node = (valid && r.tmin < r.tmax) ? p.rootLink : kSentinel;

    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a;
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
        const bool top = inst < 0;
        const bool inner = (unsigned)node < (unsigned)kSentinel;
        const bool neg = node < 0;
        int ofs = kNoNode;
        if (top) {
            if (inner) ofs = node;
            else if (neg && (unsigned)~node < (unsigned)p.numInstances) ofs = ~node * kRecordBytes;
        } else if (inner) {
            const unsigned int o = nodesOffset + (unsigned)node;
            if (o >= nodesOffset) ofs = (int)o;                       // (a sum that wraps reads nothing)
        } else if (neg) {
            const unsigned int row = rowOffset + (unsigned)~node;
            if (row < (unsigned)(kPoolMaxBytes >> kRowShift)) ofs = (int)(row << kRowShift);
        }
        fetch64_four_buffers(rTlas, rRec, rNodes, rWoop, ofs, __ballot(top && inner), __ballot(top && neg), __ballot(!top && inner),
                             __ballot(!top && neg), a, b, c, d);
        if (node == kSentinel) {
            // done: waits for the wave
        } else if (!inner && !neg) {
            // a positive word above the sentinel: the exit marker.  Leaving: the world ray again (tmin and the shrunk tmax stay)
            if (node == kExitMarker) {
                const float4 o = rays4[rayIdx * 2 + 0], dd = rays4[rayIdx * 2 + 1];
                r.ox = o.x; r.oy = o.y; r.oz = o.z;
                r.dx = dd.x; r.dy = dd.y; r.dz = dd.z;
                inst = -1;
            }
            node = stack_pop(st, spill);   // (any other such word is no link: it is dropped)
        } else if (top && inner) {
            inner_advance<false, 8>(a, b, c, d, r, node, st, spill, p.status);
        } else if (top) {
            // entering instance ~node: its record is worldToObject (a, b, c) and nodesOffset, row offset, nodesBytes (d)
            const int idx = ~node;
            if ((unsigned)idx >= (unsigned)p.numInstances) {
                node = stack_pop(st, spill);
            } else if (st.sp >= LDS_DEPTH + SPILL_DEPTH) {
                atomicOr(p.status, NTR_STATUS_STACK_OVERFLOW);   // no room for the marker: the instance is not entered
                node = stack_pop(st, spill);
            } else {
                stack_push(st, spill, kExitMarker, p.status);
                const float ox = dot4(a, r.ox, r.oy, r.oz, 1.0f), oy = dot4(b, r.ox, r.oy, r.oz, 1.0f), oz = dot4(c, r.ox, r.oy, r.oz, 1.0f);
                const float dx = dot4(a, r.dx, r.dy, r.dz, 0.0f), dy = dot4(b, r.dx, r.dy, r.dz, 0.0f), dz = dot4(c, r.dx, r.dy, r.dz, 0.0f);
                r.ox = ox; r.oy = oy; r.oz = oz;
                r.dx = dx; r.dy = dy; r.dz = dz;
                nodesOffset = __float_as_uint(d.x);
                rowOffset = __float_as_uint(d.y);
                inst = idx;
                node = 0;
            }
        } else {
            int row = -1;   // the BLAS's own row of a hit this step accepts
            unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
            if (row >= 0) {
                hitAddr = (int)(rowOffset + (unsigned)row);
                hitInst = inst;
            }
        }
    }
    if (!valid) return;
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    p.instanceIDs[rayIdx] = hitInst;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                   const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                   int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                   int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, float* seconds, void* stream)
{
    const char* fn = "ntr_trace_instanced";
    if (seconds) *seconds = 0.0f;
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_results || !d_instanceIDs) return set_error(NTR_ERR_INVALID, "%s: null ray, result or instance id buffer", fn);
    if (numInstances < 1 || (int64_t)numInstances * kRecordBytes > kPoolMaxBytes || !d_records || !d_poolNodes || !d_poolTriWoop || !d_poolTriIndex)
        return set_error(NTR_ERR_INVALID, "%s: no instances or no pool", fn);
    if (!(rootLink == 0 || (rootLink < 0 && (int64_t)~rootLink < numInstances)))
        return set_error(NTR_ERR_INVALID, "%s: rootLink %d is neither 0 nor an instance's link", fn, (int)rootLink);
    if (tlasNodesBytes < 0 || (tlasNodesBytes % kNodeBytes) != 0 || tlasNodesBytes > kMaxNodesBytes || (rootLink == 0 && (!d_tlasNodes || tlasNodesBytes < kNodeBytes)))
        return set_error(NTR_ERR_INVALID, "%s: the top-level node buffer must be a multiple of 64 bytes, at most 0x%llx, and hold the root", fn,
                         (unsigned long long)kMaxNodesBytes);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;

    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    InstancedParams p{};
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results; p.instanceIDs = d_instanceIDs;
    p.tlas = d_tlasNodes; p.records = d_records; p.poolNodes = d_poolNodes; p.poolWoop = d_poolTriWoop;
    p.tlasBytes = d_tlasNodes ? (uint32_t)tlasNodesBytes : 0u; p.recordsBytes = (uint32_t)((int64_t)numInstances * kRecordBytes);
    p.poolNodesBytes = (uint32_t)poolNodesBytes; p.poolWoopBytes = (uint32_t)poolTriWoopBytes;
    p.triIndex = d_poolTriIndex; p.rootLink = rootLink; p.numInstances = numInstances; p.status = ds->status;

    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    trace_instanced<<<(numRays + 63) / 64, 64, 0, s>>>(p);
    NTR_HIP(hipGetLastError());
    if (seconds) {
        NTR_HIP(ev.record(1));
        float ms = 0.0f;
        NTR_HIP(ev.elapsed(0, 1, &ms));
        *seconds = ms * 1e-3f;
        unsigned int bits = 0;
        if (const int rc = status_fetch(ds, s, &bits)) return rc;
        if (bits & NTR_STATUS_STACK_OVERFLOW) return set_error(NTR_ERR_OVERFLOW, "%s: traversal stack overflow", fn);
    }
    return NTR_OK;
}
