// kdtree_kernels.hip -- CDNA4 (gfx950, wave64) kd-tree traversal kernel.
//
// Replaces the reference's `trace_kdtree` kernel (contract TRACE_FUNC_KDTREE, src/rt/kernels/CudaTracerKernels.hpp:81-97) as
// compiled by CudaKDTreeTracer: fermi_kdtree_while_while_leafRef.cu:244-624 with SHORTSTACK 0, neither SPECULATIVE nor
// BRANCHLESS.  One ray per lane, 64-thread workgroups.  Buffers: host/CudaKDTree.hpp.
//
// ARITHMETIC.  The kernel's own binary32 expressions in source order (no FMA contraction: -ffp-contract=off; true division):
//   setup   idir = 1 / (|d| > 2^-80 ? d : copysign(2^-80, d)); slab t = bmin * idir - o * idir;
//           tmin = max4(slab mins, ray.tmin) - 1e-4,  tmax = min4(slab maxes, ray.tmax) + 1e-4,  max4 / min4 = fmaxf / fminf
//           chains (CudaTracerKernels.hpp:235-243: NaN operands are ignored, unlike the BVH path's selects)
//   inner   t = (split - o[axis]) * idir[axis]; the near child is picked by the sign bit of idir[axis];
//           t > tmax: near only;  t < tmin: far only;  otherwise push (far, tmax), tmax = t, go near
//   pop     tmin = tmax, then (node, tmax) = pop
//   leaf    per reference: Oz = w - ox x - oy y - oz z, t = Oz * (1 / dot(d, row0));  t >= tmin - delta && t <= tmax + delta,
//           then u in [0, 1], then v >= 0 && u + v <= 1.  A hit sets tmax = t and the leaf's loop goes on (a later reference
//           can replace the hit by one up to delta farther); a ray stops after a leaf that produced a hit.
//   Hits are not clipped to [ray.tmin, ray.tmax] beyond these slack windows, and anyHit is ignored, as in the reference.
// RECORDS.  Hit: (triId, t, bits(u), bits(v)).  DEVIATION: a miss is the BVH path's miss record (-1, ray.tmax, 0, 0); the
// reference stores its working tmax there, a value no consumer reads (countHits, reconstruct and the AO generator test id).
// DEVIATION: the reference's stack bottom is an entry (EntrypointSentinel, -1); popping it ends traversal whenever the popped
// interval is empty (tmin > -1, the case of every ray with tmin >= 0) and otherwise fetches node 0x76543210.  Here popping the
// bottom always ends traversal (a miss).
// STACK.  (node, tmax) pairs; each push happens at a different level of the current path, so the depth is at most the tree's
// (spatial median <= 18, SAH 29 at 10 M triangles).  64 entries: the first NTR_KDTREE_LDS_DEPTH in LDS laid out [entry][lane]
// (a lane's 8-byte entries sit in consecutive banks of its own column: no conflicts), the rest in scratch.  A push beyond 64
// sets NTR_STATUS_STACK_OVERFLOW and writes nothing (ntr_host_kdtree_wrap rejects deeper trees up front).  An index outside
// its buffer sets NTR_STATUS_KDTREE_RANGE and ends the ray with a miss record.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kdtree_kernels.h"
#include "trace_kernels.h"

namespace ntr {

static constexpr int KD_LDS = NTR_KDTREE_LDS_DEPTH;
static constexpr int KD_SPILL = NTR_KDTREE_STACK_DEPTH - NTR_KDTREE_LDS_DEPTH;

__global__ __launch_bounds__(64) void trace_kdtree(KdTraceParams p)
{
    __shared__ int2 s_stack[KD_LDS][64];
    int2 spill[KD_SPILL];
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    if (rayIdx >= p.numRays) return;

    const float4 o = ((const float4*)p.rays)[(size_t)rayIdx * 2 + 0];
    const float4 d = ((const float4*)p.rays)[(size_t)rayIdx * 2 + 1];
    const float ox = o.x, oy = o.y, oz = o.z;
    const float dx = d.x, dy = d.y, dz = d.z;
    const float ooeps = 0x1p-80f;
    const float idirx = 1.0f / (fabsf(dx) > ooeps ? dx : copysignf(ooeps, dx));
    const float idiry = 1.0f / (fabsf(dy) > ooeps ? dy : copysignf(ooeps, dy));
    const float idirz = 1.0f / (fabsf(dz) > ooeps ? dz : copysignf(ooeps, dz));
    const float oodx = ox * idirx, oody = oy * idiry, oodz = oz * idirz;
    const float clox = p.bmin[0] * idirx - oodx, chix = p.bmax[0] * idirx - oodx;
    const float cloy = p.bmin[1] * idiry - oody, chiy = p.bmax[1] * idiry - oody;
    const float cloz = p.bmin[2] * idirz - oodz, chiz = p.bmax[2] * idirz - oodz;
    float tmin = fmaxf(fmaxf(fmaxf(fminf(clox, chix), fminf(cloy, chiy)), fminf(cloz, chiz)), o.w) - 1e-4f;
    float tmax = fminf(fminf(fminf(fmaxf(clox, chix), fmaxf(cloy, chiy)), fmaxf(cloz, chiz)), d.w) + 1e-4f;
    const float delta = p.delta;

    int node = 0;  // the root
    int sp = 0;    // entries on the stack
    int hit = -1;
    float hitU = 0.0f, hitV = 0.0f;
    bool done = false;

    while (hit == -1 && tmax >= tmin) {
        while (node >= 0 && tmax >= tmin) {
            const int4 cell = (unsigned)node < p.numNodes ? p.nodes[node] : make_int4(0, 0, 0, -1);
            const unsigned axis = ((unsigned)cell.w & 0xF0000000u) >> 28;
            if ((unsigned)node >= p.numNodes || axis > 2u) {
                atomicOr(p.status, NTR_STATUS_KDTREE_RANGE);
                hit = -1;
                done = true;
                break;
            }
            const float split = __int_as_float(cell.z);
            const float origDim = axis == 0u ? ox : (axis == 1u ? oy : oz);
            const float idirDim = axis == 0u ? idirx : (axis == 1u ? idiry : idirz);
            const float t = (split - origDim) * idirDim;
            const bool nfd = (__float_as_uint(idirDim) >> 31) != 0u;
            const int first = nfd ? cell.y : cell.x;
            const int second = nfd ? cell.x : cell.y;
            if (t > tmax) {
                node = first;
            } else if (t < tmin) {
                node = second;
            } else {
                node = first;
                const int2 e = make_int2(second, __float_as_int(tmax));
                if (sp < KD_LDS) s_stack[sp++][lane] = e;
                else if (sp < NTR_KDTREE_STACK_DEPTH) spill[(sp++) - KD_LDS] = e;
                else atomicOr(p.status, NTR_STATUS_STACK_OVERFLOW);
                tmax = t;
            }
        }
        if (done) break;

        while (node < 0) {
            if ((node & (int)0xF0000000u) != NTR_KDTREE_EMPTYLEAF) {
                for (unsigned triAddr = (unsigned)~node;; triAddr++) {
                    const int triIdx = triAddr < p.numTriIndex ? p.triIndex[triAddr] : 0;
                    if (triAddr >= p.numTriIndex || (triIdx != NTR_KDTREE_EMPTYLEAF && (unsigned)triIdx >= p.numWoopTris)) {
                        atomicOr(p.status, NTR_STATUS_KDTREE_RANGE);
                        done = true;
                        break;
                    }
                    if (triIdx == NTR_KDTREE_EMPTYLEAF) break;
                    const float4* w = p.woop + (size_t)triIdx * 3;
                    const float4 v00 = w[0];
                    const float Oz = v00.w - ox * v00.x - oy * v00.y - oz * v00.z;
                    const float invDz = 1.0f / (dx * v00.x + dy * v00.y + dz * v00.z);
                    const float t = Oz * invDz;
                    if (t >= tmin - delta && t <= tmax + delta) {
                        const float4 v11 = w[1];
                        const float Ox = v11.w + ox * v11.x + oy * v11.y + oz * v11.z;
                        const float Dx = dx * v11.x + dy * v11.y + dz * v11.z;
                        const float u = Ox + t * Dx;
                        if (u >= 0.0f && u <= 1.0f) {
                            const float4 v22 = w[2];
                            const float Oy = v22.w + ox * v22.x + oy * v22.y + oz * v22.z;
                            const float Dy = dx * v22.x + dy * v22.y + dz * v22.z;
                            const float v = Oy + t * Dy;
                            if (v >= 0.0f && u + v <= 1.0f) {
                                tmax = t;
                                hitU = u;
                                hitV = v;
                                hit = triIdx;
                            }
                        }
                    }
                }
                if (done) {
                    hit = -1;
                    break;
                }
            }
            if (hit != -1) break;
            tmin = tmax;
            if (sp == 0) {  // the bottom of the stack: traversal ends
                done = true;
                break;
            }
            --sp;
            const int2 e = sp < KD_LDS ? s_stack[sp][lane] : spill[sp - KD_LDS];
            node = e.x;
            tmax = __int_as_float(e.y);
        }
        if (done) break;
    }

    NtrRayResult r;
    if (hit != -1) {
        r.id = hit;
        r.t = tmax;
        r.padA = __float_as_int(hitU);
        r.padB = __float_as_int(hitV);
    } else {
        r.id = -1;
        r.t = d.w;
        r.padA = 0;
        r.padB = 0;
    }
    p.results[rayIdx] = r;
}

}  // namespace ntr

extern "C" hipError_t ntr_launch_trace_kdtree(const ntr::KdTraceParams* p, hipStream_t stream)
{
    const int blocks = (int)(((int64_t)p->numRays + 63) / 64);
    hipLaunchKernelGGL(ntr::trace_kdtree, dim3(blocks), dim3(64), 0, stream, *p);
    return hipGetLastError();
}
