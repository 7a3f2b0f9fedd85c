// instanced_attr_kernels.hip -- what a two-level hit needs before anything indexes by triangle, for gfx950
// (ntr_instanced_hit_attributes).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_frame.py, and the header comment of ntr_instanced_hit_attributes
// (include/ntrace_amd.h) states the contract.  ntr_trace_instanced leaves (id, t, u, v) and an instance id per ray; id is the BLAS's own
// triangle id, relative to its mesh's firstTri, so neither a colour table nor a normal table can be indexed by it, and a table of
// normals would go stale with every ntr_bvh_refit_batch anyway.  One launch, a thread per ray, turns the pair into the pool triangle
// g = firstTri + id and the world-space geometric normal of that triangle from the CURRENT vertices:
//   reads       the record (16 B), the instance id (4 B); of a hit: worldToObject as three 16-byte loads (byte 48 of the 112-byte
//               NtrInstance of a 16-byte aligned array) and the blas word, the BLAS's (firstTri, numTris), three vertex indices, nine
//               coordinates
//   writes      one 16-byte store per output per ray
// Every index is range checked before it is used: whatever the records, the instances, the table or the index array hold, nothing
// outside the buffers is read.  No scratch, no read-back, no atomics: the call is capturable as it stands.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instanced_attr.h"

namespace ntr {
namespace {

// (instanced_attr.h states these steps once more, as functions, for instanced_motion_attr_kernels.hip: this kernel calling them compiles
// to other code than it had, so its text stays as it was -- DESIGN.md 6ab)
__global__ __launch_bounds__(IHA_BLOCK) void instanced_hit_attributes_kernel(int numRays, const int4* results, const int* __restrict__ instanceIDs,
                                                                             const NtrInstance* __restrict__ inst, int numInstances,
                                                                             const int2* __restrict__ blasTris, int numBlas,
                                                                             const int* __restrict__ triVtx, int numTrisTotal,
                                                                             const float* __restrict__ pos, int numVerts, int4* outResults,
                                                                             float4* __restrict__ normals)
{
    const unsigned int r = blockIdx.x * (unsigned int)IHA_BLOCK + threadIdx.x;   // < 2^31 + IHA_BLOCK
    if (r >= (unsigned int)numRays) return;
    const int4 res = results[r];             // (outResults may be results: this thread alone reads and writes record r)
    const int id = res.x;
    int g = -1;
    float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int i = instanceIDs[r];
    if (id >= 0 && i >= 0 && i < numInstances) {
        const int b = inst[i].blas;
        if (b >= 0 && b < numBlas) {
            const int2 bt = blasTris[b];     // (firstTri, numTris)
            const long long gg = (long long)bt.x + id;
            if (id < bt.y && gg >= 0 && gg < numTrisTotal) {
                const int va = triVtx[3 * (size_t)gg], vb = triVtx[3 * (size_t)gg + 1], vc = triVtx[3 * (size_t)gg + 2];
                if (va >= 0 && va < numVerts && vb >= 0 && vb < numVerts && vc >= 0 && vc < numVerts) {
                    g = (int)gg;
                    if (normals) {
                        const float* pa = pos + 3 * (size_t)va;
                        const float* pb = pos + 3 * (size_t)vb;
                        const float* pc = pos + 3 * (size_t)vc;
                        const float ax = pa[0], ay = pa[1], az = pa[2];
                        const float e1x = pb[0] - ax, e1y = pb[1] - ay, e1z = pb[2] - az;
                        const float e2x = pc[0] - ax, e2y = pc[1] - ay, e2z = pc[2] - az;
                        // the object-space normal (Scene.cpp:112's cross product)
                        const float ox = e1y * e2z - e1z * e2y, oy = e1z * e2x - e1x * e2z, oz = e1x * e2y - e1y * e2x;
                        // through the transpose of worldToObject's linear part: the inverse transpose of objectToWorld
                        const float4* w = reinterpret_cast<const float4*>(inst[i].worldToObject);
                        const float4 w0 = w[0], w1 = w[1], w2 = w[2];
                        const float wx = (w0.x * ox + w1.x * oy) + w2.x * oz;
                        const float wy = (w0.y * ox + w1.y * oy) + w2.y * oz;
                        const float wz = (w0.z * ox + w1.z * oy) + w2.z * oz;
                        const float l2 = (wx * wx + wy * wy) + wz * wz;
                        if (l2 > 0.0f && l2 < __builtin_inff()) {   // (a NaN fails both)
                            const float inv = 1.0f / sqrtf(l2);
                            nrm = make_float4(wx * inv, wy * inv, wz * inv, 1.0f);
                        }
                    }
                }
            }
        }
    }
    if (outResults) outResults[r] = make_int4(g, res.y, res.z, res.w);
    if (normals) normals[r] = nrm;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_instanced_hit_attributes(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs, const NtrInstancedGeometry* geom,
                                 NtrRayResult* d_outResults, float* d_normals, void* stream)
{
    const char* fn = "ntr_instanced_hit_attributes";
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (attr_check(fn, d_results, d_instanceIDs, geom, d_outResults, d_normals) != NTR_OK) return NTR_ERR_INVALID;

    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    hipLaunchKernelGGL(instanced_hit_attributes_kernel, dim3((unsigned int)(((long long)numRays + IHA_BLOCK - 1) / IHA_BLOCK)), dim3(IHA_BLOCK), 0,
                       (hipStream_t)stream, (int)numRays, reinterpret_cast<const int4*>(d_results), d_instanceIDs, geom->d_instances,
                       (int)geom->numInstances, reinterpret_cast<const int2*>(geom->d_blasTris), (int)geom->numBlas, geom->d_triVtxIndex,
                       (int)geom->numTrisTotal, geom->d_vtxPos, (int)geom->numVerts, reinterpret_cast<int4*>(d_outResults),
                       reinterpret_cast<float4*>(d_normals));
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // extern "C"
