// kdtree_kernels.h -- launch contract between ntr_kdtree.cpp and kdtree_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntrace_amd.h"

#define NTR_KDTREE_STACK_DEPTH 64   // (node, tmax) entries per ray: LDS first, then scratch
#define NTR_KDTREE_LDS_DEPTH 8      // 8 x 64 lanes x 8 B = 4 KiB per 64-thread workgroup: 32 workgroups (the CU's wave cap) fit in 160 KiB
#define NTR_KDTREE_EMPTYLEAF ((int32_t)0x80000000)
// bits of the device status word used by the kd-tree kernel (trace_kernels.h: bit 0 = NTR_STATUS_STACK_OVERFLOW)
#define NTR_STATUS_KDTREE_RANGE 2u  // a child, list offset or triangle id outside its buffer: the ray stopped there

namespace ntr {

struct KdTraceParams {
    int32_t numRays;
    const NtrRay* rays;
    NtrRayResult* results;
    const int4* nodes;
    uint32_t numNodes;        // nodesBytes / 16
    const float4* woop;
    uint32_t numWoopTris;     // triWoopBytes / 48
    const int32_t* triIndex;
    uint32_t numTriIndex;     // triIndexBytes / 4
    float bmin[3], bmax[3];
    float delta;
    unsigned int* status;
};

}  // namespace ntr

extern "C" hipError_t ntr_launch_trace_kdtree(const ntr::KdTraceParams* p, hipStream_t stream);
