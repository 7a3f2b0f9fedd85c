// CudaInstancedBVH.hpp -- an instanced scene: a pool of bottom-level trees (BLAS), instances of them placed by 3x4 transforms, a
// top-level tree (TLAS) built on the device by ntr_tlas_build and the two-level trace ntr_trace_instanced (include/ntrace_amd.h,
// DESIGN.md 6k; the rule is tests/np_instanced.py).  An extension without a reference class.
//   addBLAS       copies a CudaBVH's three buffers to aligned offsets of the pool: a Compact tree's links are relative to its own
//                 start, so no word is rewritten
//   setInstances  objectToWorld per instance; worldToObject by ntr_instance_invert
//   build         the TLAS and the instance records; per frame only this is redone when instances move
//   traceBatch    closest hit or any hit as the RayBuffer asks; instanceIDs receives one S32 per ray (-1: a miss)
#pragma once
#include <vector>

#include "CudaBVH.hpp"
#include "RayBuffer.hpp"

namespace FW {

class CudaInstancedBVH {
public:
    enum { DefaultRadius = 8 };

    CudaInstancedBVH(void);
    ~CudaInstancedBVH(void) {}

    S32  addBLAS(CudaBVH& bvh);                                                  // -> the BLAS's index
    void setInstances(S32 num, const F32* objectToWorld /* num x 12 */, const S32* blas);
    void build(S32 radius = DefaultRadius);
    F32  traceBatch(RayBuffer& rays, Buffer& instanceIDs);                       // GPU seconds

    S32  getNumBLAS(void) const { return (S32)m_ranges.size(); }
    S32  getNumInstances(void) const { return m_numInstances; }
    const NtrBlasRange&  getBLASRange(S32 i) const { return m_ranges[i]; }
    const NtrTlasResult& getBuildResult(void) const { return m_result; }
    Buffer& getPoolNodeBuffer(void) { return m_poolNodes; }
    Buffer& getPoolTriWoopBuffer(void) { return m_poolTriWoop; }
    Buffer& getPoolTriIndexBuffer(void) { return m_poolTriIndex; }
    Buffer& getInstanceBuffer(void) { return m_instances; }                      // NtrInstance per instance
    Buffer& getTLASNodeBuffer(void) { return m_tlasNodes; }
    Buffer& getRecordBuffer(void) { return m_records; }

private:
    CudaInstancedBVH(const CudaInstancedBVH&);
    CudaInstancedBVH& operator=(const CudaInstancedBVH&);

    std::vector<NtrBlasRange> m_ranges;
    Buffer        m_poolNodes, m_poolTriWoop, m_poolTriIndex;
    Buffer        m_instances, m_tlasNodes, m_records;
    S32           m_numInstances;
    bool          m_built;
    NtrTlasResult m_result;
};

}  // namespace FW
