// HLBVHBuilder.hpp -- GPU LBVH / HLBVH builder object (src/rt/bvh/HLBVH/HLBVHBuilder.hpp): a CudaBVH that
// builds itself on the device.  As in the reference (HLBVHBuilder.cpp:44-47), !hlbvh || hlbvhBits == 10 takes
// buildLBVH (ntr_lbvh_build) and anything else buildHLBVH (ntr_hlbvh_build: binned SAH over Morton clusters).
#pragma once
#include "CudaBVH.hpp"
#include "Scene.hpp"
#include "bvh/Platform.hpp"

namespace FW {

struct HLBVHParams {  // HLBVHBuilder.hpp
    bool hlbvh;
    S32  hlbvhBits;
    S32  leafSize;
    F32  epsilon;
    HLBVHParams(void) : hlbvh(false), hlbvhBits(4), leafSize(8), epsilon(0.001f) {}
};

class HLBVHBuilder : public CudaBVH {
public:
    HLBVHBuilder(Scene* scene, const Platform& platform, HLBVHParams params);
    virtual ~HLBVHBuilder(void) {}

    F32  getGPUTime(void) const { return m_gpuTime; }
    virtual F32 getRefitEpsilon(void) const { return m_params.epsilon; }   // CudaBVH::refit grows the leaf boxes as the build did
    F32  calcSAHGPU(void) { return calcSAHCost(); }                         // HLBVHBuilder.cpp:752-770 (CudaBVH::calcSAHCost)
    void getStats(U32& nodes, U32& leaves, U32& nodeTop) const { nodes = m_nodesCnt; leaves = m_leafs; nodeTop = m_nodesCnt; }
    const NtrLbvhResult& getBuildResult(void) const { return m_result; }
    const NtrHlbvhResult& getHlbvhResult(void) const { return m_hlResult; }   // zero after buildLBVH

private:
    void buildLBVH(void);
    void buildHLBVH(void);

    Scene*        m_scene;
    Platform      m_platform;
    HLBVHParams   m_params;
    F32           m_gpuTime;
    U32           m_nodesCnt, m_leafs;
    NtrLbvhResult m_result;
    NtrHlbvhResult m_hlResult;
};

}  // namespace FW
