// CudaPLOCBuilder.hpp -- a PLOC tree built on the device, selected by Renderer("PLOCBVH").  The build is ntr_ploc_build: parallel
// locally-ordered clustering over the LBVH's Morton order, mutual nearest neighbours within `radius` list positions merging round by
// round (include/ntrace_amd.h; the rule is tests/np_bvh_ploc.py).  An extension without a reference class.  Like
// CudaSAHBVHBuilder it is a CudaBVH (BVHLayout_Compact) that builds itself into its own buffers, trimmed to the exact sizes;
// CudaBVHTracer traces it, refit, optimize and reorder work on it, and serialize writes CudaBVH's stream format.
#pragma once
#include "CudaBVH.hpp"
#include "Scene.hpp"

namespace FW {

class CudaPLOCBuilder : public CudaBVH {
public:
    enum { DefaultRadius = 8 };   // a larger radius buys no quality

    // Builds over the scene's device buffers and its bounding box.  Fails (FW::fail) with the library's message on an error.
    explicit CudaPLOCBuilder(Scene* scene, S32 radius = DefaultRadius);
    virtual ~CudaPLOCBuilder(void) {}

    // the build's GPU time in seconds: the sum of its event-timed phases
    F32  getGPUTime(void) const
    {
        return (m_result.mortonMs + m_result.sortMs + m_result.emitMs + m_result.roundsMs + m_result.tailMs) * 1e-3f;
    }
    S32  getRadius(void) const { return m_radius; }
    const NtrPlocResult& getBuildResult(void) const { return m_result; }

private:
    CudaPLOCBuilder(const CudaPLOCBuilder&);
    CudaPLOCBuilder& operator=(const CudaPLOCBuilder&);

    S32           m_radius;
    NtrPlocResult m_result;
};

}  // namespace FW
