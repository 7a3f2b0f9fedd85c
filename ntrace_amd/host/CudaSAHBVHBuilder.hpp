// CudaSAHBVHBuilder.hpp -- the host SAH builder's tree built on the device, selected by Renderer("DeviceSAHBVH").  The build is
// ntr_sah_device_build: SAHBVHBuilder's rule (full sweeps over three presorted axis orders, Platform("GPU"), the platform's leaf
// preferences) one level per round on the device (include/ntrace_amd.h).  An extension without a reference class: the
// reference builds this tree on the host only (Renderer("SAHBVH"), which keeps doing so here).  Like CudaPersistentBVHBuilder it is a
// CudaBVH (BVHLayout_Compact) that builds itself into its own buffers, trimmed to the exact sizes; CudaBVHTracer traces it, refit and
// optimize work on it, and serialize writes CudaBVH's stream format.
#pragma once
#include "CudaBVH.hpp"
#include "Scene.hpp"
#include "bvh/Platform.hpp"

namespace FW {

class CudaSAHBVHBuilder : public CudaBVH {
public:
    // Builds over the scene's device buffers with the platform's leaf preferences (Renderer: (1, 1)).  Fails (FW::fail) with the
    // library's message on an error.
    CudaSAHBVHBuilder(Scene* scene, const Platform& platform);
    virtual ~CudaSAHBVHBuilder(void) {}

    // the build's GPU time in seconds: the sum of its event-timed phases
    F32  getGPUTime(void) const { return (m_result.prepMs + m_result.sortMs + m_result.levelsMs + m_result.emitMs) * 1e-3f; }
    const NtrSahDeviceResult& getBuildResult(void) const { return m_result; }

private:
    CudaSAHBVHBuilder(const CudaSAHBVHBuilder&);
    CudaSAHBVHBuilder& operator=(const CudaSAHBVHBuilder&);

    NtrSahDeviceResult m_result;
};

}  // namespace FW
