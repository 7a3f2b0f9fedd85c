// CudaBVHTracer.hpp -- BVH tracer launcher (src/rt/cuda/CudaBVHTracer.hpp:46-107).
// Same methods; runtime nvcc compilation, texrefs and g_config read-back are
// replaced by the C-ABI (ntr_query_config / ntr_trace_bvh).
#pragma once
#include "CudaBVH.hpp"
#include "CudaVirtualTracer.hpp"

namespace FW {

class CudaBVHTracer : public CudaVirtualTracer {
public:
    CudaBVHTracer(void);
    virtual ~CudaBVHTracer(void) {}

    virtual void      setMessageWindow(Window*) {}
    virtual void      setKernel(const String& kernelName);
    virtual BVHLayout getDesiredBVHLayout(void) const { return (BVHLayout)m_kernelConfig.bvhLayout; }
    virtual void      setBVH(CudaAS* bvh) { m_bvh = bvh; }
    virtual F32       traceBatch(RayBuffer& rays);
    // Multi-GPU extension (no counterpart in the reference): trace only the slots [first, first + count) of `rays` -- a rank's
    // screen-tile range of the primary batch (Renderer::setShard).
    F32               traceRange(RayBuffer& rays, S32 first, S32 count);
    // Dispatch hint for the next traceBatch / traceRange calls (ntr_trace_bvh_hinted; NULL = none).  No counterpart in the reference.
    void              setSchedHint(NtrSchedHint* hint) { m_hint = hint; }
    // Deformation motion blur (no counterpart in the reference): the time of the rays of the next traceBatch / traceRange calls --
    // one float per ray slot of the batch (setRayTimes; NULL = none) or one for all (setTime; clearTime() takes it back).  With either
    // set, a CudaBVH that hasMotion() (CudaBVH::refitMotion) is traced by ntr_trace_bvh_motion, every ray at its own time; a CudaBVH
    // without motion is traced as ever.  Anything that is not a Compact CudaBVH -- a kd-tree, a wide tree -- fails by name.  The kernel
    // name, the trace flags and the scheduling hint do not apply to the motion launch.
    void              setRayTimes(Buffer* times) { m_rayTimes = times; }
    void              setTime(F32 time) { m_time = time; m_timeSet = true; }
    void              clearTime(void) { m_timeSet = false; }

    const KernelConfig& getKernelConfig(void) const { return m_kernelConfig; }

private:
    String       m_kernelName;
    KernelConfig m_kernelConfig;
    CudaAS*      m_bvh;
    NtrSchedHint* m_hint;
    Buffer*      m_rayTimes = NULL;
    F32          m_time = 0.0f;
    bool         m_timeSet = false;
};

}  // namespace FW
