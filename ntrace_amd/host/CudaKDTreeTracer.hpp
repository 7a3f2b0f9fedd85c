// CudaKDTreeTracer.hpp -- kd-tree tracer launcher (src/rt/cuda/CudaKDTreeTracer.hpp:40-104, CudaKDTreeTracer.cpp:46-128).
// setKernel accepts any name and always runs the kd-tree kernel, as the reference's does (it replaces the name by
// fermi_kdtree_while_while_leafRef); its config, {Compact, 64, 1, 0}, is the tracer's own (no ntr_query_config entry).
#pragma once
#include "CudaKDTree.hpp"
#include "CudaVirtualTracer.hpp"

namespace FW {

class CudaKDTreeTracer : public CudaVirtualTracer {
public:
    CudaKDTreeTracer(void);
    virtual ~CudaKDTreeTracer(void) {}

    virtual void      setMessageWindow(Window*) {}
    virtual void      setKernel(const String& kernelName);
    virtual BVHLayout getDesiredBVHLayout(void) const { return (BVHLayout)m_kernelConfig.bvhLayout; }
    virtual void      setBVH(CudaAS* as);   // a CudaKDTree (anything else fails)
    virtual F32       traceBatch(RayBuffer& rays);
    // the slots [first, first + count) of `rays` (the Renderer's shard of a primary batch; CudaBVHTracer::traceRange)
    F32               traceRange(RayBuffer& rays, S32 first, S32 count);

    const KernelConfig& getKernelConfig(void) const { return m_kernelConfig; }

private:
    String       m_kernelName;
    KernelConfig m_kernelConfig;
    CudaKDTree*  m_kdtree;
};

}  // namespace FW
