#include "CudaKDTreeTracer.hpp"

namespace FW {

CudaKDTreeTracer::CudaKDTreeTracer(void) : m_kdtree(NULL)
{
    m_scene = NULL;
    m_kernelConfig.bvhLayout = BVHLayout_Compact;
    m_kernelConfig.blockWidth = 64;   // one wave per 64-thread workgroup (csrc/kdtree_kernels.hip)
    m_kernelConfig.blockHeight = 1;
    m_kernelConfig.usePersistentThreads = 0;
}

// CudaKDTreeTracer::setKernel (CudaKDTreeTracer.cpp:46-66): every name selects fermi_kdtree_while_while_leafRef
void CudaKDTreeTracer::setKernel(const String& kernelName) { m_kernelName = kernelName; }

void CudaKDTreeTracer::setBVH(CudaAS* as)
{
    m_kdtree = NULL;
    if (as && !(m_kdtree = dynamic_cast<CudaKDTree*>(as))) fail("CudaKDTreeTracer: not a kd-tree");
}

// CudaKDTreeTracer::traceBatch (CudaKDTreeTracer.cpp:70-128)
F32 CudaKDTreeTracer::traceBatch(RayBuffer& rays) { return traceRange(rays, 0, rays.getSize()); }

F32 CudaKDTreeTracer::traceRange(RayBuffer& rays, S32 first, S32 count)
{
    if (first < 0 || count < 0 || first + count > rays.getSize()) fail("CudaKDTreeTracer: ray range out of bounds");
    if (!count) return 0.0f;
    if (!m_kdtree) fail("CudaKDTreeTracer: No kd-tree!");
    const AABB& b = m_kdtree->getBBox();
    const float mn[3] = {b.min().x, b.min().y, b.min().z}, mx[3] = {b.max().x, b.max().y, b.max().z};
    float seconds = 0.0f;
    const int rc = ntr_trace_kdtree(count, rays.getNeedClosestHit() ? 0 : 1, mn, mx, (const NtrRay*)rays.getRayBuffer().getCudaPtr() + first,
                                    (NtrRayResult*)rays.getResultBuffer().getMutableCudaPtr() + first, m_kdtree->getNodeBuffer().getCudaPtr(),
                                    m_kdtree->getNodeBuffer().getSize(), m_kdtree->getTriWoopBuffer().getCudaPtr(),
                                    m_kdtree->getTriWoopBuffer().getSize(), (const int32_t*)m_kdtree->getTriIndexBuffer().getCudaPtr(),
                                    m_kdtree->getTriIndexBuffer().getSize(), NULL, &seconds);
    if (rc != NTR_OK) fail("CudaKDTreeTracer: %s", ntr_last_error());
    return seconds;
}

}  // namespace FW
