// CudaWideBVH.cpp -- a 4-wide tree over a CudaBVH, through ntr_bvh_widen / ntr_trace_wide (see the header).
#include "CudaWideBVH.hpp"

#include <cstring>

namespace FW {

CudaWideBVH::CudaWideBVH(CudaBVH& bvh) : m_bvh(bvh)
{
    std::memset(&m_result, 0, sizeof(m_result));
}

void CudaWideBVH::build(void)
{
    std::memset(&m_result, 0, sizeof(m_result));
    if (m_bvh.getLayout() != BVHLayout_Compact) fail("CudaWideBVH: Incorrect BVH layout!");
    Buffer& nodes = m_bvh.getNodeBuffer();
    int64_t cap = 0;
    if (ntr_bvh_widen_capacity(nodes.getSize(), &cap) != NTR_OK) fail("CudaWideBVH: %s", ntr_last_error());
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) fail("CudaWideBVH: no device (ntr_bvh_widen has no CPU fallback)");
    m_wideNodes.resizeDiscard(cap);
    const int rc = ntr_bvh_widen(nodes.getCudaPtr(), nodes.getSize(), m_wideNodes.getMutableCudaPtr(), cap, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaWideBVH: %s", ntr_last_error());
    m_wideNodes.resize(m_result.nodesBytes);
}

F32 CudaWideBVH::traceBatch(RayBuffer& rays)
{
    const S32 numRays = rays.getSize();
    if (!numRays) return 0.0f;
    if (!m_result.nodesBytes) fail("CudaWideBVH: No wide tree!");
    float seconds = 0.0f;
    Buffer &woop = m_bvh.getTriWoopBuffer(), &index = m_bvh.getTriIndexBuffer();
    const int rc = ntr_trace_wide(numRays, rays.getNeedClosestHit() ? 0 : 1, (const NtrRay*)rays.getRayBuffer().getCudaPtr(),
                                  (NtrRayResult*)rays.getResultBuffer().getMutableCudaPtr(), m_wideNodes.getCudaPtr(), m_result.nodesBytes,
                                  woop.getCudaPtr(), woop.getSize(), (const int32_t*)index.getCudaPtr(), m_bvh.getTraceFlags(), NULL, &seconds);
    if (rc != NTR_OK) fail("CudaWideBVH: %s", ntr_last_error());
    return seconds;
}

}  // namespace FW
