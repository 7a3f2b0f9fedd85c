// CudaPLOCBuilder.cpp -- Renderer("PLOCBVH")'s builder over ntr_ploc_build (see the header).
#include "CudaPLOCBuilder.hpp"

#include <cstring>

namespace FW {

CudaPLOCBuilder::CudaPLOCBuilder(Scene* scene, S32 radius) : CudaBVH(BVHLayout_Compact), m_radius(radius)
{
    std::memset(&m_result, 0, sizeof(m_result));
    if (!scene) fail("CudaPLOCBuilder: no scene");
    const S32 numTris = scene->getNumTriangles();
    int64_t capN, capW, capI;
    if (ntr_lbvh_capacity(numTris, &capN, &capW, &capI) != NTR_OK) fail("CudaPLOCBuilder: %s", ntr_last_error());
    m_nodes.resizeDiscard(capN);
    m_triWoop.resizeDiscard(capW);
    m_triIndex.resizeDiscard(capI);
    Vec3f lo, hi;
    scene->getBBox(lo, hi);
    const float mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
    const int rc = ntr_ploc_build(numTris, (const int32_t*)scene->getTriVtxIndexBuffer().getCudaPtr(), scene->getNumVertices(),
                                  (const float*)scene->getVtxPosBuffer().getCudaPtr(), mn, mx, radius, m_nodes.getMutableCudaPtr(), capN,
                                  m_triWoop.getMutableCudaPtr(), capW, (int32_t*)m_triIndex.getMutableCudaPtr(), capI, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaPLOCBuilder: %s", ntr_last_error());
    m_nodes.resize(m_result.nodesBytes);
    m_triWoop.resize(m_result.triWoopBytes);
    m_triIndex.resize(m_result.triIndexBytes);
    invalidateTraceFlags();
}

}  // namespace FW
