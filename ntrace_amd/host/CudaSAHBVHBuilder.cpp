// CudaSAHBVHBuilder.cpp -- Renderer("DeviceSAHBVH")'s builder over ntr_sah_device_build (see the header).
#include "CudaSAHBVHBuilder.hpp"

#include <cstring>

namespace FW {

CudaSAHBVHBuilder::CudaSAHBVHBuilder(Scene* scene, const Platform& platform) : CudaBVH(BVHLayout_Compact)
{
    std::memset(&m_result, 0, sizeof(m_result));
    if (!scene) fail("CudaSAHBVHBuilder: no scene");
    const S32 numTris = scene->getNumTriangles();
    int64_t capN, capW, capI;
    if (ntr_lbvh_capacity(numTris, &capN, &capW, &capI) != NTR_OK) fail("CudaSAHBVHBuilder: %s", ntr_last_error());
    m_nodes.resizeDiscard(capN);
    m_triWoop.resizeDiscard(capW);
    m_triIndex.resizeDiscard(capI);
    const int rc = ntr_sah_device_build(numTris, (const int32_t*)scene->getTriVtxIndexBuffer().getCudaPtr(), scene->getNumVertices(),
                                        (const float*)scene->getVtxPosBuffer().getCudaPtr(), platform.getMinLeafSize(),
                                        platform.getMaxLeafSize(), m_nodes.getMutableCudaPtr(), capN, m_triWoop.getMutableCudaPtr(), capW,
                                        (int32_t*)m_triIndex.getMutableCudaPtr(), capI, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaSAHBVHBuilder: %s", ntr_last_error());
    m_nodes.resize(m_result.nodesBytes);
    m_triWoop.resize(m_result.triWoopBytes);
    m_triIndex.resize(m_result.triIndexBytes);
    invalidateTraceFlags();
}

}  // namespace FW
