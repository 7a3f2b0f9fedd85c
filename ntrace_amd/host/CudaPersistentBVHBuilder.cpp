// CudaPersistentBVHBuilder.cpp -- Renderer("PersistentBVH")'s builder over ntr_persistent_bvh_build (see the header).
#include "CudaPersistentBVHBuilder.hpp"

#include <cstring>

namespace FW {

CudaPersistentBVHBuilder::CudaPersistentBVHBuilder(Scene* scene, F32 epsilon, const NtrPersistentBvhParams* params)
    : CudaBVH(BVHLayout_Compact), m_numTris(0)
{
    std::memset(&m_result, 0, sizeof(m_result));
    if (!scene) fail("CudaPersistentBVHBuilder: no scene");
    m_numTris = scene->getNumTriangles();
    NtrPersistentBvhParams p;
    if (params) {
        p = *params;
    } else {
        ntr_persistent_bvh_params_default(&p);
        p.epsilon = epsilon;
    }
    int64_t capN, capW, capI;
    if (ntr_lbvh_capacity(m_numTris, &capN, &capW, &capI) != NTR_OK) fail("CudaPersistentBVHBuilder: %s", ntr_last_error());
    m_nodes.resizeDiscard(capN);
    m_triWoop.resizeDiscard(capW);
    m_triIndex.resizeDiscard(capI);
    Vec3f lo, hi;
    scene->getBBox(lo, hi);
    const float mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
    const int rc = ntr_persistent_bvh_build(m_numTris, (const int32_t*)scene->getTriVtxIndexBuffer().getCudaPtr(), scene->getNumVertices(),
                                            (const float*)scene->getVtxPosBuffer().getCudaPtr(), mn, mx, &p, m_nodes.getMutableCudaPtr(), capN,
                                            m_triWoop.getMutableCudaPtr(), capW, (int32_t*)m_triIndex.getMutableCudaPtr(), capI, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaPersistentBVHBuilder: %s", ntr_last_error());
    m_nodes.resize(m_result.nodesBytes);
    m_triWoop.resize(m_result.triWoopBytes);
    m_triIndex.resize(m_result.triIndexBytes);
    invalidateTraceFlags();
}

void CudaPersistentBVHBuilder::getStats(U32& nodes, U32& leaves, U32& emptyLeaves, U32& stackTop, U32& nodeTop, U32& tris, U32& sortedTris,
                                        bool sub) const
{
    (void)sub;
    nodes = (U32)m_result.numNodes;
    leaves = (U32)m_result.numLeaves;
    emptyLeaves = m_numTris == 1 ? 1u : 0u;
    stackTop = (U32)m_result.numLevels;
    nodeTop = (U32)m_result.numNodes;
    tris = (U32)m_numTris;
    sortedTris = (U32)m_numTris;
}

}  // namespace FW
