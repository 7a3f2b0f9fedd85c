// CudaPersistentKDTreeBuilder.cpp -- Renderer("PersistentKDTree")'s builder over ntr_kdtree_device_build (see the header).
#include "CudaPersistentKDTreeBuilder.hpp"

#include <cstring>

namespace FW {

CudaPersistentKDTreeBuilder::CudaPersistentKDTreeBuilder(Scene* scene, const NtrKdtreeDeviceParams* params) : m_tree(NULL)
{
    std::memset(&m_info, 0, sizeof(m_info));
    if (!scene) fail("CudaPersistentKDTreeBuilder: no scene");
    const int rc = ntr_kdtree_device_build(scene->getNumTriangles(), (const int32_t*)scene->getTriVtxIndexBuffer().getCudaPtr(),
                                           scene->getNumVertices(), (const float*)scene->getVtxPosBuffer().getCudaPtr(), params, &m_tree, NULL);
    if (rc != NTR_OK) fail("CudaPersistentKDTreeBuilder: %s", ntr_last_error());
    if (ntr_device_kdtree_info(m_tree, &m_info) != NTR_OK) {
        ntr_device_kdtree_free(m_tree);
        m_tree = NULL;
        fail("CudaPersistentKDTreeBuilder: %s", ntr_last_error());
    }
    getNodeBuffer().wrapCuda((CUdeviceptr)m_info.nodes, m_info.nodesBytes);
    getTriWoopBuffer().wrapCuda((CUdeviceptr)m_info.triWoop, m_info.triWoopBytes);
    getTriIndexBuffer().wrapCuda((CUdeviceptr)m_info.triIndex, m_info.triIndexBytes);
    setBBox(AABB(Vec3f(m_info.sceneMin[0], m_info.sceneMin[1], m_info.sceneMin[2]),
                 Vec3f(m_info.sceneMax[0], m_info.sceneMax[1], m_info.sceneMax[2])));
}

CudaPersistentKDTreeBuilder::~CudaPersistentKDTreeBuilder(void)
{
    // the wrapped buffers never free the device memory they borrow; the tree's handle owns it
    ntr_device_kdtree_free(m_tree);
}

void CudaPersistentKDTreeBuilder::getStats(U32& nodes, U32& leaves, U32& emptyLeaves, U32& stackTop, U32& nodeTop, U32& tris, U32& sortedTris,
                                           bool sub) const
{
    (void)sub;
    nodes = (U32)m_info.numInnerNodes;
    leaves = (U32)m_info.numLeafNodes;
    emptyLeaves = (U32)m_info.numEmptyLeaves;
    stackTop = (U32)m_info.numLevels;
    nodeTop = (U32)m_info.numInnerNodes;
    tris = (U32)m_info.numTriRefs;
    sortedTris = (U32)m_info.numTriRefs;
}

}  // namespace FW
