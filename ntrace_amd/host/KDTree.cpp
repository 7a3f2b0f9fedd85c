// KDTree.cpp -- builder dispatch and statistics (src/rt/kdtree/KDTree.cpp:36-70) and the node helpers (KDTreeNode.cpp:34-63).
#include "KDTree.hpp"

#include <chrono>

#include "FastKDTreeBuilder.hpp"
#include "NaiveKDTreeBuilder.hpp"

namespace FW {

void KDTreeNode::deleteSubtree(void)
{
    for (int i = 0; i < getNumChildNodes(); i++) getChildNode(i)->deleteSubtree();
    delete this;
}

int KDTreeNode::getSubtreeSize(KDTREE_STAT stat) const
{
    int cnt = 0;
    switch (stat) {
    case KDTREE_STAT_NODE_COUNT: cnt = 1; break;
    case KDTREE_STAT_LEAF_COUNT: cnt = isLeaf() ? 1 : 0; break;
    case KDTREE_STAT_INNER_COUNT: cnt = isLeaf() ? 0 : 1; break;
    case KDTREE_STAT_TRIANGLE_COUNT: cnt = getNumTriangles(); break;
    case KDTREE_STAT_CHILDNODE_COUNT: cnt = getNumChildNodes(); break;
    case KDTREE_STAT_EMPTYLEAF_COUNT: cnt = (isLeaf() && getNumTriangles() == 0) ? 1 : 0; break;
    }
    for (int i = 0; i < getNumChildNodes(); i++) cnt += getChildNode(i)->getSubtreeSize(stat);
    return cnt;
}

int KDTreeNode::getSubtreeDepth(void) const
{
    if (isLeaf()) return 0;
    const int a = getChildNode(0)->getSubtreeDepth(), b = getChildNode(1)->getSubtreeDepth();
    return 1 + (a > b ? a : b);
}

KDTree::KDTree(Scene* scene, const Platform& platform, const BuildParams& params) : m_scene(scene), m_platform(platform), m_root(NULL)
{
    const auto t0 = std::chrono::steady_clock::now();
    S32 numDuplicates = 0;
    if (params.builder == "SpatialMedianKDTree") {
        NaiveKDTreeBuilder builder(*this, params);
        m_root = builder.run();
        numDuplicates = builder.getNumDuplicates();
    } else if (params.builder == "SAHKDTree") {
        FastKDTreeBuilder builder(*this, params);
        m_root = builder.run();
        numDuplicates = builder.getNumDuplicates();
    } else {
        fail("Unsupported KDTree builder %s", params.builder.c_str());
    }
    if (params.stats) {
        params.stats->numLeafNodes = m_root->getSubtreeSize(KDTREE_STAT_LEAF_COUNT);
        params.stats->numInnerNodes = m_root->getSubtreeSize(KDTREE_STAT_INNER_COUNT);
        params.stats->numTris = m_root->getSubtreeSize(KDTREE_STAT_TRIANGLE_COUNT);
        params.stats->numChildNodes = m_root->getSubtreeSize(KDTREE_STAT_CHILDNODE_COUNT);
        params.stats->numEmptyLeaves = m_root->getSubtreeSize(KDTREE_STAT_EMPTYLEAF_COUNT);
        params.stats->percentDuplicates = (float)numDuplicates / m_scene->getNumTriangles() * 100;
        params.stats->maxDepth = m_root->getSubtreeDepth();
        params.stats->buildTime = (F32)std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
}

}  // namespace FW
