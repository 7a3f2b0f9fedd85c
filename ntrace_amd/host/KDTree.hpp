// KDTree.hpp -- host kd-tree (src/rt/kdtree/KDTree.hpp:37-150, KDTree.cpp:36-70).
//
// The reference picks its builder from the environment (Renderer.builder); here BuildParams::builder names it:
// "SpatialMedianKDTree" (NaiveKDTreeBuilder) or "SAHKDTree" (FastKDTreeBuilder).  Both builders are single-threaded and
// deterministic: the same scene gives the same tree.
#pragma once
#include <vector>

#include "KDTreeNode.hpp"
#include "Scene.hpp"
#include "bvh/Platform.hpp"

namespace FW {

class KDTree {
public:
    // KDTree.hpp:58-80, plus the depth and the build time (no counterpart in the reference)
    struct Stats {
        Stats(void) { clear(); }
        void clear(void) { memset(this, 0, sizeof(Stats)); }
        S32 numInnerNodes;
        S32 numLeafNodes;
        S32 numChildNodes;
        S32 numTris;            // triangle references held by the leaves (KDTREE_STAT_TRIANGLE_COUNT)
        S32 numEmptyLeaves;
        F32 percentDuplicates;  // duplicated references / scene triangles * 100 (KDTree.cpp:68)
        S32 maxDepth;           // inner nodes on the longest root-to-leaf path
        F32 buildTime;          // seconds
    };

    struct BuildParams {
        BuildParams(void) : stats(NULL), builder("SAHKDTree"), enablePrints(false) {}
        Stats* stats;
        String builder;
        bool   enablePrints;
    };

    KDTree(Scene* scene, const Platform& platform, const BuildParams& params);  // KDTree.cpp:36-70
    ~KDTree(void) { if (m_root) m_root->deleteSubtree(); }

    Scene*            getScene(void) const { return m_scene; }
    const Platform&   getPlatform(void) const { return m_platform; }
    KDTreeNode*       getRoot(void) const { return m_root; }
    std::vector<S32>& getTriIndices(void) { return m_triIndices; }
    const std::vector<S32>& getTriIndices(void) const { return m_triIndices; }

private:
    KDTree(const KDTree&);
    KDTree& operator=(const KDTree&);

    Scene*           m_scene;
    Platform         m_platform;
    KDTreeNode*      m_root;
    std::vector<S32> m_triIndices;
};

}  // namespace FW
