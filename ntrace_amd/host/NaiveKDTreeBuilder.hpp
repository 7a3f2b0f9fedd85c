// NaiveKDTreeBuilder.hpp -- spatial-median kd-tree builder (src/rt/kdtree/NaiveKDTreeBuilder.hpp:37-175, .cpp:34-160).
//
// A node is split at the middle of its cell on axis level % 3; a reference whose box lies at or below the plane goes left,
// one at or above it right (the first test wins for a box flat on the plane), and a straddling reference is kept on the left
// and copied onto the right.  A node becomes a leaf at numRef <= Platform::getMaxLeafSize() or at level MaxDepth.  The
// references of a node are the top of one stack: the right child (the top part) is built first, and a leaf takes its
// references off the top of the stack (so in reverse order).
#pragma once
#include <vector>

#include "KDTree.hpp"

namespace FW {

class NaiveKDTreeBuilder {
public:
    enum { MaxDepth = 18 };  // NaiveKDTreeBuilder.hpp:47

    NaiveKDTreeBuilder(KDTree& kdtree, const KDTree::BuildParams& params);
    KDTreeNode* run(void);
    S32         getNumDuplicates(void) const { return m_numDuplicates; }

private:
    struct Reference {
        S32  triIdx;
        AABB bounds;
    };
    struct NodeSpec {
        S32  numRef;
        AABB bounds;
    };

    KDTreeNode* buildNode(const NodeSpec& spec, int level);
    KDTreeNode* createLeaf(const NodeSpec& spec);
    void        performSplit(NodeSpec& left, NodeSpec& right, const NodeSpec& spec, S32 dim, F32 pos);

    NaiveKDTreeBuilder(const NaiveKDTreeBuilder&);
    NaiveKDTreeBuilder& operator=(const NaiveKDTreeBuilder&);

    KDTree&                m_kdtree;
    const Platform&        m_platform;
    std::vector<Reference> m_refStack;
    S32                    m_numDuplicates;
};

}  // namespace FW
