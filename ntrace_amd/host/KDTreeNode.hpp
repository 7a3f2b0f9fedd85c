// KDTreeNode.hpp -- kd-tree node classes (src/rt/kdtree/KDTreeNode.hpp:37-170, KDTreeNode.cpp:34-63).
#pragma once
#include "Defs.hpp"

namespace FW {

// getSubtreeSize statistics (KDTreeNode.hpp:37-45)
enum KDTREE_STAT {
    KDTREE_STAT_NODE_COUNT,
    KDTREE_STAT_INNER_COUNT,
    KDTREE_STAT_LEAF_COUNT,
    KDTREE_STAT_TRIANGLE_COUNT,
    KDTREE_STAT_CHILDNODE_COUNT,
    KDTREE_STAT_EMPTYLEAF_COUNT
};

class KDTreeNode {
public:
    virtual ~KDTreeNode(void) {}
    virtual bool        isLeaf(void) const = 0;
    virtual S32         getNumChildNodes(void) const = 0;
    virtual KDTreeNode* getChildNode(S32 i) const = 0;
    virtual S32         getNumTriangles(void) const { return 0; }

    void deleteSubtree(void);                                           // KDTreeNode.cpp:34-40
    int  getSubtreeSize(KDTREE_STAT stat = KDTREE_STAT_NODE_COUNT) const;  // KDTreeNode.cpp:43-63
    int  getSubtreeDepth(void) const;  // inner nodes on the longest root-to-leaf path (no counterpart in the reference)
};

// KDTreeNode.hpp:76-120: split plane `m_pos` on axis `m_axis`; child 0 is the side below the plane
class KDTInnerNode : public KDTreeNode {
public:
    KDTInnerNode(F32 split, S32 axis, KDTreeNode* child0, KDTreeNode* child1) : m_pos(split), m_axis(axis)
    {
        m_children[0] = child0;
        m_children[1] = child1;
    }
    bool        isLeaf(void) const { return false; }
    S32         getNumChildNodes(void) const { return 2; }
    KDTreeNode* getChildNode(S32 i) const { return m_children[i]; }

    KDTreeNode* m_children[2];
    F32         m_pos;
    S32         m_axis;
};

// KDTreeNode.hpp:125-170: the references [m_lo, m_hi) of KDTree::getTriIndices()
class KDTLeafNode : public KDTreeNode {
public:
    KDTLeafNode(int lo, int hi) : m_lo(lo), m_hi(hi) {}
    bool        isLeaf(void) const { return true; }
    S32         getNumChildNodes(void) const { return 0; }
    KDTreeNode* getChildNode(S32) const { return NULL; }
    S32         getNumTriangles(void) const { return m_hi - m_lo; }

    S32 m_lo;
    S32 m_hi;
};

}  // namespace FW
