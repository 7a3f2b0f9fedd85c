// FastKDTreeBuilder.hpp -- SAH kd-tree builder, the O(N log N) event sweep with clipping of straddling triangles
// (src/rt/kdtree/FastKDTreeBuilder.hpp:37-266, FastKDTreeBuilder.cpp:39-700).
//
// Every triangle contributes, per axis, a Start and an End event at its (clipped) box's extent, or one Planar event when
// the box is flat on that axis.  The events of a node are the top of one sorted stack (order: position, then axis, then
// End < Planar < Start); one sweep over them prices every candidate plane with the SAH (sahPrice) and keeps the cheapest.
// Straddling triangles are clipped at the plane (splitBounds), the clipped boxes cut to the node's cell, and their events
// regenerated and merged into each side's sorted list.  The right child is built first; a leaf takes its triangles off
// the top of the triangle stack.  Single-threaded and deterministic.
#pragma once
#include <vector>

#include "KDTree.hpp"

namespace FW {

class FastKDTreeBuilder {
public:
    FastKDTreeBuilder(KDTree& kdtree, const KDTree::BuildParams& params);
    KDTreeNode* run(void);
    S32         getNumDuplicates(void) const { return m_numDuplicates; }
    S32         getMaxDepth(void) const { return m_maxDepth; }

private:
    enum EventType { End = 0, Planar = 1, Start = 2 };   // the sort order within one position and axis (.hpp:44-49)
    enum SahSide { Left, Right };                        // the side planar triangles on the chosen plane go to
    enum SplitSide { LeftOnly, RightOnly, Both };

    struct Event {
        S32 triIdx;
        F32 pos;
        S32 dim;
        S32 type;
    };
    struct NodeSpec {
        NodeSpec(void) : numEv(0), numTri(0) {}
        S32  numEv;   // the node's events: the top numEv entries of m_evStack
        AABB bounds;  // the node's cell
        S32  numTri;  // the node's triangles: the top numTri entries of m_triStack
    };
    struct Split {
        Split(void) : price(FW_F32_MAX), dim(-1), pos(0.0f), side(Left) {}
        F32     price;
        S32     dim;
        F32     pos;
        SahSide side;
    };

    KDTreeNode* buildNode(const NodeSpec& spec, int level, int forcedSplits);
    KDTreeNode* createLeaf(const NodeSpec& spec);
    Split       findSplit(const NodeSpec& spec) const;
    void        performSplit(NodeSpec& left, NodeSpec& right, const NodeSpec& spec, const Split& split);
    F32         sahPrice(S32 dim, F32 pos, const AABB& bounds, S32 nl, S32 nr) const;
    void        splitBounds(AABB& left, AABB& right, S32 triIdx, const Split& split) const;
    void        addEvents(std::vector<Event>& out, S32 triIdx, const AABB& box) const;
    void        mergeEvents(S32& top, const std::vector<Event>& a, const std::vector<Event>& b);
    void        sortEvents(std::vector<Event>& data, S32 lo, S32 hi);
    static bool eventLess(const Event& a, const Event& b);

    FastKDTreeBuilder(const FastKDTreeBuilder&);
    FastKDTreeBuilder& operator=(const FastKDTreeBuilder&);

    KDTree&            m_kdtree;
    const Platform&    m_platform;
    const S32          m_maxDepth;       // (S32)(1.2 log2(N) + 2), :39-47
    const S32          m_maxFailSplits;  // (S32)(1 + 0.2 maxDepth)
    const Vec3i*       m_tris;
    const Vec3f*       m_verts;
    std::vector<Event> m_evStack;
    std::vector<S32>   m_triStack;
    std::vector<U8>    m_side;            // SplitSide per scene triangle, Both between splits
    S32                m_numDuplicates;
    std::vector<Event> m_eventsLO, m_eventsRO, m_eventsBL, m_eventsBR, m_sortBuffer;
    std::vector<S32>   m_leftTriIdx, m_rightTriIdx;
};

}  // namespace FW
