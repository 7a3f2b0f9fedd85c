// NaiveKDTreeBuilder.cpp -- spatial-median kd-tree builder (src/rt/kdtree/NaiveKDTreeBuilder.cpp:34-160).
#include "NaiveKDTreeBuilder.hpp"

#include <utility>

namespace FW {

NaiveKDTreeBuilder::NaiveKDTreeBuilder(KDTree& kdtree, const KDTree::BuildParams&)
    : m_kdtree(kdtree), m_platform(kdtree.getPlatform()), m_numDuplicates(0)
{
}

// :43-66 -- one reference per triangle (its vertex box), the root cell is the union of those boxes
KDTreeNode* NaiveKDTreeBuilder::run(void)
{
    Scene* scene = m_kdtree.getScene();
    const Vec3i* tris = (const Vec3i*)scene->getTriVtxIndexBuffer().getPtr();
    const Vec3f* verts = (const Vec3f*)scene->getVtxPosBuffer().getPtr();
    NodeSpec root;
    root.numRef = scene->getNumTriangles();
    m_refStack.resize((size_t)root.numRef);
    for (int i = 0; i < root.numRef; i++) {
        Reference& r = m_refStack[(size_t)i];
        r.triIdx = i;
        r.bounds = AABB();
        for (int j = 0; j < 3; j++) r.bounds.grow(verts[tris[i][j]]);
        root.bounds.grow(r.bounds);
    }
    KDTreeNode* node = buildNode(root, 0);
    m_refStack.clear();
    return node;
}

// :69-88 -- the split position is the cell's middle, (lo + hi) / 2 in binary32 (findSplit, :100-115)
KDTreeNode* NaiveKDTreeBuilder::buildNode(const NodeSpec& spec, int level)
{
    if (spec.numRef <= m_platform.getMaxLeafSize() || level >= MaxDepth) return createLeaf(spec);
    const S32 dim = level % 3;
    const F32 pos = (spec.bounds.min()[dim] + spec.bounds.max()[dim]) / 2;
    NodeSpec left, right;
    performSplit(left, right, spec, dim, pos);
    KDTreeNode* rightNode = buildNode(right, level + 1);
    KDTreeNode* leftNode = buildNode(left, level + 1);
    return new KDTInnerNode(pos, dim, leftNode, rightNode);
}

// :91-97 -- references leave the top of the stack one at a time
KDTreeNode* NaiveKDTreeBuilder::createLeaf(const NodeSpec& spec)
{
    std::vector<S32>& tris = m_kdtree.getTriIndices();
    for (int i = 0; i < spec.numRef; i++) {
        tris.push_back(m_refStack.back().triIdx);
        m_refStack.pop_back();
    }
    const int hi = (int)tris.size();
    return new KDTLeafNode(hi - spec.numRef, hi);
}

// :118-158 -- one pass over the node's references that swaps left-only ones to the front and right-only ones to the back (a
// reference swapped in from the back is looked at again); what stays in the middle straddles the plane and is appended once more.
void NaiveKDTreeBuilder::performSplit(NodeSpec& left, NodeSpec& right, const NodeSpec& spec, S32 dim, F32 pos)
{
    std::vector<Reference>& refs = m_refStack;
    const int leftStart = (int)refs.size() - spec.numRef;
    int leftEnd = leftStart;
    int rightStart = (int)refs.size();
    for (int i = leftEnd; i < rightStart; i++) {
        if (refs[(size_t)i].bounds.max()[dim] <= pos) {
            std::swap(refs[(size_t)i], refs[(size_t)leftEnd]);
            leftEnd++;
        } else if (refs[(size_t)i].bounds.min()[dim] >= pos) {
            rightStart--;
            std::swap(refs[(size_t)i], refs[(size_t)rightStart]);
            i--;
        }
    }
    for (int i = leftEnd; i < rightStart; i++) {
        const Reference copy = refs[(size_t)i];
        refs.push_back(copy);
        leftEnd++;
        m_numDuplicates++;
    }
    left.numRef = leftEnd - leftStart;
    right.numRef = (int)refs.size() - rightStart;

    Vec3f leftCut = spec.bounds.max();
    leftCut[dim] = pos;
    Vec3f rightCut = spec.bounds.min();
    rightCut[dim] = pos;
    left.bounds = AABB(spec.bounds.min(), leftCut);
    right.bounds = AABB(rightCut, spec.bounds.max());
}

}  // namespace FW
