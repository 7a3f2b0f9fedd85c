// FastKDTreeBuilder.cpp -- SAH kd-tree builder (src/rt/kdtree/FastKDTreeBuilder.cpp:39-700).  Binary32 throughout, in the
// reference's operation order; Platform("GPU") costs (node 1, triangle 1).
#include "FastKDTreeBuilder.hpp"

#include <cmath>

namespace FW {

namespace {
F32 log2f_fw(F32 a) { return ::logf(a) / ::logf(2.0f); }  // FW::log2(F32) of the host build (Math.hpp:90)
}  // namespace

// :39-47
FastKDTreeBuilder::FastKDTreeBuilder(KDTree& kdtree, const KDTree::BuildParams&)
    : m_kdtree(kdtree), m_platform(kdtree.getPlatform()),
      m_maxDepth((S32)(1.2f * log2f_fw((F32)kdtree.getScene()->getNumTriangles()) + 2.f)),
      m_maxFailSplits((S32)(1.f + 0.2f * (F32)m_maxDepth)), m_tris(NULL), m_verts(NULL), m_numDuplicates(0)
{
}

void FastKDTreeBuilder::addEvents(std::vector<Event>& out, S32 triIdx, const AABB& box) const
{
    for (int dim = 0; dim < 3; dim++) {
        if (box.min()[dim] == box.max()[dim]) {
            out.push_back(Event{triIdx, box.min()[dim], dim, Planar});
        } else {
            out.push_back(Event{triIdx, box.min()[dim], dim, Start});
            out.push_back(Event{triIdx, box.max()[dim], dim, End});
        }
    }
}

// :51-125
KDTreeNode* FastKDTreeBuilder::run(void)
{
    Scene* scene = m_kdtree.getScene();
    m_tris = (const Vec3i*)scene->getTriVtxIndexBuffer().getPtr();
    m_verts = (const Vec3f*)scene->getVtxPosBuffer().getPtr();
    NodeSpec root;
    root.numTri = scene->getNumTriangles();
    m_side.assign((size_t)root.numTri, (U8)Both);
    m_evStack.clear();
    m_triStack.clear();
    m_evStack.reserve((size_t)root.numTri * 6);
    for (int i = 0; i < root.numTri; i++) {
        m_triStack.push_back(i);
        AABB box;
        for (int j = 0; j < 3; j++) box.grow(m_verts[m_tris[i][j]]);
        root.bounds.grow(box);
        addEvents(m_evStack, i, box);
    }
    sortEvents(m_evStack, 0, (S32)m_evStack.size());
    root.numEv = (S32)m_evStack.size();
    KDTreeNode* node = buildNode(root, 0, 0);
    m_evStack.clear();
    m_triStack.clear();
    return node;
}

// :131-150 -- the node's triangles leave the top of the stack one at a time; its events are dropped
KDTreeNode* FastKDTreeBuilder::createLeaf(const NodeSpec& spec)
{
    std::vector<S32>& tris = m_kdtree.getTriIndices();
    for (int i = 0; i < spec.numTri; i++) {
        tris.push_back(m_triStack.back());
        m_triStack.pop_back();
    }
    m_evStack.resize(m_evStack.size() - (size_t)spec.numEv);
    const int hi = (int)tris.size();
    return new KDTLeafNode(hi - spec.numTri, hi);
}

// :158-195 -- forced splits: a split that saves less than 10 % counts against the subtree's budget of maxFailSplits
KDTreeNode* FastKDTreeBuilder::buildNode(const NodeSpec& spec, int level, int forcedSplits)
{
    if (level == m_maxDepth) return createLeaf(spec);
    const F32 nodePrice = m_platform.getTriangleCost(spec.numTri);
    const Split split = findSplit(spec);
    if (split.price / nodePrice > 0.9f) forcedSplits++;
    if (split.price == FW_F32_MAX || forcedSplits > m_maxFailSplits) return createLeaf(spec);
    NodeSpec left, right;
    performSplit(left, right, spec, split);
    KDTreeNode* rightNode = buildNode(right, level + 1, forcedSplits);
    KDTreeNode* leftNode = buildNode(left, level + 1, forcedSplits);
    return new KDTInnerNode(split.pos, split.dim, leftNode, rightNode);
}

// :197-277 -- one sweep; per axis nl / np / nr count the triangles left of, on, and right of the current plane
FastKDTreeBuilder::Split FastKDTreeBuilder::findSplit(const NodeSpec& spec) const
{
    S32 nl[3], np[3], nr[3];
    for (int i = 0; i < 3; i++) { nl[i] = 0; np[i] = 0; nr[i] = spec.numTri; }
    Split best;
    const int end = (int)m_evStack.size();
    for (int i = end - spec.numEv; i < end;) {
        const F32 pos = m_evStack[(size_t)i].pos;
        const S32 dim = m_evStack[(size_t)i].dim;
        S32 numEnds = 0, numPlanar = 0, numStarts = 0;
        while (i < end && m_evStack[(size_t)i].dim == dim && m_evStack[(size_t)i].pos == pos && m_evStack[(size_t)i].type == End) { numEnds++; i++; }
        while (i < end && m_evStack[(size_t)i].dim == dim && m_evStack[(size_t)i].pos == pos && m_evStack[(size_t)i].type == Planar) { numPlanar++; i++; }
        while (i < end && m_evStack[(size_t)i].dim == dim && m_evStack[(size_t)i].pos == pos && m_evStack[(size_t)i].type == Start) { numStarts++; i++; }
        np[dim] = numPlanar;
        nr[dim] -= numPlanar;
        nr[dim] -= numEnds;
        const F32 costLeft = sahPrice(dim, pos, spec.bounds, nl[dim] + np[dim], nr[dim]);
        const F32 costRight = sahPrice(dim, pos, spec.bounds, nl[dim], nr[dim] + np[dim]);
        Split cur;
        cur.dim = dim;
        cur.pos = pos;
        if (costLeft < costRight) { cur.price = costLeft; cur.side = Left; }
        else { cur.price = costRight; cur.side = Right; }
        if (cur.price < best.price) best = cur;
        nl[dim] += numStarts;
        nl[dim] += numPlanar;
        np[dim] = 0;
    }
    return best;
}

// :279-445
void FastKDTreeBuilder::performSplit(NodeSpec& left, NodeSpec& right, const NodeSpec& spec, const Split& split)
{
    const int evEnd = (int)m_evStack.size(), evBase = evEnd - spec.numEv;
    // classify by the events on the split axis; a triangle no event classifies straddles the plane
    for (int i = evBase; i < evEnd; i++) {
        const Event& e = m_evStack[(size_t)i];
        if (e.dim != split.dim) continue;
        if (e.type == End && e.pos <= split.pos) m_side[(size_t)e.triIdx] = LeftOnly;
        else if (e.type == Start && e.pos >= split.pos) m_side[(size_t)e.triIdx] = RightOnly;
        else if (e.type == Planar) {
            if (e.pos < split.pos || (e.pos == split.pos && split.side == Left)) m_side[(size_t)e.triIdx] = LeftOnly;
            else if (e.pos > split.pos || (e.pos == split.pos && split.side == Right)) m_side[(size_t)e.triIdx] = RightOnly;
        }
    }
    // the events of one-sided triangles keep their (sorted) order
    for (int i = evBase; i < evEnd; i++) {
        const U8 s = m_side[(size_t)m_evStack[(size_t)i].triIdx];
        if (s == LeftOnly) m_eventsLO.push_back(m_evStack[(size_t)i]);
        else if (s == RightOnly) m_eventsRO.push_back(m_evStack[(size_t)i]);
    }
    // triangles in stack order; a straddler is clipped at the plane, each part cut to the cell, and kept on the side(s) where the
    // part is a valid box (counted as one duplicate either way)
    const int triEnd = (int)m_triStack.size(), triBase = triEnd - spec.numTri;
    for (int i = triBase; i < triEnd; i++) {
        const S32 t = m_triStack[(size_t)i];
        const U8 s = m_side[(size_t)t];
        if (s == LeftOnly) m_leftTriIdx.push_back(t);
        else if (s == RightOnly) m_rightTriIdx.push_back(t);
        else {
            AABB lb, rb;
            splitBounds(lb, rb, t, split);
            lb.intersect(spec.bounds);
            rb.intersect(spec.bounds);
            const bool lv = lb.valid(), rv = rb.valid();
            if (lv) m_leftTriIdx.push_back(t);
            if (rv) m_rightTriIdx.push_back(t);
            m_numDuplicates++;
            if (lv) addEvents(m_eventsBL, t, lb);
            if (rv) addEvents(m_eventsBR, t, rb);
        }
        m_side[(size_t)t] = Both;
    }
    sortEvents(m_eventsBL, 0, (S32)m_eventsBL.size());
    sortEvents(m_eventsBR, 0, (S32)m_eventsBR.size());

    // the left child's events, then the right child's (on top)
    left.numEv = (S32)(m_eventsLO.size() + m_eventsBL.size());
    right.numEv = (S32)(m_eventsRO.size() + m_eventsBR.size());
    m_evStack.resize((size_t)evBase + (size_t)left.numEv + (size_t)right.numEv);
    S32 top = evBase;
    mergeEvents(top, m_eventsLO, m_eventsBL);
    mergeEvents(top, m_eventsRO, m_eventsBR);

    left.numTri = (S32)m_leftTriIdx.size();
    right.numTri = (S32)m_rightTriIdx.size();
    m_triStack.resize((size_t)triBase);
    m_triStack.insert(m_triStack.end(), m_leftTriIdx.begin(), m_leftTriIdx.end());
    m_triStack.insert(m_triStack.end(), m_rightTriIdx.begin(), m_rightTriIdx.end());

    left.bounds = spec.bounds;
    left.bounds.max()[split.dim] = split.pos;
    right.bounds = spec.bounds;
    right.bounds.min()[split.dim] = split.pos;

    m_eventsLO.clear();
    m_eventsRO.clear();
    m_eventsBL.clear();
    m_eventsBR.clear();
    m_leftTriIdx.clear();
    m_rightTriIdx.clear();
}

// :449-470 -- b's element goes first unless a's is strictly smaller
void FastKDTreeBuilder::mergeEvents(S32& top, const std::vector<Event>& a, const std::vector<Event>& b)
{
    size_t ia = 0, ib = 0;
    const size_t n = a.size() + b.size();
    for (size_t k = 0; k < n; k++) {
        if (ia == a.size()) m_evStack[(size_t)top++] = b[ib++];
        else if (ib == b.size()) m_evStack[(size_t)top++] = a[ia++];
        else if (eventLess(a[ia], b[ib])) m_evStack[(size_t)top++] = a[ia++];
        else m_evStack[(size_t)top++] = b[ib++];
    }
}

// :473-510 -- flat cells cost FW_F32_MAX, so do planes on a cell face with nothing beyond them; an empty side off the cell's
// faces earns the 0.8 bonus
F32 FastKDTreeBuilder::sahPrice(S32 dim, F32 pos, const AABB& bounds, S32 nl, S32 nr) const
{
    AABB lb = bounds;
    lb.max()[dim] = pos;
    AABB rb = bounds;
    rb.min()[dim] = pos;
    if (bounds.min()[0] == bounds.max()[0] || bounds.min()[1] == bounds.max()[1] || bounds.min()[2] == bounds.max()[2]) return FW_F32_MAX;
    if ((pos == bounds.min()[dim] && nl == 0) || (pos == bounds.max()[dim] && nr == 0)) return FW_F32_MAX;
    const F32 pl = lb.area() / bounds.area();
    const F32 pr = rb.area() / bounds.area();
    F32 cost = pl * m_platform.getTriangleCost(nl) + pr * m_platform.getTriangleCost(nr);
    if ((nl == 0 || nr == 0) && !(pos == bounds.min()[dim] || pos == bounds.max()[dim])) cost *= 0.8f;
    cost += m_platform.getNodeCost(1);
    return cost;
}

// :512-615 -- the triangle's vertices ordered along the split axis (first minimum; ties between the other two keep the
// later one second); the two edges crossing the plane give the two new vertices, put exactly on the plane
void FastKDTreeBuilder::splitBounds(AABB& left, AABB& right, S32 triIdx, const Split& split) const
{
    const int d = split.dim;
    const Vec3f v[3] = {m_verts[m_tris[triIdx][0]], m_verts[m_tris[triIdx][1]], m_verts[m_tris[triIdx][2]]};
    int a = 0;
    for (int i = 0; i < 3; i++)
        if (v[i][d] < v[a][d]) a = i;
    int b, c;
    if (v[(a + 1) % 3][d] < v[(a + 2) % 3][d]) { b = (a + 1) % 3; c = (a + 2) % 3; }
    else { b = (a + 2) % 3; c = (a + 1) % 3; }

    left = AABB();
    right = AABB();
    left.grow(v[a]);
    right.grow(v[c]);
    if (v[b][d] <= split.pos) {
        const F32 aToSplit = split.pos - v[a][d], bToSplit = split.pos - v[b][d];
        const F32 aToC = v[c][d] - v[a][d], bToC = v[c][d] - v[b][d];
        const Vec3f e1 = (v[c] - v[a]) * (aToSplit / aToC);
        const Vec3f e2 = (v[c] - v[b]) * (bToSplit / bToC);
        Vec3f n1 = v[a] + e1, n2 = v[b] + e2;
        n1[d] = split.pos;
        n2[d] = split.pos;
        left.grow(v[b]);
        left.grow(n1);
        left.grow(n2);
        right.grow(n1);
        right.grow(n2);
    } else if (v[b][d] > split.pos) {
        const F32 aToSplit = split.pos - v[a][d];
        const F32 aToB = v[b][d] - v[a][d], aToC = v[c][d] - v[a][d];
        const Vec3f e1 = (v[b] - v[a]) * (aToSplit / aToB);
        const Vec3f e2 = (v[c] - v[a]) * (aToSplit / aToC);
        Vec3f n1 = v[a] + e1, n2 = v[a] + e2;
        n1[d] = split.pos;
        n2[d] = split.pos;
        left.grow(n1);
        left.grow(n2);
        right.grow(n1);
        right.grow(n2);
        right.grow(v[b]);
    }
}

// :683-700
bool FastKDTreeBuilder::eventLess(const Event& a, const Event& b)
{
    if (a.pos == b.pos) {
        if (a.dim == b.dim) return a.type < b.type;
        return a.dim < b.dim;
    }
    return a.pos < b.pos;
}

// :617-680 -- top-down merge sort, halves split at (lo + hi) / 2; a merge takes the left element only when it is strictly
// smaller (the reference's in-place merge does the same: its right half is never the shorter one)
void FastKDTreeBuilder::sortEvents(std::vector<Event>& data, S32 lo, S32 hi)
{
    if (hi - lo <= 1) return;
    const S32 mid = (hi + lo) / 2;
    sortEvents(data, lo, mid);
    sortEvents(data, mid, hi);
    m_sortBuffer.assign(data.begin() + lo, data.begin() + mid);
    size_t il = 0;
    S32 ir = mid, out = lo;
    while (il < m_sortBuffer.size()) {
        if (ir >= hi || eventLess(m_sortBuffer[il], data[(size_t)ir])) data[(size_t)out++] = m_sortBuffer[il++];
        else data[(size_t)out++] = data[(size_t)ir++];
    }
}

}  // namespace FW
