// CudaKDTree.cpp -- host kd-tree -> the three buffers of trace_kdtree (src/rt/cuda/CudaKDTree.cpp:18-183).
#include "CudaKDTree.hpp"

#include <cmath>
#include <istream>
#include <ostream>
#include <vector>

#include "CudaBVH.hpp"

namespace FW {

namespace {
const S32 kEmptyLeaf = (S32)0x80000000;  // KDTREE_EMPTYLEAF (CudaTracerKernels.hpp:45)

struct Int4 { S32 x, y, z, w; };
}  // namespace

CudaKDTree::CudaKDTree(const KDTree& kdtree)
{
    createNodeTriIdx(kdtree);
    createWoopTri(kdtree);
}

CudaKDTree::CudaKDTree(std::istream& in)
{
    Vec3f mn, mx;
    in.read((char*)&mn, sizeof(mn));
    in.read((char*)&mx, sizeof(mx));
    m_nodes.readFromStream(in);
    m_triWoop.readFromStream(in);
    m_triIndex.readFromStream(in);
    m_bbox = AABB(mn, mx);
    if (!in) setError("CudaKDTree: truncated stream");
}

void CudaKDTree::serialize(std::ostream& out)
{
    const Vec3f mn = m_bbox.min(), mx = m_bbox.max();
    out.write((const char*)&mn, sizeof(mn));
    out.write((const char*)&mx, sizeof(mx));
    m_nodes.writeToStream(out);
    m_triWoop.writeToStream(out);
    m_triIndex.writeToStream(out);
}

void CudaKDTree::trace(RayBuffer&, Buffer&)
{
    fail("CudaKDTree: no host tracer (trace kd-trees on the device, CudaKDTreeTracer)");
}

// CudaKDTreeTracer.cpp:97: (bbox.max + bbox.min).length() * 0.000001f, the length's sum taken left to right in binary32
F32 CudaKDTree::getDelta(void) const
{
    const Vec3f s = m_bbox.max() + m_bbox.min();
    return ::sqrtf(s.x * s.x + s.y * s.y + s.z * s.z) * 0.000001f;
}

// CudaKDTree.cpp:94-160
void CudaKDTree::createNodeTriIdx(const KDTree& kdtree)
{
    Scene* scene = kdtree.getScene();
    const Vec3i* tris = (const Vec3i*)scene->getTriVtxIndexBuffer().getPtr();
    const Vec3f* verts = (const Vec3f*)scene->getVtxPosBuffer().getPtr();
    const std::vector<S32>& tidx = kdtree.getTriIndices();
    std::vector<S32> triIndexData;
    m_bbox = AABB();

    // a leaf's child entry: its list appended to triIndex (+ terminator) and its vertices grown into the box
    auto emitLeaf = [&](const KDTreeNode* n) -> S32 {
        const KDTLeafNode* leaf = static_cast<const KDTLeafNode*>(n);
        const S32 ofs = (S32)triIndexData.size();
        for (int i = leaf->m_lo; i < leaf->m_hi; i++) {
            triIndexData.push_back(tidx[(size_t)i]);
            for (int j = 0; j < 3; j++) m_bbox.grow(verts[tris[tidx[(size_t)i]][j]]);
        }
        if (leaf->getNumTriangles() == 0) return kEmptyLeaf;  // ~(~KDTREE_EMPTYLEAF) through encodeIdx
        triIndexData.push_back(kEmptyLeaf);
        return ~ofs;
    };

    const KDTreeNode* root = kdtree.getRoot();
    std::vector<Int4> nodeData;
    if (root->isLeaf()) {
        // DEVIATION (CudaKDTree.hpp): one inner node over the root leaf and an empty leaf
        const S32 c0 = emitLeaf(root);
        nodeData.push_back(Int4{c0, kEmptyLeaf, (S32)floatToBits(m_bbox.max().x), 0});
    } else {
        nodeData.resize((size_t)root->getSubtreeSize(KDTREE_STAT_INNER_COUNT));
        struct Entry { const KDTreeNode* node; S32 idx; };
        std::vector<Entry> stack(1, Entry{root, 0});
        S32 nextNodeIdx = 1;
        while (!stack.empty()) {
            const Entry e = stack.back();
            stack.pop_back();
            S32 child[2];
            for (int c = 0; c < 2; c++) {
                const KDTreeNode* ch = e.node->getChildNode(c);
                if (ch->isLeaf()) {
                    child[c] = emitLeaf(ch);
                } else {
                    child[c] = nextNodeIdx;
                    stack.push_back(Entry{ch, nextNodeIdx++});
                }
            }
            const KDTInnerNode* in = static_cast<const KDTInnerNode*>(e.node);
            nodeData[(size_t)e.idx] = Int4{child[0], child[1], (S32)floatToBits(in->m_pos), (S32)(((U32)in->m_axis << 28) & 0xF0000000u)};
        }
    }
    m_nodes.set(nodeData.data(), (S64)(nodeData.size() * sizeof(Int4)));
    m_triIndex.set(triIndexData.data(), (S64)(triIndexData.size() * sizeof(S32)));
}

// CudaKDTree.cpp:74-91: rows of every scene triangle at triangle id * 48 B, the buffer rounded up to 4096 B
void CudaKDTree::createWoopTri(const KDTree& kdtree)
{
    Scene* scene = kdtree.getScene();
    const S64 n = scene->getNumTriangles();
    const Vec3i* triVtxIndex = (const Vec3i*)scene->getTriVtxIndexBuffer().getPtr();
    const Vec3f* vtxPos = (const Vec3f*)scene->getVtxPosBuffer().getPtr();
    m_triWoop.resizeDiscard((n * 48 + 4096 - 1) & ~(S64)4095);
    U8* dst = m_triWoop.getMutablePtr();
    memset(dst, 0, (size_t)m_triWoop.getSize());
    for (S64 i = 0; i < n; i++) {
        Vec4f w[3];
        CudaBVH::woopify(triVtxIndex, vtxPos, (S32)i, w);
        if (w[0].x == 0.0f) w[0].x = 0.0f;  // as CudaBVH::createCompact: a triangle's rows are the same bytes in both structures
        memcpy(dst + i * 48, w, sizeof(w));
    }
}

}  // namespace FW
