// CudaKDTree.hpp -- flattened GPU kd-tree (src/rt/cuda/CudaKDTree.hpp:40-170, CudaKDTree.cpp:4-183).
//
// Buffers (the layout trace_kdtree reads, csrc/kdtree_kernels.hip):
//   nodes    16 B per inner node: (left, right, floatBits(split), axis << 28), numbered in the order of createNodeTriIdx's
//            explicit stack (CudaKDTree.cpp:94-160: pop a node; an inner child takes the next index and is pushed, child 0
//            before child 1).  A child is a node index (>= 0), ~offset of a non-empty leaf's list in triIndex, or 0x80000000
//            for an empty leaf.
//   triIndex each non-empty leaf's triangle ids in builder order, then 0x80000000
//   triWoop  3 x float4 per SCENE triangle, indexed by triangle id (not by reference), padded to 4096 B; the rows are
//            CudaBVH's (CudaBVH::woopify with its -0 fix), so a triangle's rows equal its rows in a Compact BVH.
//   bbox     the union of the vertices of every triangle some leaf references
// DEVIATION: a tree whose root is a leaf (one triangle, or no SAH split worth making at the root) -- where the reference's
// kernel would read a child of the root and fail -- is stored as one inner node on axis 0 at bbox.max.x with the leaf as
// child 0 and an empty leaf as child 1.
#pragma once
#include "CudaAS.hpp"
#include "KDTree.hpp"

namespace FW {

class CudaKDTree : public CudaAS {
public:
    explicit CudaKDTree(const KDTree& kdtree);      // CudaKDTree.cpp:18-30
    explicit CudaKDTree(std::istream& in);          // CudaKDTree.cpp:35-40
    CudaKDTree(void) {}
    virtual ~CudaKDTree(void) {}

    virtual BVHLayout getLayout(void) const { return BVHLayout_Compact; }  // the kernel's config names Compact
    virtual Buffer&   getNodeBuffer(void) { return m_nodes; }
    virtual Buffer&   getTriWoopBuffer(void) { return m_triWoop; }
    virtual Buffer&   getTriIndexBuffer(void) { return m_triIndex; }
    // bbox.min, bbox.max (3 floats each), then nodes, triWoop, triIndex in CudaBVH's stream convention (S64 size + bytes)
    // (CudaKDTree.cpp:47-57)
    virtual void      serialize(std::ostream& out);
    // The reference's host kd-tree tracer (CudaKDTree.cpp:348-498) never narrows its interval and is not offered: this fails.
    virtual void      trace(RayBuffer& rays, Buffer& visibility);

    const AABB& getBBox(void) const { return m_bbox; }
    void        setBBox(const AABB& b) { m_bbox = b; }
    F32         getDelta(void) const;  // length(bbox.max + bbox.min) * 1e-6 (CudaKDTreeTracer.cpp:97)

private:
    void createNodeTriIdx(const KDTree& kdtree);
    void createWoopTri(const KDTree& kdtree);

    Buffer m_nodes;
    Buffer m_triIndex;
    Buffer m_triWoop;
    AABB   m_bbox;
};

}  // namespace FW
