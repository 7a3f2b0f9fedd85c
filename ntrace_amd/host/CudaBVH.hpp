// CudaBVH.hpp -- flattened GPU BVH (src/rt/cuda/CudaBVH.hpp:95-330).
//
// BVHLayout_Compact (CudaBVH.hpp:42-56):
//   nodes   [innerOfs +  0] = (c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y)
//           [innerOfs + 16] = (c1.lo.x, c1.hi.x, c1.lo.y, c1.hi.y)
//           [innerOfs + 32] = (c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z)
//           [innerOfs + 48] = (c0 byte offset or ~c0.triOfs, c1 ..., splitBits, 0)
//   triWoop [triOfs*16 + 0/16/32] = woopZ, woopU, woopV ; leaf terminator = 0x80000000
//   triIndex[triOfs] = original triangle id (parallel to triWoop float4 index)
#pragma once
#include "CudaAS.hpp"
#include "bvh/BVH.hpp"

namespace FW {

class CudaBVH : public CudaAS {
public:
    enum { Align = 4096 };

    explicit CudaBVH(const BVH& bvh, BVHLayout layout);         // CudaBVH.cpp:60-103
    explicit CudaBVH(BVHLayout layout) : m_layout(layout), m_flags(0), m_flagsValid(false), m_refitResult() {}
    explicit CudaBVH(std::istream& in);                          // CudaBVH.cpp:105-108
    virtual ~CudaBVH(void) {}

    virtual BVHLayout getLayout(void) const { return m_layout; }
    virtual Buffer&   getNodeBuffer(void) { return m_nodes; }
    virtual Buffer&   getTriWoopBuffer(void) { return m_triWoop; }
    virtual Buffer&   getTriIndexBuffer(void) { return m_triIndex; }
    virtual void      serialize(std::ostream& out);             // CudaBVH.cpp:118-125
    virtual void      trace(RayBuffer& rays, Buffer& visibility) { trace(rays, visibility, NULL); }  // CudaBVH.cpp:213-302 (host tracer)
    void              trace(RayBuffer& rays, Buffer& visibility, RayStats* stats);

    // Hint flags for ntr_trace_bvh (NTR_BVH_FINITE), computed once on the device.
    U32 getTraceFlags(void);
    void invalidateTraceFlags(void) { m_flagsValid = false; }

    // Mirror extension (the reference's scenes are static; no counterpart there): keep the topology and recompute every box and Woop
    // row on the device from the scene's CURRENT vertex positions (ntr_bvh_refit on this tree's buffers; the scene must hold the
    // triangles the tree was built over, see Scene::setVertexPositions), then invalidateTraceFlags().  Works on a tree of any
    // origin, a bvhcache import included.  epsilon grows the leaf boxes; refit(scene) takes getRefitEpsilon(): 0, the exact union a
    // host SAH tree stores, unless the builder says otherwise (HLBVHBuilder: the epsilon it was built with).  Blocking; fails
    // (FW::fail) with the library's message.
    void        refit(Scene& scene, F32 epsilon);
    void        refit(Scene& scene) { refit(scene, getRefitEpsilon()); }
    virtual F32 getRefitEpsilon(void) const { return 0.0f; }
    const NtrBvhRefitResult& getRefitResult(void) const { return m_refitResult; }   // of the last refit (zero before the first)

    // Mirror extension: deformation motion blur (ntr_bvh_motion_refit; the rule is tests/np_bvh_motion.py).  Key 0, the shutter's
    // opening, is the scene's CURRENT vertex positions, as for refit(); key 1, its close, is key1Positions: scene.getNumVertices()
    // host vectors.  The tree's own buffers come out as refit() leaves them; the object owns the key-1 node buffer and the two keys'
    // vertex rows, and hasMotion() says that they are current.  A CudaBVHTracer with a time or ray times set then traces every ray at
    // its own time (ntr_trace_bvh_motion).  A later refit(), optimize() or reorder() drops the motion state: the tree is static again,
    // at whatever that call leaves.  Blocking; fails (FW::fail) with the library's message, the motion state then dropped.
    void        refitMotion(Scene& scene, const Vec3f* key1Positions, F32 epsilon);
    void        refitMotion(Scene& scene, const Vec3f* key1Positions) { refitMotion(scene, key1Positions, getRefitEpsilon()); }
    bool        hasMotion(void) const { return m_hasMotion; }
    Buffer&     getMotionNodeBuffer(void) { return m_nodes1; }                // key 1's nodes (empty without motion)
    Buffer&     getVertRowsBuffer(int key) { return m_vertRows[key ? 1 : 0]; } // a key's vertex rows (empty without motion)

    // Mirror extension (no counterpart in the reference): restructure the tree's treelets on the device for a lower SAH cost
    // (ntr_bvh_optimize on this tree's node buffer; triangles and leaves stay), then invalidateTraceFlags().  Works on a tree of any
    // origin, fresh or refitted.  Leaf depths change with the topology: whoever cached ntr_bvh_leaf_depths recomputes them
    // (Renderer::optimizeBVH does).  passes in 1..8; DefaultOptimizePasses is the count after which the measured trace rate stopped
    // improving by more than its run-to-run spread.  Nothing calls this implicitly.  Blocking; fails (FW::fail) with
    // the library's message.
    enum { DefaultOptimizePasses = 2 };
    void        optimize(int passes = DefaultOptimizePasses);
    const NtrBvhOptimizeResult& getOptimizeResult(void) const { return m_optimizeResult; }   // of the last optimize (zero before)
    // Mirror extension (no counterpart in the reference as a pass of its own): renumber the tree on the device into the node and row
    // order createCompact gives a host tree (ntr_bvh_reorder into three fresh Buffers of the current sizes, which are swapped in and
    // trimmed to the result's extents), then invalidateTraceFlags(): the top-of-tree table belongs to the node buffer.  The tree --
    // boxes, topology, leaf contents, leaf depths -- stays; slots and rows no link reaches are dropped.  Works on a tree of any
    // origin.  Nothing calls this implicitly.  Blocking; fails (FW::fail) with the library's message, the tree then as it was.
    void        reorder(void);
    const NtrBvhReorderResult& getReorderResult(void) const { return m_reorderResult; }       // of the last reorder (zero before)
    // HLBVHBuilder::calcSAHGPU (HLBVHBuilder.cpp:752-770) for a tree of any origin: ntr_bvh_sah_cost on this tree's buffers.
    F32         calcSAHCost(void);
    const NtrBvhSahResult& getSAHResult(void) const { return m_sahResult; }                   // of the last calcSAHCost

protected:
    friend class CudaKDTree;  // the kd-tree's Woop rows are CudaBVH's (CudaKDTree.hpp)
    void createCompact(const BVH& bvh, int nodeOffsetSizeDiv);  // CudaBVH.cpp:579-664
    static void woopify(const Vec3i* triVtxIndex, const Vec3f* vtxPos, S32 tri, Vec4f (&out)[3]);  // CudaBVH.cpp:668-687

    BVHLayout m_layout;
    Buffer    m_nodes;
    Buffer    m_triWoop;
    Buffer    m_triIndex;
    U32       m_flags;
    bool      m_flagsValid;
    NtrBvhRefitResult m_refitResult;
    void      dropMotion(void);
    Buffer    m_nodes1;
    Buffer    m_vertRows[2];
    bool      m_hasMotion = false;
    NtrBvhOptimizeResult m_optimizeResult = NtrBvhOptimizeResult();
    NtrBvhSahResult   m_sahResult = NtrBvhSahResult();
    NtrBvhReorderResult m_reorderResult = NtrBvhReorderResult();
};

}  // namespace FW
