// CudaPersistentKDTreeBuilder.hpp -- the reference's GPU kd-tree builder (src/rt/persistentds/CudaPersistentKDTreeBuilder.hpp:40-120),
// selected by Renderer("PersistentKDTree") (Renderer.cpp:348-353).  The build is ntr_kdtree_device_build: the reference's split rule
// (SPLIT_TYPE 5, PLANE_COUNT 32, no clipping; config.conf block PersistentKDTree) one level per round on the device, without the
// persistent task pool or device heap (include/ntrace_amd.h).  The object is a CudaKDTree whose three buffers wrap the
// device tree's own memory (Buffer::wrapCuda); it keeps the tree's handle and frees it on destruction.  serialize writes CudaKDTree's
// stream format, so CudaKDTree(std::istream&) reads it back.
#pragma once
#include "CudaKDTree.hpp"

namespace FW {

class CudaPersistentKDTreeBuilder : public CudaKDTree {
public:
    // Builds over the scene's device buffers (its triangle and vertex buffers are uploaded if needed).  params == NULL: config.conf's
    // PersistentKDTree block (ntr_kdtree_device_params_default).  Fails (FW::fail) with the library's message on an error.
    explicit CudaPersistentKDTreeBuilder(Scene* scene, const NtrKdtreeDeviceParams* params = NULL);
    virtual ~CudaPersistentKDTreeBuilder(void);

    // CudaPersistentKDTreeBuilder.hpp:87: the build's GPU time in seconds -- here the sum of its event-timed phases
    F32  getGPUTime(void) const { return (m_info.prepMs + m_info.levelsMs + m_info.emitMs) * 1e-3f; }
    // CudaPersistentKDTreeBuilder.hpp:88.  The reference reads counters of its task pool; here: nodes = inner nodes, leaves (empty ones
    // included), emptyLeaves, stackTop = rounds of the level loop (there is no task stack), nodeTop = inner nodes, tris = references in
    // leaves, sortedTris = the same (every reference is partitioned once per level).  sub is accepted and ignored.
    void getStats(U32& nodes, U32& leaves, U32& emptyLeaves, U32& stackTop, U32& nodeTop, U32& tris, U32& sortedTris, bool sub = true) const;
    const NtrDeviceKdtreeInfo& getInfo(void) const { return m_info; }

private:
    CudaPersistentKDTreeBuilder(const CudaPersistentKDTreeBuilder&);
    CudaPersistentKDTreeBuilder& operator=(const CudaPersistentKDTreeBuilder&);

    NtrDeviceKdtree*    m_tree;
    NtrDeviceKdtreeInfo m_info;
};

}  // namespace FW
