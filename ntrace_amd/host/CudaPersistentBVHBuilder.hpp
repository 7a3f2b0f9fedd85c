// CudaPersistentBVHBuilder.hpp -- the reference's GPU SAH BVH builder (src/rt/persistentds/CudaPersistentBVHBuilder.hpp), selected by
// Renderer("PersistentBVH") (Renderer.cpp:262-267).  The build is ntr_persistent_bvh_build: the reference's split rule (SPLIT_TYPE 5,
// PLANE_COUNT 32, BINNING_TYPE 2, SAH termination, median bounds; config.conf block PersistentBVH) one level per round on the device,
// without the persistent task pool or device heap (include/ntrace_amd.h).  Like HLBVHBuilder it is a CudaBVH
// (BVHLayout_Compact) that builds itself into its own buffers, trimmed to the exact sizes; CudaBVHTracer traces it and serialize
// writes CudaBVH's stream format.
#pragma once
#include <float.h>

#include "CudaBVH.hpp"
#include "Scene.hpp"

namespace FW {

class CudaPersistentBVHBuilder : public CudaBVH {
public:
    // Builds over the scene's device buffers and its box (Scene::getBBox).  epsilon: Renderer.cpp:264 passes FLT_EPSILON; params == NULL:
    // config.conf's PersistentBVH block (ntr_persistent_bvh_params_default) with this epsilon.  Fails (FW::fail) with the library's
    // message on an error.
    explicit CudaPersistentBVHBuilder(Scene* scene, F32 epsilon = FLT_EPSILON, const NtrPersistentBvhParams* params = NULL);
    virtual ~CudaPersistentBVHBuilder(void) {}

    // CudaPersistentBVHBuilder.hpp: the build's GPU time in seconds -- here the sum of its event-timed phases
    F32  getGPUTime(void) const { return (m_result.prepMs + m_result.levelsMs + m_result.emitMs) * 1e-3f; }
    // The reference reads counters of its task pool; here: nodes = inner nodes, leaves, emptyLeaves = leaves without triangles (only the
    // one-triangle root's child 0), stackTop = rounds of the level loop (there is no task stack), nodeTop = inner nodes, tris = sortedTris
    // = triangles (every reference is partitioned once per level and never duplicated).  sub is accepted and ignored.
    void getStats(U32& nodes, U32& leaves, U32& emptyLeaves, U32& stackTop, U32& nodeTop, U32& tris, U32& sortedTris, bool sub = true) const;
    const NtrPersistentBvhResult& getBuildResult(void) const { return m_result; }

private:
    CudaPersistentBVHBuilder(const CudaPersistentBVHBuilder&);
    CudaPersistentBVHBuilder& operator=(const CudaPersistentBVHBuilder&);

    S32                    m_numTris;
    NtrPersistentBvhResult m_result;
};

}  // namespace FW
