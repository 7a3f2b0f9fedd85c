// Renderer.hpp -- frame driver with the reference's batching semantics
// (src/rt/cuda/Renderer.hpp:78-115; Renderer.cpp:44-94, 147-305, 405-497, 501-579, 676-710).
// Kept: setMesh / setScene / setParams / getCudaBVH / beginFrame / nextBatch / traceBatch / updateResult (countHits + reconstruct:
// SURVEY 8(f-2)) / getTotalNumRays for the primary, AO and diffuse ray types; setShard for the multi-GPU extension; the kd-tree data
// structure (builders "SpatialMedianKDTree" / "SAHKDTree" on the host and "PersistentKDTree" on the device: CudaKDTreeTracer over
// getCudaKDTree, Renderer.cpp:75-76, 309-382, 415-416); the device BVH builders "HLBVH" and "PersistentBVH" (Renderer.cpp:194-267)
// and, as extensions, "DeviceSAHBVH" and "PLOCBVH".
// Out of scope: GL display, visualisation, VPL, the persistent builders' task pools and allocators, kd-tree cache files.
#pragma once
#include "MeshWavefrontIO.hpp"
#include "CudaBVHTracer.hpp"
#include "CudaKDTreeTracer.hpp"
#include "CudaPersistentBVHBuilder.hpp"
#include "CudaPersistentKDTreeBuilder.hpp"
#include "CudaSAHBVHBuilder.hpp"
#include "CudaPLOCBuilder.hpp"
#include "HLBVHBuilder.hpp"
#include "RayGen.hpp"

namespace FW {

class Renderer {
public:
    enum RayType { RayType_Primary = 0, RayType_AO, RayType_Diffuse, RayType_Max };

    struct Params {
        String  kernelName;
        RayType rayType;
        F32     aoRadius;
        S32     numSamples;
        bool    sortSecondary;
        Params(void) : kernelName(""), rayType(RayType_Primary), aoRadius(1.0f), numSamples(32), sortSecondary(false) {}
    };

    // builder: "SAHBVH" (host, leaf preferences (1,1)), "HLBVH" (device LBVH), "PersistentBVH" (device binned SAH,
    // CudaPersistentBVHBuilder), "DeviceSAHBVH" ("SAHBVH"'s tree built on the device, CudaSAHBVHBuilder),
    // "PLOCBVH" (PLOC over the LBVH's Morton order at radius 8, CudaPLOCBuilder), or a kd-tree: "SpatialMedianKDTree" / "SAHKDTree"
    // (host builds) or "PersistentKDTree" (device build, CudaPersistentKDTreeBuilder), traced by CudaKDTreeTracer --
    // Renderer.builder / Renderer.dataStructure in config.conf
    explicit Renderer(const String& builder = "SAHBVH");
    ~Renderer(void);

    void   setScene(Scene* scene);  // a Scene the caller built and owns
    // Renderer::setMesh (src/rt/cuda/Renderer.cpp:98-132): the same mesh -> nothing; otherwise the Renderer's own Scene of the previous
    // mesh goes, the BVH is invalidated, and a Scene is made from the mesh (Scene(const MeshBase&), Scene.cpp:101-136: here the OBJ
    // importer's WavefrontMesh, whose triangle ids are the reference's).  NULL releases the mesh.
    void   setMesh(const WavefrontMesh* mesh);
    Scene* getScene(void) const { return m_scene; }
    void   setBuildParams(const BVH::BuildParams& params) { invalidateBVH(); m_buildParams = params; }
    // Mirror extension (the reference reads these from its environment, Renderer.cpp:201-209): the parameters of the "HLBVH" builder.
    // The default is hlbvh = false, leafSize 8, epsilon 0.001 -- the plain LBVH; hlbvh = true with hlbvhBits 4 is the reference's
    // setup (binned SAH over Morton clusters, ntr_hlbvh_build).  Invalidates the BVH; cache names then depend on (hlbvh, hlbvhBits).
    void   setHLBVHParams(const HLBVHParams& params) { invalidateBVH(); m_hlbvhParams = params; }
    const HLBVHParams& getHLBVHParams(void) const { return m_hlbvhParams; }
    BVH::BuildParams& getBuildParams(void) { return m_buildParams; }
    void   invalidateBVH(void) { delete m_accelStruct; m_accelStruct = NULL; m_leafDepthOf = NULL; }
    // Mirror extension (no counterpart in the reference): after Scene::setVertexPositions, bring the current BVH up to date with
    // CudaBVH::refit instead of rebuilding it (it is built first if there is none).  The leaf depths behind the AO dispatch hint are
    // kept: they are topology.  A bvhcache file is not rewritten.  A kd-tree builder fails: "Renderer::refit: the kd-tree has no refit".
    void   refit(void);
    // Mirror extension (no counterpart in the reference): CudaBVH::optimize on the current BVH (it is built first if there is none),
    // for a fresh tree or after refit().  The leaf depths behind the AO dispatch hint are recomputed at the next AO batch: they are
    // topology, which this changes.  A bvhcache file is not rewritten.  A kd-tree builder fails:
    // "Renderer::optimizeBVH: the kd-tree has no treelet optimiser".  Nothing calls this implicitly.
    void   optimizeBVH(int passes = CudaBVH::DefaultOptimizePasses);
    // Mirror extension: CudaBVH::reorder on the current BVH (it is built first if there is none), for a tree of any BVH builder,
    // fresh, refitted or optimised.  The leaf depths behind the AO dispatch hint are kept: they are per triangle and the tree is the
    // same.  A bvhcache file is not rewritten.  A kd-tree builder fails: "Renderer::reorderBVH: the kd-tree has no node order to
    // restore".  Nothing calls this implicitly.
    void   reorderBVH(void);
    void   setParams(const Params& params);
    void   setEnableRandom(bool enable) { m_enableRandom = enable; }
    CudaVirtualTracer& getCudaTracer(void) { return *m_cudaTracer; }
    CudaAS* getCudaBVH(void);   // the kd-tree for a kd-tree builder
    CudaAS* getCudaKDTree(void);  // Renderer.cpp:309-382 with the PersistentKDTree branch (:348-353), no cache files
    bool    isKDTree(void) const { return m_isKDTree; }
    // Multi-GPU (no counterpart in the reference, which is single-device).  setShard: this Renderer traces the rank-th of
    // `world` screen-tile ranges of every frame -- contiguous 64-aligned ranges of the PixelTable index space (ntr_frame_shard) -- and
    // the AO / diffuse rays of its own primary hits; (0, 1) = the whole frame.  adoptCudaBVH: use a BVH built elsewhere (the root's,
    // replicated by DistGroup::broadcastBVH) instead of building one; the Renderer owns it from then on.
    void   setShard(int rank, int world);
    S32    getShardLo(void) const { return m_shardLo; }
    S32    getShardHi(void) const { return m_shardHi; }
    void   adoptCudaBVH(CudaAS* as) { delete m_accelStruct; m_accelStruct = as; m_leafDepthOf = NULL; }
    RayGen& getRayGen(void) { return m_raygen; }
    // Dispatch hint of the AO batches (no counterpart in the reference): beside generating a batch the Renderer predicts the cost of its
    // 256-ray blocks from the depth of the leaves its pixels' primary rays hit (ntr_bvh_leaf_depths, ntr_secondary_block_costs) and hands
    // the tracer a hint that starts from that order (ntr_sched_hint_predict).  On by default; hit records do not depend on it.
    void   setPredictSecondaryOrder(bool enable) { m_predictSecondary = enable; }
    // BVH cache files, "<cachePath>/<hash>_<builder>.dat" (Renderer.cpp:173-191, 293-299; format of CudaBVH::serialize).  Off by
    // default, like Renderer.cacheDataStructure in the reference's environment.
    void   setCachePath(const String& path) { m_cachePath = path; }
    void   setCacheDataStructure(bool enable) { m_cacheDataStructure = enable; }
    String getCacheFileName(void);

    void beginFrame(const CameraView& camera);
    bool nextBatch(void);
    F32  traceBatch(void);       // launch time in seconds
    int  getTotalNumRays(void);  // for the selected ray type, excluding degenerates
    // Renderer::updateResult (Renderer.cpp:583-659): current batch -> ABGR8 pixels (width*height, by pixel id).
    // Per-triangle colours replace Scene::getTriMaterialColorBuffer / getTriShadedColorBuffer.
    void updateResult(Buffer& pixels, Buffer& triMaterialColor, Buffer& triShadedColor);
    RayBuffer& getPrimaryRays(void) { return m_primaryRays; }
    RayBuffer* getBatchRays(void) { return m_batchRays; }

private:
    void predictSecondaryOrder(void);
    F32  traceRange(RayBuffer& rays, S32 first, S32 count);  // the BVH or kd-tree tracer's traceRange
    Renderer(const Renderer&);
    Renderer& operator=(const Renderer&);

    String             m_builder;
    bool               m_isKDTree;
    Platform           m_platform;
    BVH::BuildParams   m_buildParams;
    HLBVHParams        m_hlbvhParams;
    RayGen             m_raygen;
    Params             m_params;
    bool               m_enableRandom;
    Scene*             m_scene;
    const WavefrontMesh* m_mesh;            // setMesh: the mesh m_scene was made from (the Renderer then owns m_scene)
    bool               m_ownsScene;
    F32                m_cameraFar;
    RayBuffer          m_primaryRays;
    RayBuffer          m_secondaryRays;
    bool               m_newBatch;
    RayBuffer*         m_batchRays;
    S32                m_batchStart;
    CudaAS*            m_accelStruct;
    String             m_cachePath;
    bool               m_cacheDataStructure;
    CudaVirtualTracer* m_cudaTracer;
    bool               m_predictSecondary;
    Buffer             m_leafDepth;            // S32 per triangle: depth of its leaf in m_leafDepthOf
    CudaAS*            m_leafDepthOf;
    Buffer             m_blockCost;            // U32 per 256-ray block of the current secondary batch
    NtrSchedHint*      m_secondaryHint;
    int                m_shardRank, m_shardWorld;
    S32                m_shardLo, m_shardHi;   // this rank's range of the current frame's primary slots
};

}  // namespace FW
