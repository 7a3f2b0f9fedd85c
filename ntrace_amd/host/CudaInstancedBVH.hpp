// CudaInstancedBVH.hpp -- an instanced scene: a pool of bottom-level trees (BLAS), instances of them placed by 3x4 transforms, a
// top-level tree (TLAS) built on the device by ntr_tlas_build and the two-level trace ntr_trace_instanced (include/ntrace_amd.h,
// DESIGN.md 6k; the rule is tests/np_instanced.py).  An extension without a reference class.
// What is current -- isBuilt(), isWide(), the FAST flags, the motion refits -- is one InstancedState (InstancedState.hpp): a
// method below names what it writes and, once its library call succeeded, what it makes; the table there says which write voids what.
//   addBLAS       copies a CudaBVH's three buffers to aligned offsets of the pool: a Compact tree's links are relative to its own
//                 start, so no word is rewritten.  writes: PoolTrees
//   buildBLASes   builds every mesh of a batch straight into the pool in one pass (ntr_ploc_build_batch).  The pool then
//                 holds exactly these BLASes, in mesh order, and a world is dropped.  writes: World, PoolTrees
//   refitBLASes   after the meshes' vertices have moved (their triangles kept): refits the selected BLASes in place in one pass
//                 (ntr_bvh_refit_batch).  The meshes are those buildBLASes was given, which this class remembers; a BLAS
//                 that came through addBLAS has no mesh here and cannot be selected.  writes: PoolBoxes
//   optimizeBLASes   restructures the selected BLASes' treelets in place in one pass (ntr_bvh_optimize_batch): the repair
//                 of BLASes whose refitted trees have degraded, short of buildBLASes.  Needs no mesh, so addBLAS trees may be selected.
//                 Leaves, rows and triIndex stay, and so does isBuilt(): a BLAS's slot 0 is only re-split into two other parts whose
//                 union (min / max, exact) keeps its bits, so every box the TLAS holds is still its BLAS's.  writes: PoolInnerBoxes
//   measureBLASes ntr_bvh_sah_cost of every selected BLAS in two launches (ntr_bvh_sah_cost_batch).  Reads only
//   setInstances  objectToWorld per instance; worldToObject by ntr_instance_invert.  Another count drops the masks and key 1 of the
//                 motion too; a world's record is kept.  writes: Instances; with another count also InstanceCount, MotionKey
//   setInstancesDevice   setInstances for transforms on the device, and for a hierarchy of them: numNodes local transforms
//                 (48 bytes each) with an optional parent per node, and per instance an optional node index and a BLAS index.
//                 ntr_instances_update composes every chain from its root down, inverts and writes the instance array in one launch.
//                 The state follows setInstances exactly.  check == true reads the status back and fails naming the first bad instance;
//                 check == false reads nothing back -- a world's one record is still copied from the host -- and leaves the status to
//                 getInstanceStatus: the caller then answers for not tracing through a bad instance
//   setInstanceMasks  one 32-bit visibility mask per instance; NULL: all visible again.  Fails before setInstances.  writes nothing
//   build         the TLAS and the instance records, from scratch: a blocking chain of launches (ntr_tlas_build).  writes and makes: TlasTopology, TlasBoxes
//   refit         keeps the last build()'s topology and rewrites the records and every box from the current instances and the pool's
//                 node-0 boxes in two launches (ntr_tlas_refit).  Needs TlasTopology.  Its boxes overlap more the further
//                 the instances travel: build() every so many frames.  writes: TlasBoxes; makes: TlasBoxes (a failed call loses it)
//   traceBatch    closest hit or any hit as the RayBuffer asks; instanceIDs receives one S32 per ray (-1: a miss).  A ray enters
//                 instance i only if (mask_i & rayMask) != 0 (ntr_trace_instanced_masked; with no masks and the default ray mask
//                 ntr_trace_instanced).  Needs isBuilt(); a stale product that its launch reads is made first, exactly once
//   widen          needs isBuilt(): widens the pool into a second node buffer unless WidePool is current
//                 (ntr_pool_widen_batch; ntr_pool_widen for a pool of one BLAS: the same bytes), and the TLAS and the
//                 records always (ntr_tlas_widen).  writes: WideTlas, WidePool; makes: WidePool, WideTlas, WideTopology
//   refitBLASesWide   refitBLASes, then the same selection of the wide pool in place (ntr_pool_wide_refit, rewriteRows 0:
//                 the binary refit has just written the rows).  Needs WidePool.  writes: PoolBoxes, WidePool; makes: WidePool
//   refitWide     refit(), then the wide TLAS and records in place (ntr_tlas_wide_refit).  Needs TlasTopology, WideTopology and
//                 WidePool; afterwards isBuilt() && isWide().  writes: TlasBoxes, WideTlas; makes: TlasBoxes, WideTlas
//   setTraceWide  traceBatch takes the wide path (ntr_trace_instanced_wide) when isWide() and this was set; default false.  The records
//                 may differ from the binary path's in rays within rounding of a box surface (tests/np_instanced_wide.py has the limit)
//   getBLASTrisBuffer  NtrBlasTris per BLAS, on the device: the meshes buildBLASes remembers, by which ntr_instanced_hit_attributes turns a
//                 two-level hit's id into a pool triangle; an addBLAS tree has numTris 0: hits resolve to -1.  makes: BlasTris
//   setWorld       a static world beside the instances: one BLAS of the pool, traced in its own space by the single-level kernel
//                 kernelName; the TLAS never sees it.  Its instance id is getNumInstances(), and while it is set getInstanceBuffer() carries
//                 one more NtrInstance there (identity, blas = the world's), so that ntr_instanced_hit_attributes with numInstances + 1
//                 resolves world hits.  traceBatch then runs ntr_trace_bvh on the world's range of the pool and ntr_trace_instanced_seeded
//                 (or the wide form) in place over its records: the sum of both GPU times.  clearWorld drops it.  writes: World
//   setTraceFast   the binary traceBatch takes ntr_trace_instanced_fast -- with a world, its seeded form: the same records
//                 in every word, with the FAST slab test wherever a wave's rays and the validate flags of the two levels allow it.
//                 Default false; ignored on the wide path.  With FastFlags stale that traceBatch, or getFastFlags, first runs
//                 ntr_instanced_validate into a 16-byte device buffer, on its stream, once: makes FastFlags.  A pool that holds a
//                 one-triangle BLAS has FASTDIV withheld as a whole (include/ntrace_amd.h) and runs FAST on the top level only
//   setTraceWideFast   the same over the wide trees: ntr_trace_instanced_wide_fast, and ntr_instanced_wide_validate over
//                 the wide buffers themselves into a second 16-byte buffer: makes WideFastFlags.  Default false
//   setMotionKey   motion blur: key 1 of the instances' transforms, the shutter's close, beside setInstances' key 0: num x 12
//                 F32 on the host, or -- setMotionKeyDevice -- an NtrInstance array on the device, as a second ntr_instances_update fills
//                 it (only objectToWorld is read).  num must be getNumInstances().  While hasMotion(), traceBatch takes
//                 ntr_trace_instanced_motion with setRayTimes' per-ray times (a Buffer of F32 that stays the caller's; NULL: none) or else
//                 setTime's scalar, after refitMotion() if isMotionStale().  clearMotion() drops key 1: traceBatch is the static one
//                 again, over boxes that still bound the sweep until the next refit().  writes: MotionKey.  With motion, setTraceWide
//                 (unless setTraceWideMotion opts in), setTraceFast, setTraceWideFast and a world are not combinable: traceBatch fail()s
//                 naming the switch.  InstancedRenderer::setMotionBlur points setRayTimes at each batch's hashed times
//   refitMotion   ntr_tlas_motion_refit over the current tree: swept leaf boxes, the moving flags in the records, the motion key buffer.
//                 Needs hasMotion() and isBuilt().  writes: TlasBoxes; makes: MotionRefit (a failed call loses TlasBoxes)
//   setTraceWideMotion   motion over the 4-wide trees, opt-in, default false: with hasMotion(), setTraceWide(true) and this on,
//                 traceBatch takes ntr_trace_instanced_wide_motion, after refitMotionWide() if isMotionWideStale(); else the binary launch
//   refitMotionWide  refitMotion(), then ntr_tlas_wide_motion_refit in place over the wide TLAS and records; needs what refitWide() and
//                 refitMotion() need.  writes: TlasBoxes, WideTlas; makes: MotionRefit, WideTlas, WideMotionRefit
//   refitBLASesMotion   deformation inside the shutter: refits the selected BLASes to TWO vertex arrays, the shutter's opening
//                 and its close (one ntr_bvh_motion_refit_batch over the selection; getBLASMotionRefitResult), into the pool and
//                 into key-1 buffers that this object owns -- the second key's nodes, the two keys' vertex rows and a flag per BLAS -- and
//                 marks them deforming.  While hasDeform(), refitMotion() takes ntr_tlas_deform_refit (without a motion key it passes key 0
//                 twice) and traceBatch ntr_trace_instanced_deform, after refitMotion() if isMotionStale().  A later refitBLASes,
//                 optimizeBLASes, buildBLASes or addBLAS leaves the second key stale: hasDeform() drops and the scene is key 0's again.
//                 clearDeform() drops it by hand.  With hasDeform(), setTraceWide, setTraceFast, setTraceWideFast, setTraceWideMotion and a
//                 world are not combinable: traceBatch fail()s naming the switch.  InstancedRenderer::setMotionBlur with setDeformGeometry
//                  resolves every batch at the ray's time, the triangle posed too, reading getBLASDeformingBuffer.
//                 writes: PoolBoxes, PoolKey1; makes: PoolDeform
// Rendering: InstancedRenderer (InstancedRenderer.hpp) sits over this class and carries Renderer's batching.  Per frame, a moving, deforming
// scene is refitBLASes -> optimizeBLASes every so many frames -> setInstances (or setInstancesDevice: no step then computes on the host) ->
// refit -> InstancedRenderer::beginFrame -> nextBatch / traceBatch / updateResult per batch, with build() every so many frames; on the wide
// path refitBLASesWide -> setInstances -> refitWide, with build() + widen().  A world's BLAS is left out of refitBLASes' selection.
#pragma once
#include <string>
#include <vector>

#include "CudaBVH.hpp"
#include "InstancedState.hpp"
#include "RayBuffer.hpp"

namespace FW {

class CudaInstancedBVH {
public:
    enum { DefaultRadius = 8 };

    CudaInstancedBVH(void);
    ~CudaInstancedBVH(void) {}

    S32  addBLAS(CudaBVH& bvh);                                                  // -> the BLAS's index
    // meshes: triangle ranges of triVtxIndex (Vec3i per triangle) over vtxPos (Vec3f per vertex), each with the box of its Morton codes;
    // BLAS k is mesh k.  Replaces whatever the pool held.
    void buildBLASes(S32 numMeshes, const NtrPlocBatchMesh* meshes, Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, S32 radius = DefaultRadius);
    // blas: num indices of BLASes to refit, each at most once (NULL: all of them); epsilon: the leaf-box rule of ntr_bvh_refit, 0 for
    // the PLOC trees buildBLASes makes.  triVtxIndex must hold the triangles buildBLASes saw.
    void refitBLASes(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas = NULL, S32 num = -1, F32 epsilon = 0.f);
    // blas: num indices of BLASes, each at most once (NULL: all of them), addBLAS trees included; passes: 1..8 treelet passes.
    void optimizeBLASes(const S32* blas = NULL, S32 num = -1, S32 passes = 2);
    // out[i]: ntr_bvh_sah_cost of the i-th selected BLAS (its seconds is 0); a BLAS may be named more than once.
    void measureBLASes(std::vector<NtrBvhSahResult>& out, const S32* blas = NULL, S32 num = -1);
    void setInstances(S32 num, const F32* objectToWorld /* num x 12 */, const S32* blas);
    // nodeLocal: numNodes x 12 F32; nodeParent: numNodes S32, -1 a root (NULL: all roots); instanceNode: num S32 (NULL: instance i uses
    // node i); blas: num S32.  All device-side inputs of ntr_instances_update.
    void setInstancesDevice(S32 numNodes, Buffer& nodeLocal, Buffer* nodeParent, S32 num, Buffer* instanceNode, Buffer& blas, bool check = true);
    void getInstanceStatus(U32 out[4]);                                          // the last setInstancesDevice's status words; blocks
    const NtrInstancesUpdateResult& getInstancesUpdateResult(void) const { return m_instancesUpdateResult; }   // of the last checked setInstancesDevice (zero otherwise)
    void build(S32 radius = DefaultRadius);
    void refit(void);
    void setInstanceMasks(const U32* masks /* getNumInstances() words; NULL: all visible */);
    void setMotionKey(S32 num, const F32* objectToWorld1 /* num x 12 */);        // key 1; num == getNumInstances()
    void setMotionKeyDevice(S32 num, Buffer& instances1 /* num NtrInstance */);
    void clearMotion(void);
    bool hasMotion(void) const { return m_hasMotion; }
    bool isMotionStale(void) const { return m_state.isMotionStale(); }           // the next traceBatch with motion calls refitMotion() first
    void refitMotion(void);
    S32  getMotionRefits(void) const { return m_motionRefits; }                  // ntr_tlas_motion_refit calls so far
    const NtrTlasMotionRefitResult& getMotionRefitResult(void) const { return m_motionRefitResult; }   // of the last refitMotion (zero before)
    // blas: num indices of BLASes, each at most once (NULL: all of them), each with a mesh of buildBLASes; vtxPos0 / vtxPos1: the shutter's
    // opening and close over the triangles buildBLASes saw
    void refitBLASesMotion(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos0, Buffer& vtxPos1, const S32* blas = NULL, S32 num = -1, F32 epsilon = 0.f);
    void clearDeform(void);
    bool hasDeform(void) const { return m_hasDeform && m_state.isPoolDeformCurrent(); }
    const NtrTlasDeformRefitResult& getDeformRefitResult(void) const { return m_deformRefitResult; }   // of the last refitMotion with hasDeform() (zero before)
    Buffer& getPoolNode1Buffer(void) { return m_poolNodes1; }                    // the second key's nodes; with getPoolVertRowBuffer(0 / 1) NtrInstanceDeform
    Buffer& getPoolVertRowBuffer(S32 key) { return key ? m_poolVertRows1 : m_poolVertRows0; }
    Buffer& getBLASDeformingBuffer(void) { return m_blasDeforming; }             // U32 per BLAS, on the device
    void setTraceWideMotion(bool on) { m_traceWideMotion = on; }                 // motion over the 4-wide trees, with setTraceWide(true)
    bool getTraceWideMotion(void) const { return m_traceWideMotion; }
    void refitMotionWide(void);
    bool isMotionWideStale(void) const { return m_state.isMotionWideStale(); }   // the next wide motion traceBatch refits first
    S32  getMotionWideRefits(void) const { return m_motionWideRefits; }          // ntr_tlas_wide_motion_refit calls so far
    const NtrTlasMotionRefitResult& getMotionWideRefitResult(void) const { return m_motionWideRefitResult; }   // of the last refitMotionWide (zero before)
    void setRayTimes(Buffer* times) { m_rayTimes = times; }                      // F32 per ray, the caller's; NULL: every ray has setTime's
    Buffer* getRayTimes(void) const { return m_rayTimes; }
    void setTime(F32 time) { m_time = time; }
    F32  getTime(void) const { return m_time; }
    Buffer& getMotionKeyBuffer(void) { return m_motionKeys; }                    // 128 bytes per instance, as refitMotion wrote them
    Buffer& getMotionInstanceBuffer(void) { return m_instances1; }               // key 1: NtrInstance per instance
    F32  traceBatch(RayBuffer& rays, Buffer& instanceIDs, U32 rayMask = 0xFFFFFFFFu);   // GPU seconds
    void widen(void);
    void refitBLASesWide(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas = NULL, S32 num = 0, F32 epsilon = 0.0f);
    void refitWide(void);
    void setWorld(S32 blas, const char* kernelName = "fermi_speculative_while_while");
    void clearWorld(void);
    bool hasWorld(void) const { return m_world >= 0; }
    S32  getWorldBLAS(void) const { return m_world; }                            // -1: no world
    void setTraceWide(bool on) { m_traceWide = on; }
    bool getTraceWide(void) const { return m_traceWide; }
    void setTraceFast(bool on) { m_traceFast = on; }
    bool getTraceFast(void) const { return m_traceFast; }
    bool isFastFlagsStale(void) const { return m_state.isFastFlagsStale(); }     // the next fast traceBatch validates first
    S32  getFastValidations(void) const { return m_fastValidations; }            // ntr_instanced_validate calls so far
    void getFastFlags(U32& tlasFlags, U32& poolFlags);                           // the granted sets; validates if stale; needs isBuilt(); blocks
    void setTraceWideFast(bool on) { m_traceWideFast = on; }
    bool getTraceWideFast(void) const { return m_traceWideFast; }
    bool isWideFastFlagsStale(void) const { return m_state.isWideFastFlagsStale(); }   // the next wide fast traceBatch validates first
    S32  getWideFastValidations(void) const { return m_wideFastValidations; }    // ntr_instanced_wide_validate calls so far
    void getWideFastFlags(U32& tlasFlags, U32& poolFlags);                       // the granted sets; validates if stale; needs isWide(); blocks
    bool isWide(void) const { return m_state.isWide(); }                         // the wide pool, TLAS and records are current
    bool isWidePoolCurrent(void) const { return m_state.isWidePoolCurrent(); }
    const NtrTlasWideResult& getWideResult(void) const { return m_wideResult; }            // of the last widen() (zero before)
    const NtrBvhWideResult&  getWidePoolResult(void) const { return m_widePoolResult; }    // of the last pool widening (zero before)
    const NtrWideRefitResult& getWideBLASRefitResult(void) const { return m_wideBlasRefitResult; }   // of the last refitBLASesWide (zero before)
    const NtrTlasRefitResult& getWideRefitResult(void) const { return m_wideTlasRefitResult; }       // of the last refitWide (zero before)
    Buffer& getWidePoolNodeBuffer(void) { return m_widePoolNodes; }
    Buffer& getWideTLASNodeBuffer(void) { return m_wideTlasNodes; }
    Buffer& getWideRecordBuffer(void) { return m_wideRecords; }

    Buffer& getInstanceMaskBuffer(void) { return m_instanceMasks; }              // U32 per instance; empty: all visible
    Buffer& getBLASTrisBuffer(void);                                             // NtrBlasTris per BLAS (numTris 0: an addBLAS tree)
    bool isBuilt(void) const { return m_state.isBuilt(); }                       // the TLAS is current: traceBatch may run
    S32  getFirstMeshlessBLAS(void) const;                                       // the first addBLAS tree of the pool, -1 if none

    S32  getNumBLAS(void) const { return (S32)m_ranges.size(); }
    S32  getNumInstances(void) const { return m_numInstances; }
    const NtrBlasRange&  getBLASRange(S32 i) const { return m_ranges[i]; }
    const NtrWideBlasRange& getWideBLASRange(S32 i) const { return m_wideRanges[i]; }   // of the wide pool; needs isWidePoolCurrent()
    const NtrTlasResult& getBuildResult(void) const { return m_result; }
    const NtrPlocBatchResult& getBLASBuildResult(void) const { return m_blasResult; }   // of the last buildBLASes (zero before)
    const NtrBvhRefitBatchResult& getBLASRefitResult(void) const { return m_refitResult; }   // of the last refitBLASes (zero before)
    const NtrBvhRefitBatchResult& getBLASMotionRefitResult(void) const { return m_blasMotionRefitResult; }   // of the last refitBLASesMotion (zero before)
    const NtrBvhOptimizeBatchResult& getBLASOptimizeResult(void) const { return m_optimizeResult; }   // of the last optimizeBLASes (zero before)
    const NtrTlasRefitResult& getRefitResult(void) const { return m_tlasRefitResult; }       // of the last refit (zero before)
    Buffer& getPoolNodeBuffer(void) { return m_poolNodes; }
    Buffer& getPoolTriWoopBuffer(void) { return m_poolTriWoop; }
    Buffer& getPoolTriIndexBuffer(void) { return m_poolTriIndex; }
    Buffer& getInstanceBuffer(void) { return m_instances; }                      // NtrInstance per instance; with a world, one more: the world's
    Buffer& getTLASNodeBuffer(void) { return m_tlasNodes; }
    Buffer& getRecordBuffer(void) { return m_records; }

private:
    CudaInstancedBVH(const CudaInstancedBVH&);
    CudaInstancedBVH& operator=(const CudaInstancedBVH&);

    struct Mesh { S32 firstTri, numTris; };                                      // numTris 0: an addBLAS tree, no mesh
    InstancedState m_state;                                                      // which derived product is current
    std::vector<NtrBlasRange> m_ranges;
    std::vector<Mesh>         m_meshes;                                          // per BLAS, as m_ranges
    Buffer        m_poolNodes, m_poolTriWoop, m_poolTriIndex;
    Buffer        m_instances, m_tlasNodes, m_records;
    Buffer        m_instanceMasks, m_blasTris;                                   // empty: no masks; filled from m_meshes on demand
    S32           m_numInstances = 0;
    NtrTlasResult m_result = {};
    NtrPlocBatchResult m_blasResult = {};
    NtrBvhRefitBatchResult m_refitResult = {};
    NtrBvhRefitBatchResult m_blasMotionRefitResult = {};
    NtrBvhOptimizeBatchResult m_optimizeResult = {};
    NtrTlasRefitResult m_tlasRefitResult = {};
    void          selectRanges(const S32* blas, S32 num, std::vector<NtrBlasRange>& out, const char* what) const;
    std::vector<NtrRefitBatchEntry> refitEntries(const S32* blas, S32 num, F32 epsilon) const;
    Buffer        m_instanceStatus;                                              // setInstancesDevice's four status words, on the device
    NtrInstancesUpdateResult m_instancesUpdateResult = {};
    // the wide path (widen): a second node buffer beside the pool, a wide TLAS and wide records
    std::vector<NtrWideBlasRange> m_wideRanges;
    Buffer        m_widePoolNodes, m_wideTlasNodes, m_wideRecords;
    bool          m_traceWide = false;
    NtrBvhWideResult  m_widePoolResult = {};
    NtrTlasWideResult m_wideResult = {};
    NtrWideRefitResult m_wideBlasRefitResult = {};
    NtrTlasRefitResult m_wideTlasRefitResult = {};
    // the static world (setWorld): a BLAS of the pool that seeds the two-level trace
    void          writeWorldRecord(void);                                        // m_instances[m_numInstances], when a world is set
    S32           m_world = -1;                                                  // -1: none
    std::string   m_worldKernel;
    // the FAST paths (setTraceFast, setTraceWideFast): ntr_instanced_validate's four words, and ntr_instanced_wide_validate's over the wide buffers
    const uint32_t* currentFastFlags(void);                                      // validates if stale
    const uint32_t* currentWideFastFlags(void);                                  // validates if stale
    Buffer        m_fastFlags, m_wideFastFlags;
    bool          m_traceFast = false, m_traceWideFast = false;
    S32           m_fastValidations = 0, m_wideFastValidations = 0;
    // motion blur (setMotionKey): key 1 of the instances, what ntr_tlas_motion_refit wrote beside the records, the rays' times
    Buffer        m_instances1, m_motionKeys;
    Buffer*       m_rayTimes = NULL;
    F32           m_time = 0.0f;
    bool          m_hasMotion = false, m_traceWideMotion = false;                // key 1 is set; motion over the 4-wide trees (setTraceWideMotion)
    S32           m_motionRefits = 0, m_motionWideRefits = 0;
    NtrTlasMotionRefitResult m_motionRefitResult = {}, m_motionWideRefitResult = {};
    // deforming BLASes (refitBLASesMotion): the pool's key-1 buffers and the flag per BLAS that ntr_tlas_deform_refit reads
    Buffer        m_poolNodes1, m_poolVertRows0, m_poolVertRows1, m_blasDeforming;
    std::vector<U32> m_deformFlags;                                              // per BLAS, as m_ranges
    bool          m_hasDeform = false;
    NtrTlasDeformRefitResult m_deformRefitResult = {};
};

}  // namespace FW
