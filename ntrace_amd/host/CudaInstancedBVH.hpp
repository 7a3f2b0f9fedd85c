// CudaInstancedBVH.hpp -- an instanced scene: a pool of bottom-level trees (BLAS), instances of them placed by 3x4 transforms, a
// top-level tree (TLAS) built on the device by ntr_tlas_build and the two-level trace ntr_trace_instanced (include/ntrace_amd.h,
// DESIGN.md 6k; the rule is tests/np_instanced.py).  An extension without a reference class.
//   addBLAS       copies a CudaBVH's three buffers to aligned offsets of the pool: a Compact tree's links are relative to its own
//                 start, so no word is rewritten
//   buildBLASes   builds every mesh of a batch straight into the pool by ntr_ploc_build_batch: one pass for all of them
//                 instead of one blocking builder call and one copy per BLAS.  The pool then holds exactly these BLASes, in mesh order
//   refitBLASes   after the meshes' vertices have moved (their triangles kept): refits the selected BLASes in place by
//                 ntr_bvh_refit_batch, all in one pass.  The meshes are those buildBLASes was given, which this class
//                 remembers; a BLAS that came through addBLAS has no mesh here and cannot be selected.  refit() (or build()) afterwards
//                 brings the TLAS to the new node-0 boxes; nothing else is needed
//   setInstances  objectToWorld per instance; worldToObject by ntr_instance_invert.  With an unchanged count the TLAS built before stays
//                 usable for refit()
//   setInstancesDevice   setInstances for transforms that live on the device, and for a hierarchy of them: numNodes
//                 local transforms (48 bytes each) with an optional parent per node, and per instance an optional node index and a
//                 BLAS index, all in device buffers.  ntr_instances_update composes every instance's chain from its root down, inverts
//                 and writes the instance array in one launch; no matrix crosses to the host.  The state follows setInstances exactly:
//                 isBuilt() falls, an unchanged count keeps the topology for refit() and the masks, a world's record is kept.
//                 check == true reads the status back and fails naming the first bad instance (a singular composition, a bad index,
//                 a chain of more than 16); check == false reads nothing back -- with a world set its one record is still copied from
//                 the host -- and leaves the status in a device buffer that getInstanceStatus reads: the caller then answers for not
//                 tracing through a bad instance
//   build         the TLAS and the instance records, from scratch: a blocking chain of launches (ntr_tlas_build)
//   refit         keeps the topology of the last build() and rewrites the records and every box from the current instances and the
//                 pool's current node-0 boxes in two launches (ntr_tlas_refit).  Needs a build() with the same instance
//                 count; a changed count, addBLAS and buildBLASes invalidate it as they invalidate build().  The frame loop of a moving,
//                 deforming scene is refitBLASes -> optimizeBLASes every so many frames -> setInstances -> refit -> traceBatch, with
//                 build() every so many frames: a refit keeps the tree the old positions suggested, and its boxes overlap more the
//                 further the instances travel.  setInstancesDevice stands in for setInstances wherever the transforms are on the
//                 device already: the loop then has no step that computes on the host
//   optimizeBLASes   restructures the selected BLASes' treelets in place by ntr_bvh_optimize_batch, all in one pass: the
//                 repair of BLASes whose refitted trees have degraded, short of buildBLASes (which replaces every BLAS and drops the
//                 world).  It needs no mesh, so addBLAS trees may be selected.  Leaves, rows and triIndex stay.  isBuilt(), the binary
//                 TLAS, the records and the world stay as they are: restructuring only re-splits a BLAS's slot 0 into two other parts,
//                 and the union of the two (min / max, exact) keeps its bits, so every box the TLAS holds is still the box of its BLAS.
//                 The wide pool is made of the binary pool's topology and is dropped with the wide TLAS, exactly as refitBLASes
//                 drops them: widen() again.  A treelet is only ever replaced by a strictly better one, so there is nothing to decide
//   measureBLASes ntr_bvh_sah_cost of every selected BLAS in two launches (ntr_bvh_sah_cost_batch): how good the trees are, before
//                 and after.  Reads only
//   setInstanceMasks  one 32-bit visibility mask per instance; NULL: all visible again.  Visibility is not geometry: the
//                 TLAS is not touched and isBuilt() stays as it was.  Fails before setInstances; a later setInstances with another
//                 count drops the masks back to all visible, one with the same count keeps them
//   traceBatch    closest hit or any hit as the RayBuffer asks; instanceIDs receives one S32 per ray (-1: a miss).  A ray enters
//                 instance i only if (mask_i & rayMask) != 0 (ntr_trace_instanced_masked); with no masks set and the default ray mask
//                 the call is ntr_trace_instanced's
//   widen          valid once isBuilt(): widens the pool into a second node buffer if the pool changed since the last widen()
//                 (ntr_pool_widen_batch; ntr_pool_widen for a pool of one BLAS: the same bytes), and the TLAS and the records always (ntr_tlas_widen).  build() and refit() drop the wide TLAS;
//                 refitBLASes, buildBLASes and addBLAS drop the wide pool too: widen again after them.  The binary pool, TLAS and
//                 records stay what they are
//   refitBLASesWide   refitBLASes, then the same selection of the wide pool in place by ntr_pool_wide_refit (rewriteRows 0:
//                 the binary refit has just written the rows).  Needs isWidePoolCurrent() on entry and keeps it: the wide BLASes keep
//                 the topology of the last pool widening.  The TLAS flags fall as after refitBLASes
//   refitWide     refit(), then the wide TLAS and the wide records in place by ntr_tlas_wide_refit.  Needs a build() and a widen() with
//                 the current instance count since, and a current wide pool; afterwards isBuilt() && isWide().  The frame loop of a
//                 moving, deforming scene on the wide path is refitBLASesWide -> setInstances (or setInstancesDevice) -> refitWide ->
//                 traceBatch, with build() + widen() every so many frames; none of its steps reads anything back but the results
//   setTraceWide  traceBatch takes the wide path (ntr_trace_instanced_wide) when isWide() and this was set; default false, so nothing
//                 changes for existing callers.  The records may differ from the binary path's in rays within rounding of a box
//                 surface (the spec tests/np_instanced_wide.py states the limit)
//   getBLASTrisBuffer  NtrBlasTris per BLAS, on the device: the meshes buildBLASes remembers, which ntr_instanced_hit_attributes needs
//                 to turn a two-level hit's id into a pool triangle.  A BLAS that came through addBLAS has numTris 0:
//                 its hits resolve to -1
//   setWorld       a static world beside the instances: one BLAS of the pool, traced in its own space -- its object space
//                 is world space -- by the single-level kernel.  It is no entry of setInstances and the TLAS never sees it: build() and
//                 refit() cover the N instances as before.  Its instance id is getNumInstances(), and while it is set getInstanceBuffer()
//                 carries one more NtrInstance at that index (identity both ways, blas = the world's), so that
//                 ntr_instanced_hit_attributes with numInstances + 1 resolves world hits without change.  traceBatch then runs
//                 ntr_trace_bvh(kernelName) on the world BLAS's range of the pool and ntr_trace_instanced_seeded (the wide form when
//                 setTraceWide and isWide() say so) in place over its records, and returns the sum of both GPU times.  Refuses a BLAS
//                 index outside the pool; traceBatch still needs at least one instance and a current TLAS.  buildBLASes replaces the
//                 pool and drops the world; clearWorld drops it and the extra record
//   setTraceFast   the binary traceBatch takes ntr_trace_instanced_fast -- with a world set, its seeded form -- in place of
//                 ntr_trace_instanced / _masked / _seeded: the same records in every word, with the FAST slab test wherever a wave's rays
//                 and the validate flags of the two levels allow it.  Default false.  The flags live in a 16-byte device buffer that
//                 buildBLASes, addBLAS, refitBLASes, optimizeBLASes, build, refit, setWorld and clearWorld mark stale; the next binary
//                 traceBatch with the switch on runs ntr_instanced_validate ahead of the trace, on its stream, once.  The wide path is
//                 untouched: with setTraceWide(true) and isWide() the switch is ignored.  A pool that holds a one-triangle BLAS has
//                 FASTDIV withheld as a whole (include/ntrace_amd.h) and runs FAST on the top level only
//   setTraceWideFast   with setTraceWide(true) and isWide(), traceBatch takes ntr_trace_instanced_wide_fast -- with a world
//                 set, its seeded form over ntr_trace_bvh's records in place -- in place of ntr_trace_instanced_wide / _wide_seeded: the
//                 same records in every word.  Default false; setTraceFast keeps being ignored on the wide path.  A second 16-byte
//                 device buffer holds the WIDE buffers' flags (ntr_instanced_wide_validate: after refitBLASesWide / refitWide's update
//                 the wide boxes are what is traced, whatever the binary flags say); widen, refitBLASesWide, refitWide, setWorld,
//                 clearWorld and everything that drops the wide pool or the wide TLAS mark it stale, and the next wide fast traceBatch
//                 validates ahead of the trace, on its stream, once
//   setMotionKey   motion blur: a second key of the instances' transforms, the shutter's close, beside setInstances' (the
//                 shutter's opening): num x 12 F32 on the host, or -- setMotionKeyDevice -- an NtrInstance array on the device, which
//                 is what a second ntr_instances_update fills (only its objectToWorld is read).  num must be getNumInstances().
//                 While hasMotion(), traceBatch takes ntr_trace_instanced_motion with setRayTimes' per-ray times (a Buffer of F32,
//                 one per ray, that stays the caller's; NULL: none) or else setTime's scalar.  refitMotion() is ntr_tlas_motion_refit
//                 over the current tree: swept leaf boxes, the moving flags in the records, the motion key buffer; it needs isBuilt().
//                 Staleness, as the FAST flags': setMotionKey, setMotionKeyDevice, setInstances, setInstancesDevice, build and refit
//                 mark the motion refit stale -- build() and refit() write records without moving flags and boxes of key 0 alone -- and
//                 the class then reports hasMotion() with isMotionStale(); the next traceBatch with motion calls refitMotion() first,
//                 exactly once.  clearMotion() drops key 1: traceBatch is the static one again, over boxes that still bound the sweep
//                 until the next refit().  setInstances with another count clears the motion, as it clears the masks.
//                 Not combinable: with motion set and setTraceWide (unless setTraceWideMotion opts in, below), setTraceFast or
//                 setTraceWideFast on, or a world set, traceBatch fail()s with a message naming the switch; it ignores neither silently.
//                 InstancedRenderer::setMotionBlur renders motion-blurred frames over this class: it points setRayTimes
//                 at each batch's hashed times for the trace (getRayTimes: the caller's pointer comes back after it) and takes the
//                 normals at the same times.
//   setTraceWideMotion   motion over the 4-wide trees, opt-in, default false: with hasMotion(), setTraceWide(true) and this on,
//                 traceBatch takes ntr_trace_instanced_wide_motion.  Off, every refusal above is what it was; without setTraceWide(true)
//                 the switch changes nothing and the launch is the binary motion launch.  setTraceWideFast, setTraceFast and a world
//                 stay refused with motion.  refitMotionWide() is refitMotion(), then ntr_tlas_wide_motion_refit in place over the wide
//                 TLAS and the wide records (swept wide boxes, the moving flags, the same key buffer); it needs what refitWide() needs
//                 -- a build() and a widen() with the current instance count since, and a current wide pool -- and afterwards
//                 isBuilt() && isWide() && !isMotionStale().  Staleness is setMotionKey's rule, and widen() and refitWide() -- which
//                 write wide records without moving flags -- make the wide side stale too (isMotionWideStale()): the next traceBatch on
//                 the wide motion path calls refitMotionWide() first, exactly once.
// Rendering: InstancedRenderer (InstancedRenderer.hpp) sits over this class and the mesh buffers and carries Renderer's batching for
// primary, AO and diffuse frames.  Per frame, the loop of a moving, deforming scene is
//   refitBLASes -> optimizeBLASes every so many frames -> setInstances (setInstancesDevice for transforms on the device) -> refit ->
//   InstancedRenderer::beginFrame -> nextBatch / traceBatch / updateResult per batch
// and with a static world set (setWorld, once) nothing of that loop changes: the world BLAS is left out of refitBLASes' selection, the
// instances move, and every traceBatch of the frame is the world's single-level trace followed by the seeded two-level trace.
#pragma once
#include <string>
#include <vector>

#include "CudaBVH.hpp"
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
    bool isMotionStale(void) const { return m_motionStale; }                     // the next traceBatch with motion calls refitMotion() first
    void refitMotion(void);
    S32  getMotionRefits(void) const { return m_motionRefits; }                  // ntr_tlas_motion_refit calls so far
    const NtrTlasMotionRefitResult& getMotionRefitResult(void) const { return m_motionRefitResult; }   // of the last refitMotion (zero before)
    void setTraceWideMotion(bool on) { m_traceWideMotion = on; }                 // motion over the 4-wide trees, with setTraceWide(true)
    bool getTraceWideMotion(void) const { return m_traceWideMotion; }
    void refitMotionWide(void);
    bool isMotionWideStale(void) const { return m_motionStale || !m_wideMotionCurrent || !m_wideTlas; }   // the next wide motion traceBatch refits first
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
    bool isFastFlagsStale(void) const { return m_fastStale; }                    // the next fast traceBatch validates first
    S32  getFastValidations(void) const { return m_fastValidations; }            // ntr_instanced_validate calls so far
    void getFastFlags(U32& tlasFlags, U32& poolFlags);                           // the granted sets; validates if stale; needs isBuilt(); blocks
    void setTraceWideFast(bool on) { m_traceWideFast = on; }
    bool getTraceWideFast(void) const { return m_traceWideFast; }
    bool isWideFastFlagsStale(void) const { return m_wideFastStale; }            // the next wide fast traceBatch validates first
    S32  getWideFastValidations(void) const { return m_wideFastValidations; }    // ntr_instanced_wide_validate calls so far
    void getWideFastFlags(U32& tlasFlags, U32& poolFlags);                       // the granted sets; validates if stale; needs isWide(); blocks
    bool isWide(void) const { return m_built && m_widePool && m_wideTlas; }      // the wide pool, TLAS and records are current
    bool isWidePoolCurrent(void) const { return m_widePool; }
    const NtrTlasWideResult& getWideResult(void) const { return m_wideResult; }            // of the last widen() (zero before)
    const NtrBvhWideResult&  getWidePoolResult(void) const { return m_widePoolResult; }    // of the last pool widening (zero before)
    const NtrWideRefitResult& getWideBLASRefitResult(void) const { return m_wideBlasRefitResult; }   // of the last refitBLASesWide (zero before)
    const NtrTlasRefitResult& getWideRefitResult(void) const { return m_wideTlasRefitResult; }       // of the last refitWide (zero before)
    Buffer& getWidePoolNodeBuffer(void) { return m_widePoolNodes; }
    Buffer& getWideTLASNodeBuffer(void) { return m_wideTlasNodes; }
    Buffer& getWideRecordBuffer(void) { return m_wideRecords; }

    Buffer& getInstanceMaskBuffer(void) { return m_instanceMasks; }              // U32 per instance; empty: all visible
    Buffer& getBLASTrisBuffer(void);                                             // NtrBlasTris per BLAS (numTris 0: an addBLAS tree)
    bool isBuilt(void) const { return m_built; }                                 // the TLAS is current: traceBatch may run
    S32  getFirstMeshlessBLAS(void) const;                                       // the first addBLAS tree of the pool, -1 if none

    S32  getNumBLAS(void) const { return (S32)m_ranges.size(); }
    S32  getNumInstances(void) const { return m_numInstances; }
    const NtrBlasRange&  getBLASRange(S32 i) const { return m_ranges[i]; }
    const NtrWideBlasRange& getWideBLASRange(S32 i) const { return m_wideRanges[i]; }   // of the wide pool; needs isWidePoolCurrent()
    const NtrTlasResult& getBuildResult(void) const { return m_result; }
    const NtrPlocBatchResult& getBLASBuildResult(void) const { return m_blasResult; }   // of the last buildBLASes (zero before)
    const NtrBvhRefitBatchResult& getBLASRefitResult(void) const { return m_refitResult; }   // of the last refitBLASes (zero before)
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
    std::vector<NtrBlasRange> m_ranges;
    std::vector<Mesh>         m_meshes;                                          // per BLAS, as m_ranges
    Buffer        m_poolNodes, m_poolTriWoop, m_poolTriIndex;
    Buffer        m_instances, m_tlasNodes, m_records;
    Buffer        m_instanceMasks;                                               // empty: no masks
    Buffer        m_blasTris;                                                    // filled from m_meshes on demand
    bool          m_blasTrisCurrent;
    S32           m_numInstances;
    bool          m_built;                                                       // the TLAS is current: traceBatch may run
    bool          m_topology;                                                    // a TLAS of m_numInstances leaves over these BLASes exists: refit may run
    bool          m_wideTopology;                                                // ... and widen() has widened it since that build(): refitWide may run
    NtrTlasResult m_result;
    NtrPlocBatchResult m_blasResult;
    NtrBvhRefitBatchResult m_refitResult;
    NtrBvhOptimizeBatchResult m_optimizeResult;
    void          selectRanges(const S32* blas, S32 num, std::vector<NtrBlasRange>& out, const char* what) const;
    NtrTlasRefitResult m_tlasRefitResult;
    Buffer        m_instanceStatus;                                              // setInstancesDevice's four status words, on the device
    NtrInstancesUpdateResult m_instancesUpdateResult;
    // the wide path (widen): a second node buffer beside the pool, a wide TLAS and wide records
    std::vector<NtrWideBlasRange> m_wideRanges;
    Buffer        m_widePoolNodes, m_wideTlasNodes, m_wideRecords;
    bool          m_widePool, m_wideTlas, m_traceWide;
    NtrBvhWideResult  m_widePoolResult;
    NtrTlasWideResult m_wideResult;
    NtrWideRefitResult m_wideBlasRefitResult;
    NtrTlasRefitResult m_wideTlasRefitResult;
    // the static world (setWorld): a BLAS of the pool that seeds the two-level trace
    void          writeWorldRecord(void);                                        // m_instances[m_numInstances], when a world is set
    S32           m_world;                                                       // -1: none
    std::string   m_worldKernel;
    // the FAST path (setTraceFast): ntr_instanced_validate's four words and whether a node box was rewritten since they were written
    const uint32_t* currentFastFlags(void);                                      // validates if stale
    Buffer        m_fastFlags;
    bool          m_traceFast, m_fastStale;
    S32           m_fastValidations;
    // the same for the wide path (setTraceWideFast): ntr_instanced_wide_validate's four words over the wide buffers
    const uint32_t* currentWideFastFlags(void);                                  // validates if stale
    Buffer        m_wideFastFlags;
    bool          m_traceWideFast, m_wideFastStale;
    S32           m_wideFastValidations;
    // motion blur (setMotionKey): key 1 of the instances, what ntr_tlas_motion_refit wrote beside the records, the rays' times
    Buffer        m_instances1, m_motionKeys;
    Buffer*       m_rayTimes;
    F32           m_time;
    bool          m_hasMotion, m_motionStale;
    S32           m_motionRefits;
    NtrTlasMotionRefitResult m_motionRefitResult;
    // motion over the 4-wide trees (setTraceWideMotion): the wide records hold the moving flags and the wide boxes the sweep
    bool          m_traceWideMotion, m_wideMotionCurrent;
    S32           m_motionWideRefits;
    NtrTlasMotionRefitResult m_motionWideRefitResult;
};

}  // namespace FW
