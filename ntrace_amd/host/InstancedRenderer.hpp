// InstancedRenderer.hpp -- frames of an instanced scene: Renderer's batching (src/rt/cuda/Renderer.cpp:405-497, 501-579, 583-659,
// 676-710) for the primary, AO and diffuse ray types over a CudaInstancedBVH and the meshes its BLASes were built from.  An extension
// without a reference class.
//   setGeometry   the index and vertex buffers CudaInstancedBVH::buildBLASes / refitBLASes were given; the vertex buffer holds the
//                 CURRENT positions whenever a batch is traced (the buffers are borrowed, not copied)
//   setParams     the ray type, the AO radius and the samples per primary hit
//   setRayMasks   the ray masks of CudaInstancedBVH::traceBatch: primary batches are traced with the first, AO and diffuse
//                 batches with the second; both default to all ones.  Nothing else in the frame changes: a masked-out primary hit is a
//                 miss, and ntr_instanced_hit_attributes resolves it as one
//   setWide       trace every batch of the frame over the 4-wide trees (CudaInstancedBVH::widen); default false.  beginFrame
//                 widens when the CudaInstancedBVH is not wide -- that is, after each build() / refit() of the frame loop -- and the
//                 batches are traced with setTraceWide(true), which is put back after each trace.  Nothing else of the frame changes:
//                 the hit attributes, the AO rays and the reconstruction read the binary geometry, which the wide path keeps
//   setFast       trace every binary batch of the frame with the FAST slab test where the rays and the validate flags allow it
//                 (CudaInstancedBVH::setTraceFast); default false.  The batches are traced with setTraceFast(true) -- or
//                 with whatever the CudaInstancedBVH itself was told, when this is off -- which is put back after each trace.  The
//                 records are the same in every word, so nothing else of the frame changes.  The wide path is untouched: with
//                 setWide(true) the switch is ignored
//   setWideFast   the same for the wide batches of a setWide(true) frame (CudaInstancedBVH::setTraceWideFast); default
//                 false; in the manner of setFast: on, or whatever the CudaInstancedBVH itself was told, and put back after each trace
//   setMotionBlur motion-blurred frames over a CudaInstancedBVH with a motion key (setMotionKey); default off, and off
//                 every path is what it was: the batches are traced as the CudaInstancedBVH stands, the caller's setRayTimes
//                 included, and resolved at key 0.  On: beginFrame fails unless the CudaInstancedBVH hasMotion() or hasDeform() (a scene
//                 that only deforms renders blurred frames: refitMotion() passes key 0 twice), then gives every
//                 pixel one hashed time in the shutter [open, close] (ntr_ray_times_primary over the primary slot-to-id table; another
//                 seed per accumulated frame gives another sample); every batch is traced with setRayTimes pointing at its times -- the
//                 caller's pointer is put back after each trace -- and resolved by ntr_instanced_hit_attributes_motion with the same key
//                 buffer and times, so the normal is the one of the pose the ray hit; an AO or diffuse ray inherits its primary
//                 ray's time (ntr_ray_times_secondary): it sees its instance where its primary ray saw it.  Primary, AO and diffuse
//                 frames all work.  setWide (without setWideMotion), setFast, setWideFast and a world stay not combinable with motion:
//                 the CudaInstancedBVH's traceBatch refuses each by name, and the refusal is passed on
//   setDeformGeometry  motion-blurred frames over deforming BLASes (CudaInstancedBVH::refitBLASesMotion): the closing vertices
//                 refitBLASesMotion was last given -- setGeometry's vertex buffer holds the opening ones -- borrowed, not copied; refused
//                 when the buffer is smaller than numVerts * 12 bytes.  Under setMotionBlur with hasDeform(), every batch is resolved by
//                 ntr_instanced_hit_attributes_deform with the CudaInstancedBVH's flag buffer (getBLASDeformingBuffer): the normal is the one
//                 of the triangle posed at the ray's time, the triangle ntr_trace_instanced_deform tested.  The trace and the inherited
//                 secondary times are setMotionBlur's, unchanged.  Without it (or after clearDeformGeometry) beginFrame refuses
//                 setMotionBlur over deforming BLASes, as the normals would be key 0's.  Once hasDeform() drops (refitBLASes, clearDeform)
//                 the frames are the motion path's again.  Without setMotionBlur a deforming scene keeps key-0 normals and the scalar time
//   setWideMotion motion-blurred frames over the 4-wide trees (CudaInstancedBVH::setTraceWideMotion); default false; in the
//                 manner of setFast: on, or whatever the CudaInstancedBVH itself was told, and put back after each trace.  With it on,
//                 setWide(true) and setMotionBlur(true), primary, AO and diffuse frames run over the wide trees: the first batch after
//                 beginFrame's widen() refits both trees over the two keys (refitMotionWide); times, attributes at the ray's time and
//                 inherited secondary times are exactly setMotionBlur's -- ntr_instanced_hit_attributes_motion takes no records
//   beginFrame    w x h primary rays from the camera's position and nscreenToWorld (its width and height are not read); for AO and
//                 diffuse frames the primary rays are traced and resolved at once
//   nextBatch / traceBatch / updateResult / getTotalNumRays  as Renderer's.  Every traced batch is resolved by
//                 ntr_instanced_hit_attributes before anything indexes by triangle: the records updateResult and getTotalNumRays
//                 read name POOL triangles (the caller's colour tables are per pool triangle, in object space), and the AO and diffuse
//                 rays start from the world-space normals of the current vertices (ntr_raygen_ao_normals)
// With a static world set on the CudaInstancedBVH (setWorld) primary, AO and diffuse frames run through its traceBatch
// unchanged otherwise: every batch is the world's single-level trace followed by the seeded two-level trace (AO batches any-hit), world
// hits carry instance id getNumInstances() and resolve through the one more NtrInstance the instance buffer then holds, and updateResult
// works over pool triangles as before.
// beginFrame fails, and says what to do, when there is no geometry, when the CudaInstancedBVH's TLAS is not current (build() or refit()
// after setInstances / refitBLASes), and when the pool holds a tree that came through addBLAS (its mesh is not known here).
// No kd-tree, no shard, no cache and no dispatch hints; Renderer itself is untouched.
#pragma once
#include "CudaInstancedBVH.hpp"
#include "RayGen.hpp"

namespace FW {

class InstancedRenderer {
public:
    enum RayType { RayType_Primary = 0, RayType_AO, RayType_Diffuse, RayType_Max };   // Renderer::RayType's values: ntr_reconstruct's rayType

    explicit InstancedRenderer(CudaInstancedBVH& bvh);

    void setGeometry(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos);
    void setDeformGeometry(Buffer& vtxPos1);
    void clearDeformGeometry(void) { m_vtxPos1 = NULL; }
    void setParams(RayType rayType, F32 aoRadius, S32 numSamples);
    void setRayMasks(U32 primaryMask = 0xFFFFFFFFu, U32 secondaryMask = 0xFFFFFFFFu);
    void setWide(bool on) { m_wide = on; }
    bool getWide(void) const { return m_wide; }
    void setFast(bool on) { m_fast = on; }
    bool getFast(void) const { return m_fast; }
    void setWideFast(bool on) { m_wideFast = on; }
    bool getWideFast(void) const { return m_wideFast; }
    void setWideMotion(bool on) { m_wideMotion = on; }
    bool getWideMotion(void) const { return m_wideMotion; }
    void setMotionBlur(bool on, U32 seed = 0, F32 open = 0.0f, F32 close = 1.0f);
    bool getMotionBlur(void) const { return m_motionBlur; }

    void beginFrame(const CameraView& camera, S32 w, S32 h);
    bool nextBatch(void);
    F32  traceBatch(void);       // the two-level trace's GPU seconds
    int  getTotalNumRays(void);  // for the selected ray type, excluding degenerates
    void updateResult(Buffer& pixels, Buffer& triMaterialColor, Buffer& triShadedColor);   // colours per pool triangle

    RayGen&    getRayGen(void) { return m_raygen; }
    RayBuffer& getPrimaryRays(void) { return m_primaryRays; }
    RayBuffer* getBatchRays(void) { return m_batchRays; }
    Buffer&    getPrimaryResolvedBuffer(void) { return m_primaryResolved; }   // NtrRayResult per primary slot, ids of pool triangles
    Buffer&    getPrimaryNormalBuffer(void) { return m_primaryNormals; }      // 4 floats per primary slot
    Buffer&    getBatchResolvedBuffer(void) { return *m_batchResolved; }      // NtrRayResult per slot of the current batch
    Buffer&    getPrimaryInstanceIDBuffer(void) { return m_primaryIDs; }      // S32 per primary slot: the instance of the hit (AO, diffuse)
    Buffer&    getBatchInstanceIDBuffer(void) { return m_batchRays == &m_primaryRays ? m_primaryIDs : m_secondaryIDs; }   // of the current batch
    Buffer&    getPrimaryTimeBuffer(void) { return m_primaryTimes; }          // setMotionBlur: F32 per primary slot
    Buffer&    getBatchTimeBuffer(void) { return m_batchRays == &m_primaryRays ? m_primaryTimes : m_secondaryTimes; }   // F32 per slot of the current batch

private:
    // times: the batch's, read when setMotionBlur is on
    void resolve(RayBuffer& rays, Buffer& instanceIDs, Buffer& times, Buffer& resolved, Buffer* normals);
    // the CudaInstancedBVH's traceBatch, wide when setWide asked for it, fast when setFast / setWideFast did, at `times` under setMotionBlur
    F32  trace(RayBuffer& rays, Buffer& instanceIDs, Buffer& times, U32 rayMask);
    InstancedRenderer(const InstancedRenderer&);
    InstancedRenderer& operator=(const InstancedRenderer&);

    CudaInstancedBVH& m_bvh;
    Buffer*    m_triVtxIndex;
    Buffer*    m_vtxPos;
    Buffer*    m_vtxPos1;                                // setDeformGeometry: the closing vertices, or NULL
    S32        m_numVerts;
    RayType    m_rayType;
    F32        m_aoRadius;
    S32        m_numSamples;
    U32        m_primaryMask, m_secondaryMask;
    bool       m_wide, m_fast, m_wideFast, m_wideMotion;
    bool       m_motionBlur;
    U32        m_motionSeed;
    F32        m_shutterOpen, m_shutterClose;
    RayGen     m_raygen;
    F32        m_cameraFar;
    RayBuffer  m_primaryRays, m_secondaryRays;
    Buffer     m_primaryIDs, m_secondaryIDs;             // S32 per slot: the instance of the hit
    Buffer     m_primaryResolved, m_primaryNormals, m_secondaryResolved;
    Buffer     m_primaryTimes, m_secondaryTimes;         // setMotionBlur: F32 per slot
    bool       m_newBatch;
    RayBuffer* m_batchRays;
    Buffer*    m_batchResolved;
    S32        m_batchStart;
};

}  // namespace FW
