// InstancedRenderer.cpp -- Renderer's batching over a CudaInstancedBVH: every traced batch goes through ntr_instanced_hit_attributes
// before ntr_raygen_ao_normals, ntr_count_hits or ntr_reconstruct sees it (see the header).  Under setMotionBlur every batch has a
// time per ray: the trace and ntr_instanced_hit_attributes_motion read the same buffer; over deforming BLASes (setDeformGeometry) the
// attributes are ntr_instanced_hit_attributes_deform's, which poses the hit triangle at that time too.
#include "InstancedRenderer.hpp"

namespace FW {

InstancedRenderer::InstancedRenderer(CudaInstancedBVH& bvh)
    : m_bvh(bvh), m_triVtxIndex(NULL), m_vtxPos(NULL), m_vtxPos1(NULL), m_numVerts(0), m_rayType(RayType_Primary), m_aoRadius(1.0f), m_numSamples(32),
      m_primaryMask(0xFFFFFFFFu), m_secondaryMask(0xFFFFFFFFu), m_wide(false), m_fast(false), m_wideFast(false), m_wideMotion(false),
      m_motionBlur(false), m_motionSeed(0), m_shutterOpen(0.0f), m_shutterClose(1.0f),
      m_raygen(1 << 20), m_cameraFar(0.0f), m_newBatch(true), m_batchRays(NULL), m_batchResolved(NULL), m_batchStart(0)
{
}

void InstancedRenderer::setGeometry(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos)
{
    if (triVtxIndex.getSize() < (S64)(3 * sizeof(S32)) || numVerts < 1 || vtxPos.getSize() < (S64)numVerts * (S64)(3 * sizeof(F32)))
        fail("InstancedRenderer::setGeometry: bad mesh buffers");
    m_triVtxIndex = &triVtxIndex;
    m_vtxPos = &vtxPos;
    m_numVerts = numVerts;
}

void InstancedRenderer::setDeformGeometry(Buffer& vtxPos1)
{
    if (m_numVerts < 1) fail("InstancedRenderer::setDeformGeometry: no geometry: call setGeometry() first");
    if (vtxPos1.getSize() < (S64)m_numVerts * (S64)(3 * sizeof(F32)))
        fail("InstancedRenderer::setDeformGeometry: the buffer holds fewer than %d vertices (setGeometry's numVerts)", m_numVerts);
    m_vtxPos1 = &vtxPos1;
}

void InstancedRenderer::setParams(RayType rayType, F32 aoRadius, S32 numSamples)
{
    if (rayType < RayType_Primary || rayType >= RayType_Max || numSamples < 1) fail("InstancedRenderer::setParams: bad ray type or sample count");
    m_rayType = rayType;
    m_aoRadius = aoRadius;
    m_numSamples = numSamples;
}

void InstancedRenderer::setRayMasks(U32 primaryMask, U32 secondaryMask)
{
    m_primaryMask = primaryMask;
    m_secondaryMask = secondaryMask;
}

void InstancedRenderer::setMotionBlur(bool on, U32 seed, F32 open, F32 close)
{
    if (!(open >= 0.0f && open <= close && close <= 1.0f)) fail("InstancedRenderer::setMotionBlur: the shutter must be 0 <= open <= close <= 1");
    m_motionBlur = on;
    m_motionSeed = seed;
    m_shutterOpen = open;
    m_shutterClose = close;
}

F32 InstancedRenderer::trace(RayBuffer& rays, Buffer& instanceIDs, Buffer& times, U32 rayMask)
{
    struct Restore {   // the caller's flags and times come back on every path: traceBatch fails by throwing
        CudaInstancedBVH& bvh;
        bool was, wasFast, wasWideFast, wasWideMotion;
        Buffer* wasTimes;
        ~Restore()
        {
            bvh.setTraceWide(was); bvh.setTraceFast(wasFast); bvh.setTraceWideFast(wasWideFast); bvh.setTraceWideMotion(wasWideMotion);
            bvh.setRayTimes(wasTimes);
        }
    } restore = {m_bvh, m_bvh.getTraceWide(), m_bvh.getTraceFast(), m_bvh.getTraceWideFast(), m_bvh.getTraceWideMotion(), m_bvh.getRayTimes()};
    if (m_motionBlur) m_bvh.setRayTimes(&times);
    m_bvh.setTraceWide(m_wide);
    m_bvh.setTraceWideMotion(m_wideMotion || restore.wasWideMotion);
    m_bvh.setTraceFast(m_fast || restore.wasFast);
    m_bvh.setTraceWideFast(m_wideFast || restore.wasWideFast);
    return m_bvh.traceBatch(rays, instanceIDs, rayMask);
}

// the batch's records with pool triangle ids and, for a batch that secondary rays start from, the world-space normals
void InstancedRenderer::resolve(RayBuffer& rays, Buffer& instanceIDs, Buffer& times, Buffer& resolved, Buffer* normals)
{
    const S32 n = rays.getSize();
    resolved.resizeDiscard((S64)n * sizeof(NtrRayResult));
    if (normals) normals->resizeDiscard((S64)n * (S64)(4 * sizeof(F32)));
    if (!n) return;
    NtrInstancedGeometry g;
    g.numInstances = m_bvh.getNumInstances() + (m_bvh.hasWorld() ? 1 : 0);   // a world's hits carry instance id N: its record lies there
    g.numBlas = m_bvh.getNumBLAS();
    g.numTrisTotal = (int32_t)(m_triVtxIndex->getSize() / (S64)(3 * sizeof(S32)));
    g.numVerts = m_numVerts;
    g.d_instances = (const NtrInstance*)m_bvh.getInstanceBuffer().getCudaPtr();
    g.d_blasTris = (const NtrBlasTris*)m_bvh.getBLASTrisBuffer().getCudaPtr();
    g.d_triVtxIndex = (const int32_t*)m_triVtxIndex->getCudaPtr();
    g.d_vtxPos = (const float*)m_vtxPos->getCudaPtr();
    int rc;
    if (m_motionBlur) {   // the key buffer and the times the trace has just read: the normal of the pose the ray hit
        if (times.getSize() < (S64)n * (S64)sizeof(F32)) fail("InstancedRenderer: the batch has no times");
        NtrInstanceMotion motion;
        motion.d_motionKeys = m_bvh.getMotionKeyBuffer().getCudaPtr();
        motion.motionKeysBytes = m_bvh.getMotionKeyBuffer().getSize();
        motion.d_rayTimes = (const float*)times.getCudaPtr();
        motion.time = 0.0f;
        motion.pad = 0.0f;
        NtrInstancedDeformGeometry deform;   // over deforming BLASes the triangle is posed too: the one the trace tested
        const bool deforming = m_bvh.hasDeform();
        if (deforming) {
            if (!m_vtxPos1 || m_vtxPos1->getSize() < (S64)m_numVerts * (S64)(3 * sizeof(F32))) fail("InstancedRenderer: no closing vertices");
            deform.d_vtxPos1 = (const float*)m_vtxPos1->getCudaPtr();
            deform.d_blasDeforming = (const uint32_t*)m_bvh.getBLASDeformingBuffer().getCudaPtr();
        }
        rc = ntr_instanced_hit_attributes_deform(n, (const NtrRayResult*)rays.getResultBuffer().getCudaPtr(), (const int32_t*)instanceIDs.getCudaPtr(),
                                                 &g, &motion, deforming ? &deform : NULL /* ntr_instanced_hit_attributes_motion */,
                                                 (NtrRayResult*)resolved.getMutableCudaPtr(), normals ? (float*)normals->getMutableCudaPtr() : NULL,
                                                 NULL);
    } else
        rc = ntr_instanced_hit_attributes(n, (const NtrRayResult*)rays.getResultBuffer().getCudaPtr(), (const int32_t*)instanceIDs.getCudaPtr(), &g,
                                          (NtrRayResult*)resolved.getMutableCudaPtr(), normals ? (float*)normals->getMutableCudaPtr() : NULL, NULL);
    if (rc != NTR_OK) fail("InstancedRenderer: %s", ntr_last_error());
}

void InstancedRenderer::beginFrame(const CameraView& camera, S32 w, S32 h)
{
    if (m_motionBlur && m_bvh.hasDeform() && (!m_vtxPos1 || m_vtxPos1->getSize() < (S64)m_numVerts * (S64)(3 * sizeof(F32))))
        fail("InstancedRenderer: setMotionBlur is not combinable with deforming BLASes (CudaInstancedBVH::refitBLASesMotion) without their closing "
             "vertices: the normals of their hits would be key 0's; call setDeformGeometry with the closing vertices refitBLASesMotion was given, "
             "clearDeform() or setMotionBlur(false)");
    if (m_motionBlur && !m_bvh.hasMotion() && !m_bvh.hasDeform())
        fail("InstancedRenderer: setMotionBlur is on and the CudaInstancedBVH has no motion key: call setMotionKey (or setMotionKeyDevice) with the "
             "shutter's closing transforms, or setMotionBlur(false)");
    if (!m_triVtxIndex)
        fail("InstancedRenderer: no geometry: call setGeometry() with the index and vertex buffers CudaInstancedBVH::buildBLASes was given");
    const S32 meshless = m_bvh.getFirstMeshlessBLAS();
    if (meshless >= 0)
        fail("InstancedRenderer: BLAS %d came through addBLAS and has no mesh here, so its hits cannot be resolved: build the pool with "
             "CudaInstancedBVH::buildBLASes", meshless);
    if (!m_bvh.isBuilt())
        fail("InstancedRenderer: the TLAS is not current: call build() or refit() on the CudaInstancedBVH (after buildBLASes / refitBLASes and "
             "setInstances) before beginFrame");
    if (w < 1 || h < 1) fail("InstancedRenderer::beginFrame: bad frame size");
    if (m_wide && !m_bvh.isWide()) m_bvh.widen();   // after each build() / refit() of the frame loop
    m_raygen.primary(m_primaryRays, camera.position, camera.nscreenToWorld, w, h, camera.cameraFar, 0);
    if (m_motionBlur) m_raygen.primaryTimes(m_primaryTimes, m_primaryRays, m_motionSeed, m_shutterOpen, m_shutterClose);
    if (m_rayType != RayType_Primary) {   // Renderer.cpp:482-488
        trace(m_primaryRays, m_primaryIDs, m_primaryTimes, m_primaryMask);
        resolve(m_primaryRays, m_primaryIDs, m_primaryTimes, m_primaryResolved, &m_primaryNormals);
    }
    m_cameraFar = camera.cameraFar;
    m_newBatch = true;
    m_batchRays = NULL;
    m_batchResolved = NULL;
    m_batchStart = 0;
}

bool InstancedRenderer::nextBatch(void)
{
    if (m_batchRays) m_batchStart += m_batchRays->getSize();
    m_batchRays = NULL;
    m_batchResolved = NULL;
    switch (m_rayType) {
    case RayType_Primary:
        if (!m_newBatch) return false;
        m_newBatch = false;
        m_batchRays = &m_primaryRays;
        m_batchResolved = &m_primaryResolved;
        break;
    case RayType_AO:
        if (!m_raygen.aoNormals(m_secondaryRays, m_primaryRays, m_primaryNormals, m_numSamples, m_aoRadius, m_newBatch, 0)) return false;
        m_batchRays = &m_secondaryRays;
        m_batchResolved = &m_secondaryResolved;
        break;
    case RayType_Diffuse:
        if (!m_raygen.aoNormals(m_secondaryRays, m_primaryRays, m_primaryNormals, m_numSamples, m_cameraFar, m_newBatch, 0)) return false;
        m_secondaryRays.setNeedClosestHit(true);
        m_batchRays = &m_secondaryRays;
        m_batchResolved = &m_secondaryResolved;
        break;
    default:
        return false;
    }
    // a secondary ray inherits its primary ray's time: input slot m_batchStart / m_numSamples + k made slots k * m_numSamples + j
    if (m_motionBlur && m_batchRays == &m_secondaryRays)
        m_raygen.secondaryTimes(m_secondaryTimes, m_primaryTimes, m_batchStart / m_numSamples, m_secondaryRays.getSize() / m_numSamples, m_numSamples);
    return true;
}

F32 InstancedRenderer::traceBatch(void)
{
    if (!m_batchRays) fail("InstancedRenderer::traceBatch: no batch");
    const bool primary = m_batchRays == &m_primaryRays;
    Buffer& ids = primary ? m_primaryIDs : m_secondaryIDs;
    Buffer& times = primary ? m_primaryTimes : m_secondaryTimes;
    const F32 sec = trace(*m_batchRays, ids, times, primary ? m_primaryMask : m_secondaryMask);
    resolve(*m_batchRays, ids, times, *m_batchResolved, primary ? &m_primaryNormals : NULL);
    return sec;
}

void InstancedRenderer::updateResult(Buffer& pixels, Buffer& triMaterialColor, Buffer& triShadedColor)
{
    if (!m_batchRays) fail("InstancedRenderer::updateResult: no batch");
    if (m_batchResolved->getSize() != (S64)m_batchRays->getSize() * (S64)sizeof(NtrRayResult) ||
        m_primaryResolved.getSize() != (S64)m_primaryRays.getSize() * (S64)sizeof(NtrRayResult))
        fail("InstancedRenderer::updateResult: the batch has not been traced: call traceBatch() first");
    const int perPrimary = (m_rayType == RayType_Primary) ? 1 : m_numSamples;
    const int rc = ntr_reconstruct((int)m_rayType, perPrimary, m_batchStart / perPrimary, m_batchRays->getSize() / perPrimary,
                                   (const int32_t*)m_primaryRays.getSlotToIDBuffer().getCudaPtr(),
                                   (const NtrRayResult*)m_primaryResolved.getCudaPtr(),
                                   (const int32_t*)m_batchRays->getIDToSlotBuffer().getCudaPtr(),
                                   (const NtrRayResult*)m_batchResolved->getCudaPtr(), (const uint32_t*)triMaterialColor.getCudaPtr(),
                                   (const uint32_t*)triShadedColor.getCudaPtr(), (uint32_t*)pixels.getMutableCudaPtr(), NULL);
    if (rc != NTR_OK) fail("InstancedRenderer::updateResult: %s", ntr_last_error());
    if (ntr_stream_synchronize(NULL) != NTR_OK) fail("InstancedRenderer::updateResult: %s", ntr_last_error());
}

int InstancedRenderer::getTotalNumRays(void)
{
    if (m_rayType == RayType_Primary) return m_primaryRays.getSize();
    int32_t hits = 0;
    if (ntr_count_hits((const NtrRayResult*)m_primaryResolved.getCudaPtr(), m_primaryRays.getSize(), &hits, NULL) != NTR_OK)
        fail("InstancedRenderer: %s", ntr_last_error());
    return hits * m_numSamples;
}

}  // namespace FW
