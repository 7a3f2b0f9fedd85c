// CudaInstancedBVH.cpp -- a pool of BLASes, instances and their top-level tree over ntr_tlas_build / ntr_tlas_refit / ntr_trace_instanced
// and ntr_trace_instanced_masked, and the wide path over ntr_pool_widen_batch (ntr_pool_widen for one BLAS) / ntr_tlas_widen / ntr_pool_wide_refit / ntr_tlas_wide_refit /
// ntr_trace_instanced_wide, and a static world over ntr_trace_bvh / ntr_trace_instanced_seeded / ntr_trace_instanced_wide_seeded (see the
// header), and the FAST path over ntr_instanced_validate / ntr_trace_instanced_fast, and over the wide trees
// ntr_instanced_wide_validate / ntr_trace_instanced_wide_fast, and motion blur over ntr_tlas_motion_refit / ntr_trace_instanced_motion.
#include "CudaInstancedBVH.hpp"

#include <cstring>

namespace FW {

CudaInstancedBVH::CudaInstancedBVH(void) : m_blasTrisCurrent(false), m_numInstances(0), m_built(false), m_topology(false),
                                           m_wideTopology(false), m_widePool(false), m_wideTlas(false), m_traceWide(false), m_world(-1),
                                           m_traceFast(false), m_fastStale(true), m_fastValidations(0), m_traceWideFast(false),
                                           m_wideFastStale(true), m_wideFastValidations(0), m_rayTimes(NULL), m_time(0.0f),
                                           m_hasMotion(false), m_motionStale(true), m_motionRefits(0),
                                           m_traceWideMotion(false), m_wideMotionCurrent(false), m_motionWideRefits(0)
{
    std::memset(&m_motionRefitResult, 0, sizeof(m_motionRefitResult));
    std::memset(&m_motionWideRefitResult, 0, sizeof(m_motionWideRefitResult));
    std::memset(&m_widePoolResult, 0, sizeof(m_widePoolResult));
    std::memset(&m_wideResult, 0, sizeof(m_wideResult));
    std::memset(&m_wideBlasRefitResult, 0, sizeof(m_wideBlasRefitResult));
    std::memset(&m_wideTlasRefitResult, 0, sizeof(m_wideTlasRefitResult));
    std::memset(&m_result, 0, sizeof(m_result));
    std::memset(&m_blasResult, 0, sizeof(m_blasResult));
    std::memset(&m_refitResult, 0, sizeof(m_refitResult));
    std::memset(&m_optimizeResult, 0, sizeof(m_optimizeResult));
    std::memset(&m_tlasRefitResult, 0, sizeof(m_tlasRefitResult));
    std::memset(&m_instancesUpdateResult, 0, sizeof(m_instancesUpdateResult));
}

S32 CudaInstancedBVH::addBLAS(CudaBVH& bvh)
{
    if (bvh.getLayout() != BVHLayout_Compact) fail("CudaInstancedBVH: Incorrect BVH layout!");
    Buffer &nodes = bvh.getNodeBuffer(), &woop = bvh.getTriWoopBuffer(), &index = bvh.getTriIndexBuffer();
    if (nodes.getSize() < 64 || nodes.getSize() % 64 || woop.getSize() < 16 || woop.getSize() % 16 || index.getSize() * 4 != woop.getSize())
        fail("CudaInstancedBVH: not a Compact tree's buffers");
    // the pool's sizes are multiples of 64 and 16 already: every range was one
    NtrBlasRange r;
    r.nodesOffset = m_poolNodes.getSize();
    r.nodesBytes = nodes.getSize();
    r.triWoopOffset = m_poolTriWoop.getSize();
    r.triWoopBytes = woop.getSize();
    if (r.nodesOffset + r.nodesBytes > 0xFFFFFF00ll || r.triWoopOffset + r.triWoopBytes > 0xFFFFFF00ll) fail("CudaInstancedBVH: the pool is full");
    m_poolNodes.resize(r.nodesOffset + r.nodesBytes);
    m_poolTriWoop.resize(r.triWoopOffset + r.triWoopBytes);
    m_poolTriIndex.resize((r.triWoopOffset + r.triWoopBytes) / 4);
    m_poolNodes.setRange(r.nodesOffset, nodes, 0, r.nodesBytes);
    m_poolTriWoop.setRange(r.triWoopOffset, woop, 0, r.triWoopBytes);
    m_poolTriIndex.setRange(r.triWoopOffset / 4, index, 0, r.triWoopBytes / 4);
    m_ranges.push_back(r);
    const Mesh none = {0, 0};
    m_meshes.push_back(none);
    m_built = m_topology = m_wideTopology = m_blasTrisCurrent = false;
    m_widePool = m_wideTlas = false;
    m_fastStale = m_wideFastStale = true;
    return (S32)m_ranges.size() - 1;
}

void CudaInstancedBVH::buildBLASes(S32 numMeshes, const NtrPlocBatchMesh* meshes, Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, S32 radius)
{
    if (numMeshes < 1 || !meshes) fail("CudaInstancedBVH: no meshes");
    std::vector<NtrBlasRange> ranges((size_t)numMeshes);
    int64_t capN, capW, capI;
    if (ntr_ploc_batch_capacity(numMeshes, meshes, ranges.data(), &capN, &capW, &capI) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    const S64 numTris = triVtxIndex.getSize() / (S64)(3 * sizeof(S32));
    if (numTris < 1 || numTris >= (1ll << 28) || vtxPos.getSize() < (S64)numVerts * (S64)(3 * sizeof(F32))) fail("CudaInstancedBVH: bad mesh buffers");
    m_ranges.clear();
    m_meshes.clear();
    clearWorld();                                    // the pool is replaced: whatever BLAS the world named is gone
    m_built = m_topology = m_wideTopology = m_blasTrisCurrent = false;
    m_widePool = m_wideTlas = false;
    m_fastStale = m_wideFastStale = true;
    m_poolNodes.resizeDiscard(capN);
    m_poolTriWoop.resizeDiscard(capW);
    m_poolTriIndex.resizeDiscard(capI);
    const int rc = ntr_ploc_build_batch(numMeshes, meshes, (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(), numVerts,
                                        (const float*)vtxPos.getCudaPtr(), radius, m_poolNodes.getMutableCudaPtr(), capN,
                                        m_poolTriWoop.getMutableCudaPtr(), capW, (int32_t*)m_poolTriIndex.getMutableCudaPtr(), capI, ranges.data(),
                                        NULL, &m_blasResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_ranges.swap(ranges);
    m_meshes.resize((size_t)numMeshes);
    for (S32 k = 0; k < numMeshes; k++) {
        m_meshes[k].firstTri = meshes[k].firstTri;
        m_meshes[k].numTris = meshes[k].numTris;
    }
}

Buffer& CudaInstancedBVH::getBLASTrisBuffer(void)
{
    if (!m_blasTrisCurrent) {
        static_assert(sizeof(Mesh) == sizeof(NtrBlasTris), "Mesh is NtrBlasTris");
        m_blasTris.resizeDiscard((S64)m_meshes.size() * sizeof(NtrBlasTris));
        if (!m_meshes.empty()) m_blasTris.set(m_meshes.data(), (S64)m_meshes.size() * sizeof(NtrBlasTris));
        m_blasTrisCurrent = true;
    }
    return m_blasTris;
}

S32 CudaInstancedBVH::getFirstMeshlessBLAS(void) const
{
    for (size_t k = 0; k < m_meshes.size(); k++)
        if (m_meshes[k].numTris < 1) return (S32)k;
    return -1;
}

void CudaInstancedBVH::refitBLASes(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas, S32 num, F32 epsilon)
{
    if (m_ranges.empty()) fail("CudaInstancedBVH: no BLASes to refit (call buildBLASes first)");
    if (!blas) num = (S32)m_ranges.size();
    if (num < 1) fail("CudaInstancedBVH: no BLASes selected");
    const S64 numTris = triVtxIndex.getSize() / (S64)(3 * sizeof(S32));
    if (numTris < 1 || numTris >= (1ll << 28) || vtxPos.getSize() < (S64)numVerts * (S64)(3 * sizeof(F32))) fail("CudaInstancedBVH: bad mesh buffers");
    std::vector<NtrRefitBatchEntry> entries((size_t)num);
    for (S32 i = 0; i < num; i++) {
        const S32 b = blas ? blas[i] : i;
        if (b < 0 || b >= (S32)m_ranges.size()) fail("CudaInstancedBVH: BLAS index %d outside [0, %d)", b, (S32)m_ranges.size());
        if (m_meshes[b].numTris < 1) fail("CudaInstancedBVH: BLAS %d came through addBLAS and has no mesh here: refit its CudaBVH and add it again", b);
        NtrRefitBatchEntry& e = entries[i];
        e.range = m_ranges[b];
        e.firstTri = m_meshes[b].firstTri;
        e.numTris = m_meshes[b].numTris;
        e.epsilon = epsilon;
        e.pad = 0;
    }
    m_built = false;
    m_widePool = m_wideTlas = false;             // this method refits the binary pool only: widen() again, or call refitBLASesWide
    m_fastStale = m_wideFastStale = true;
    const int rc = ntr_bvh_refit_batch(num, entries.data(), m_poolNodes.getMutableCudaPtr(), m_poolNodes.getSize(),
                                       m_poolTriWoop.getMutableCudaPtr(), m_poolTriWoop.getSize(), (const int32_t*)m_poolTriIndex.getCudaPtr(),
                                       (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(), numVerts, (const float*)vtxPos.getCudaPtr(),
                                       NULL, &m_refitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
}

void CudaInstancedBVH::selectRanges(const S32* blas, S32 num, std::vector<NtrBlasRange>& out, const char* what) const
{
    if (m_ranges.empty()) fail("CudaInstancedBVH: no BLASes to %s", what);
    if (!blas) num = (S32)m_ranges.size();
    if (num < 1) fail("CudaInstancedBVH: no BLASes selected");
    out.resize((size_t)num);
    for (S32 i = 0; i < num; i++) {
        const S32 b = blas ? blas[i] : i;
        if (b < 0 || b >= (S32)m_ranges.size()) fail("CudaInstancedBVH: BLAS index %d outside [0, %d)", b, (S32)m_ranges.size());
        out[(size_t)i] = m_ranges[(size_t)b];
    }
}

void CudaInstancedBVH::optimizeBLASes(const S32* blas, S32 num, S32 passes)
{
    std::vector<NtrBlasRange> sel;
    selectRanges(blas, num, sel, "optimise");
    m_widePool = m_wideTlas = false;             // the binary pool's topology changes: widen() again (m_built stays, see the header)
    m_fastStale = m_wideFastStale = true;                          // node boxes are rewritten
    const int rc = ntr_bvh_optimize_batch((int32_t)sel.size(), sel.data(), m_poolNodes.getMutableCudaPtr(), m_poolNodes.getSize(), passes, NULL,
                                          &m_optimizeResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
}

void CudaInstancedBVH::measureBLASes(std::vector<NtrBvhSahResult>& out, const S32* blas, S32 num)
{
    std::vector<NtrBlasRange> sel;
    selectRanges(blas, num, sel, "measure");
    out.assign(sel.size(), NtrBvhSahResult());
    const int rc = ntr_bvh_sah_cost_batch((int32_t)sel.size(), sel.data(), m_poolNodes.getCudaPtr(), m_poolNodes.getSize(),
                                          m_poolTriWoop.getCudaPtr(), m_poolTriWoop.getSize(), out.data(), NULL, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
}

void CudaInstancedBVH::setInstances(S32 num, const F32* objectToWorld, const S32* blas)
{
    if (num < 1 || !objectToWorld || !blas) fail("CudaInstancedBVH: no instances");
    const S32 total = num + (m_world >= 0 ? 1 : 0);  // a world's record lies behind the instances'
    m_instances.resizeDiscard((S64)total * sizeof(NtrInstance));
    NtrInstance* inst = (NtrInstance*)m_instances.getMutablePtrDiscard();
    std::memset(inst, 0, (size_t)total * sizeof(NtrInstance));
    for (S32 i = 0; i < num; i++) {
        std::memcpy(inst[i].objectToWorld, objectToWorld + 12 * (size_t)i, sizeof(inst[i].objectToWorld));
        if (ntr_instance_invert(inst[i].objectToWorld, inst[i].worldToObject) != NTR_OK) fail("CudaInstancedBVH: instance %d: %s", i, ntr_last_error());
        inst[i].blas = blas[i];
    }
    if (num != m_numInstances) {
        m_topology = m_wideTopology = false;         // an unchanged count keeps the TLAS's topology for refit() ...
        m_instanceMasks.resizeDiscard(0);            // ... and the instance masks: with another count they would name other instances
        clearMotion();                               // ... and key 1 of the motion
    }
    m_numInstances = num;
    m_built = false;
    m_motionStale = true;
    writeWorldRecord();
}

void CudaInstancedBVH::setInstancesDevice(S32 numNodes, Buffer& nodeLocal, Buffer* nodeParent, S32 num, Buffer* instanceNode, Buffer& blas, bool check)
{
    if (num < 1 || numNodes < 1) fail("CudaInstancedBVH: no instances");
    if (!instanceNode && numNodes < num) fail("CudaInstancedBVH: without instanceNode instance i uses node i: %d nodes for %d instances", numNodes, num);
    if (nodeLocal.getSize() < (S64)numNodes * 48 || (nodeParent && nodeParent->getSize() < (S64)numNodes * 4) ||
        (instanceNode && instanceNode->getSize() < (S64)num * 4) || blas.getSize() < (S64)num * 4)
        fail("CudaInstancedBVH: a transform or index buffer is smaller than its count");
    const S32 total = num + (m_world >= 0 ? 1 : 0);  // a world's record lies behind the instances'
    m_instances.resizeDiscard((S64)total * sizeof(NtrInstance));
    m_instanceStatus.resizeDiscard(4 * sizeof(U32));
    std::memset(&m_instancesUpdateResult, 0, sizeof(m_instancesUpdateResult));
    const int rc = ntr_instances_update(numNodes, (const float*)nodeLocal.getCudaPtr(), nodeParent ? (const int32_t*)nodeParent->getCudaPtr() : NULL,
                                        num, instanceNode ? (const int32_t*)instanceNode->getCudaPtr() : NULL, (const int32_t*)blas.getCudaPtr(),
                                        (NtrInstance*)m_instances.getMutableCudaPtrDiscard(), (uint32_t*)m_instanceStatus.getMutableCudaPtrDiscard(),
                                        check ? &m_instancesUpdateResult : NULL, NULL);
    // the instance array has been rewritten whatever the status says: the state follows before a bad instance is reported
    if (num != m_numInstances) {
        m_topology = m_wideTopology = false;         // as setInstances: an unchanged count keeps the topology, the masks and key 1
        m_instanceMasks.resizeDiscard(0);
        clearMotion();
    }
    m_numInstances = num;
    m_built = false;
    m_motionStale = true;
    const std::string message = rc != NTR_OK ? ntr_last_error() : "";
    if (rc == NTR_OK || m_instancesUpdateResult.statusBits != 0) writeWorldRecord();   // (the kernel ran: the array is the scene's)
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", message.c_str());
}

void CudaInstancedBVH::getInstanceStatus(U32 out[4])
{
    if (m_instanceStatus.getSize() != 4 * (S64)sizeof(U32)) fail("CudaInstancedBVH: no instance status: call setInstancesDevice first");
    uint32_t st[4];
    if (ntr_instances_status_read((const uint32_t*)m_instanceStatus.getCudaPtr(), st, NULL) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    for (int k = 0; k < 4; k++) out[k] = st[k];
}

void CudaInstancedBVH::writeWorldRecord(void)
{
    if (m_world < 0) return;
    NtrInstance w;
    std::memset(&w, 0, sizeof(w));
    w.objectToWorld[0] = w.objectToWorld[5] = w.objectToWorld[10] = 1.0f;   // identity both ways: the world's object space is world space
    w.worldToObject[0] = w.worldToObject[5] = w.worldToObject[10] = 1.0f;
    w.blas = m_world;
    m_instances.resize((S64)(m_numInstances + 1) * sizeof(NtrInstance));   // keeps the instances' records
    m_instances.setRange((S64)m_numInstances * sizeof(NtrInstance), &w, sizeof(w));
}

void CudaInstancedBVH::setWorld(S32 blas, const char* kernelName)
{
    if (blas < 0 || blas >= (S32)m_ranges.size()) fail("CudaInstancedBVH::setWorld: BLAS index %d outside [0, %d)", blas, (S32)m_ranges.size());
    if (!kernelName || !kernelName[0]) fail("CudaInstancedBVH::setWorld: no kernel name");
    m_world = blas;
    m_worldKernel = kernelName;
    m_fastStale = m_wideFastStale = true;
    writeWorldRecord();                              // the TLAS never sees the world: m_built stays
}

void CudaInstancedBVH::clearWorld(void)
{
    if (m_world < 0) return;
    m_world = -1;
    m_fastStale = m_wideFastStale = true;
    m_instances.resize((S64)m_numInstances * sizeof(NtrInstance));
}

void CudaInstancedBVH::setInstanceMasks(const U32* masks)
{
    if (m_numInstances < 1) fail("CudaInstancedBVH: no instances to mask (call setInstances first)");
    if (!masks) { m_instanceMasks.resizeDiscard(0); return; }
    m_instanceMasks.resizeDiscard((S64)m_numInstances * sizeof(U32));
    m_instanceMasks.set(masks, (S64)m_numInstances * sizeof(U32));   // the TLAS knows nothing of visibility: m_built stays
}

void CudaInstancedBVH::build(S32 radius)
{
    if (m_ranges.empty() || m_numInstances < 1) fail("CudaInstancedBVH: nothing to build");
    int64_t capN, capR;
    if (ntr_tlas_capacity(m_numInstances, &capN, &capR) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_built = m_topology = m_wideTopology = false;
    m_wideTlas = false;
    m_fastStale = m_wideFastStale = true;
    m_motionStale = true;                        // the build writes records without moving flags and boxes of key 0 alone
    m_tlasNodes.resizeDiscard(capN);
    m_records.resizeDiscard(capR);
    const int rc = ntr_tlas_build(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                  m_poolNodes.getCudaPtr(), m_poolNodes.getSize(), radius, m_tlasNodes.getMutableCudaPtr(), capN,
                                  m_records.getMutableCudaPtr(), capR, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    if (m_result.nodesBytes) m_tlasNodes.resize(m_result.nodesBytes);   // (N == 1 has no node: the buffer keeps its one unused slot)
    m_built = m_topology = true;
}

void CudaInstancedBVH::refit(void)
{
    if (!m_topology || m_numInstances < 1)
        fail("CudaInstancedBVH: no TLAS to refit: call build() first, and again after the instance count or the BLASes have changed");
    m_wideTlas = false;
    m_fastStale = m_wideFastStale = true;
    m_motionStale = true;                        // as build(): the moving flags are cleared, the scene is frozen at key 0
    const int rc = ntr_tlas_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                  m_poolNodes.getCudaPtr(), m_poolNodes.getSize(), m_result.nodesBytes ? m_tlasNodes.getMutableCudaPtr() : NULL,
                                  m_result.nodesBytes, m_result.rootLink, m_records.getMutableCudaPtr(), m_records.getSize(), NULL,
                                  &m_tlasRefitResult, NULL);
    if (rc != NTR_OK) {
        m_built = false;                         // a part of the tree kept stale boxes
        fail("CudaInstancedBVH: %s", ntr_last_error());
    }
    for (int a = 0; a < 3; a++) {
        m_result.sceneMin[a] = m_tlasRefitResult.sceneMin[a];
        m_result.sceneMax[a] = m_tlasRefitResult.sceneMax[a];
    }
    m_built = true;
}

void CudaInstancedBVH::setMotionKey(S32 num, const F32* objectToWorld1)
{
    if (num < 1 || !objectToWorld1) fail("CudaInstancedBVH: no motion key");
    if (num != m_numInstances) fail("CudaInstancedBVH: the motion key names %d instances, setInstances %d", num, m_numInstances);
    m_instances1.resizeDiscard((S64)num * sizeof(NtrInstance));
    NtrInstance* inst = (NtrInstance*)m_instances1.getMutablePtrDiscard();
    std::memset(inst, 0, (size_t)num * sizeof(NtrInstance));   // of key 1 only objectToWorld is read
    for (S32 i = 0; i < num; i++) std::memcpy(inst[i].objectToWorld, objectToWorld1 + 12 * (size_t)i, sizeof(inst[i].objectToWorld));
    m_hasMotion = m_motionStale = true;
}

void CudaInstancedBVH::setMotionKeyDevice(S32 num, Buffer& instances1)
{
    if (num < 1) fail("CudaInstancedBVH: no motion key");
    if (num != m_numInstances) fail("CudaInstancedBVH: the motion key names %d instances, setInstances %d", num, m_numInstances);
    if (instances1.getSize() < (S64)num * (S64)sizeof(NtrInstance)) fail("CudaInstancedBVH: the motion key's buffer is smaller than its count");
    m_instances1.resizeDiscard((S64)num * sizeof(NtrInstance));
    m_instances1.setRange(0, instances1, 0, (S64)num * sizeof(NtrInstance));
    m_hasMotion = m_motionStale = true;
}

void CudaInstancedBVH::clearMotion(void)
{
    // the records keep their moving flags, which only the motion trace reads, and the boxes still bound the sweep: m_built stays
    m_hasMotion = false;
    m_motionStale = true;
    m_instances1.resizeDiscard(0);
}

void CudaInstancedBVH::refitMotion(void)
{
    if (!m_hasMotion) fail("CudaInstancedBVH: no motion key: call setMotionKey first");
    if (!m_built) fail("CudaInstancedBVH: No TLAS!");
    m_wideTlas = false;                          // the binary boxes become the swept ones: as refit()
    m_fastStale = m_wideFastStale = true;
    m_motionKeys.resizeDiscard((S64)m_numInstances * 128);
    const int rc = ntr_tlas_motion_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (const NtrInstance*)m_instances1.getCudaPtr(),
                                         (int32_t)m_ranges.size(), m_ranges.data(), m_poolNodes.getCudaPtr(), m_poolNodes.getSize(),
                                         m_result.nodesBytes ? m_tlasNodes.getMutableCudaPtr() : NULL, m_result.nodesBytes, m_result.rootLink,
                                         m_records.getMutableCudaPtr(), m_records.getSize(), m_motionKeys.getMutableCudaPtrDiscard(),
                                         m_motionKeys.getSize(), NULL, &m_motionRefitResult, NULL);
    m_motionRefits++;
    if (rc != NTR_OK) {
        m_built = false;                         // a part of the tree kept stale boxes
        fail("CudaInstancedBVH: %s", ntr_last_error());
    }
    for (int a = 0; a < 3; a++) {
        m_result.sceneMin[a] = m_motionRefitResult.refit.sceneMin[a];
        m_result.sceneMax[a] = m_motionRefitResult.refit.sceneMax[a];
    }
    m_motionStale = false;
}

void CudaInstancedBVH::widen(void)
{
    if (!m_built) fail("CudaInstancedBVH: no TLAS to widen: call build() or refit() first");
    const int32_t numBlas = (int32_t)m_ranges.size();
    m_wideFastStale = true;                      // wide boxes are written
    if (!m_widePool) {
        int64_t cap = 0;
        if (ntr_pool_widen_capacity(numBlas, m_ranges.data(), &cap) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_wideRanges.assign((size_t)numBlas, NtrWideBlasRange());
        m_widePoolNodes.resizeDiscard(cap);
        // the same bytes either way; the batched pass costs launches by the tallest BLAS, the loop by the number of BLASes
        const int rc = numBlas > 1 ? ntr_pool_widen_batch(numBlas, m_ranges.data(), m_poolNodes.getCudaPtr(), m_poolNodes.getSize(),
                                                          m_widePoolNodes.getMutableCudaPtr(), cap, m_wideRanges.data(), &m_widePoolResult, NULL)
                                   : ntr_pool_widen(numBlas, m_ranges.data(), m_poolNodes.getCudaPtr(), m_poolNodes.getSize(),
                                                    m_widePoolNodes.getMutableCudaPtr(), cap, m_wideRanges.data(), &m_widePoolResult, NULL);
        if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_widePool = true;
    }
    m_wideTlas = false;
    int64_t capT = 0;
    if (m_result.rootLink == 0 && ntr_bvh_widen_capacity(m_result.nodesBytes, &capT) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_wideTlasNodes.resizeDiscard(capT ? capT : 128);
    m_wideRecords.resizeDiscard((S64)m_numInstances * 64);
    const int rc = ntr_tlas_widen(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), m_result.rootLink == 0 ? m_tlasNodes.getCudaPtr() : NULL,
                                  m_result.nodesBytes, m_result.rootLink, numBlas, m_ranges.data(), m_wideRanges.data(),
                                  m_result.rootLink == 0 ? m_wideTlasNodes.getMutableCudaPtr() : NULL, capT, m_wideRecords.getMutableCudaPtr(),
                                  m_wideRecords.getSize(), &m_wideResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_wideTlas = m_wideTopology = true;
    m_wideMotionCurrent = false;                 // the wide records have no moving flags, the wide boxes are the binary tree's
}

void CudaInstancedBVH::refitBLASesWide(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas, S32 num, F32 epsilon)
{
    if (!m_widePool) fail("CudaInstancedBVH: no current wide pool to refit: call widen() first, and again after refitBLASes, buildBLASes or addBLAS");
    if (!blas) num = (S32)m_ranges.size();
    refitBLASes(triVtxIndex, numVerts, vtxPos, blas, num, epsilon);   // the binary pool stays current; the selection is checked there
    std::vector<NtrWideRefitEntry> entries((size_t)num);
    for (S32 i = 0; i < num; i++) {
        const S32 b = blas ? blas[i] : i;
        NtrWideRefitEntry& e = entries[i];
        e.wideNodesOffset = m_wideRanges[b].nodesOffset;
        e.wideNodesBytes = m_wideRanges[b].nodesBytes;
        e.triWoopOffset = m_ranges[b].triWoopOffset;
        e.triWoopBytes = m_ranges[b].triWoopBytes;
        e.firstTri = m_meshes[b].firstTri;
        e.numTris = m_meshes[b].numTris;
        e.epsilon = epsilon;
        e.pad = 0;
    }
    const S64 numTris = triVtxIndex.getSize() / (S64)(3 * sizeof(S32));
    const int rc = ntr_pool_wide_refit(num, entries.data(), m_widePoolNodes.getMutableCudaPtr(), m_widePoolResult.nodesBytes,
                                       m_poolTriWoop.getMutableCudaPtr(), m_poolTriWoop.getSize(), (const int32_t*)m_poolTriIndex.getCudaPtr(),
                                       (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(), numVerts, (const float*)vtxPos.getCudaPtr(),
                                       0 /* the binary refit has written the rows */, NULL, &m_wideBlasRefitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_widePool = true;                           // (refitBLASes dropped it: the wide boxes are the new ones again)
    m_wideFastStale = true;
}

void CudaInstancedBVH::refitWide(void)
{
    if (!m_topology || !m_wideTopology || m_numInstances < 1)
        fail("CudaInstancedBVH: no wide TLAS to refit: call build() and widen() first, and again after the instance count or the BLASes have changed");
    if (!m_widePool) fail("CudaInstancedBVH: the wide pool is not current: call refitBLASesWide() in place of refitBLASes(), or widen()");
    refit();                                     // the binary TLAS and records stay current
    const int rc = ntr_tlas_wide_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                       m_wideRanges.data(), m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                       m_wideResult.nodesBytes ? m_wideTlasNodes.getMutableCudaPtr() : NULL, m_wideResult.nodesBytes,
                                       m_result.rootLink, m_wideRecords.getMutableCudaPtr(), m_wideRecords.getSize(), NULL,
                                       &m_wideTlasRefitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_wideTlas = true;
    m_wideFastStale = true;
    m_wideMotionCurrent = false;                 // word 15 = 0 everywhere: the wide trees are frozen at key 0
}

void CudaInstancedBVH::refitMotionWide(void)
{
    if (!m_topology || !m_wideTopology || m_numInstances < 1)
        fail("CudaInstancedBVH: no wide TLAS for the motion refit: call build() and widen() first, and again after the instance count or the BLASes "
             "have changed");
    if (!m_widePool) fail("CudaInstancedBVH: the wide pool is not current: call refitBLASesWide() in place of refitBLASes(), or widen()");
    refitMotion();                               // the binary TLAS, its records and the motion keys stay current
    m_wideMotionCurrent = false;
    const int rc = ntr_tlas_wide_motion_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(),
                                              (const NtrInstance*)m_instances1.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                              m_wideRanges.data(), m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                              m_wideResult.nodesBytes ? m_wideTlasNodes.getMutableCudaPtr() : NULL, m_wideResult.nodesBytes,
                                              m_result.rootLink, m_wideRecords.getMutableCudaPtr(), m_wideRecords.getSize(),
                                              m_motionKeys.getMutableCudaPtr(), m_motionKeys.getSize(), NULL, &m_motionWideRefitResult, NULL);
    m_motionWideRefits++;
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_wideTlas = m_wideMotionCurrent = true;
    m_wideFastStale = true;
}

const uint32_t* CudaInstancedBVH::currentFastFlags(void)
{
    if (m_fastStale) {
        // on the trace's stream, ahead of it: asynchronous, nothing is read back
        m_fastFlags.resizeDiscard(4 * sizeof(U32));
        const int rc = ntr_instanced_validate(m_result.nodesBytes ? m_tlasNodes.getCudaPtr() : NULL, m_result.nodesBytes, m_poolNodes.getCudaPtr(),
                                              m_poolNodes.getSize(), (uint32_t*)m_fastFlags.getMutableCudaPtr(), NULL);
        if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_fastStale = false;
        m_fastValidations++;
    }
    return (const uint32_t*)m_fastFlags.getCudaPtr();
}

void CudaInstancedBVH::getFastFlags(U32& tlasFlags, U32& poolFlags)
{
    if (!m_built) fail("CudaInstancedBVH: No TLAS!");
    uint32_t t = 0, p = 0;
    if (ntr_instanced_flags_read(currentFastFlags(), &t, &p, NULL) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    tlasFlags = t;
    poolFlags = p;
}

const uint32_t* CudaInstancedBVH::currentWideFastFlags(void)
{
    if (m_wideFastStale) {
        // over the wide buffers themselves: after the all-wide update path the binary boxes say nothing about them
        m_wideFastFlags.resizeDiscard(4 * sizeof(U32));
        const int rc = ntr_instanced_wide_validate(m_wideResult.nodesBytes ? m_wideTlasNodes.getCudaPtr() : NULL, m_wideResult.nodesBytes,
                                                   m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                                   (uint32_t*)m_wideFastFlags.getMutableCudaPtr(), NULL);
        if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_wideFastStale = false;
        m_wideFastValidations++;
    }
    return (const uint32_t*)m_wideFastFlags.getCudaPtr();
}

void CudaInstancedBVH::getWideFastFlags(U32& tlasFlags, U32& poolFlags)
{
    if (!isWide()) fail("CudaInstancedBVH: the wide trees are not current: call widen() first");
    uint32_t t = 0, p = 0;
    if (ntr_instanced_flags_read(currentWideFastFlags(), &t, &p, NULL) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    tlasFlags = t;
    poolFlags = p;
}

F32 CudaInstancedBVH::traceBatch(RayBuffer& rays, Buffer& instanceIDs, U32 rayMask)
{
    const S32 numRays = rays.getSize();
    instanceIDs.resizeDiscard((S64)numRays * sizeof(S32));
    if (!numRays) return 0.0f;
    if (m_hasMotion) {
        // motion over the 4-wide trees, the FAST form and the seeded / world form does not exist: neither is ignored silently
        // (over the 4-wide trees only by opting in: setTraceWideMotion)
        if (m_traceWide && !m_traceWideMotion)
            fail("CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceWide: clearMotion() or setTraceWide(false)");
        if (m_traceWideFast) fail("CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceWideFast: clearMotion() or setTraceWideFast(false)");
        if (m_traceFast) fail("CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceFast: clearMotion() or setTraceFast(false)");
        if (m_world >= 0) fail("CudaInstancedBVH: motion (setMotionKey) is not combinable with setWorld: clearMotion() or clearWorld()");
    }
    if (!m_built) fail("CudaInstancedBVH: No TLAS!");
    if (m_hasMotion && m_rayTimes && m_rayTimes->getSize() < (S64)numRays * (S64)sizeof(F32))
        fail("CudaInstancedBVH: setRayTimes' buffer holds fewer than %d times", numRays);
    if (m_hasMotion && m_traceWide) {            // (m_traceWideMotion: checked above) both trees, the wide one in place, exactly once
        if (isMotionWideStale()) refitMotionWide();
    } else if (m_hasMotion && m_motionStale) refitMotion();
    float seconds = 0.0f, worldSeconds = 0.0f;
    const bool masks = m_instanceMasks.getSize() == (S64)m_numInstances * (S64)sizeof(U32);
    const bool world = m_world >= 0, wide = m_traceWide && isWide();
    const int32_t anyHit = rays.getNeedClosestHit() ? 0 : 1;
    const NtrRay* d_rays = (const NtrRay*)rays.getRayBuffer().getCudaPtr();
    NtrRayResult* d_results = (NtrRayResult*)rays.getResultBuffer().getMutableCudaPtr();
    int32_t* d_ids = (int32_t*)instanceIDs.getMutableCudaPtr();
    int rc;
    if (world) {
        // the world's single-level trace on its range of the pool; the seeded two-level trace below then runs over its records, in place
        const NtrBlasRange& wr = m_ranges[m_world];
        rc = ntr_trace_bvh(m_worldKernel.c_str(), numRays, anyHit, d_rays, d_results, (const U8*)m_poolNodes.getCudaPtr() + wr.nodesOffset,
                           wr.nodesBytes, (const U8*)m_poolTriWoop.getCudaPtr() + wr.triWoopOffset, wr.triWoopBytes,
                           (const int32_t*)m_poolTriIndex.getCudaPtr() + wr.triWoopOffset / 16, BVHLayout_Compact, 0u, NULL, &worldSeconds);
        if (rc != NTR_OK) fail("CudaInstancedBVH: the world's trace: %s", ntr_last_error());
    }
    const NtrRayResult* d_seed = world ? d_results : NULL;
    const int32_t seedInstance = world ? m_numInstances : -1;
    NtrInstanceVisibility vis;
    vis.d_instanceMasks = masks ? (const uint32_t*)m_instanceMasks.getCudaPtr() : NULL;
    vis.d_rayMasks = NULL;
    vis.rayMask = rayMask;
    vis.pad = 0;
    // the trees of the state: the 4-wide buffers or the binary ones, over the pool's one set of Woop rows
    const void* d_tlas = !wide ? m_tlasNodes.getCudaPtr() : m_wideResult.nodesBytes ? m_wideTlasNodes.getCudaPtr() : NULL;
    const int64_t tlasBytes = wide ? m_wideResult.nodesBytes : m_result.nodesBytes;
    const void* d_records = wide ? m_wideRecords.getCudaPtr() : m_records.getCudaPtr();
    const void* d_nodes = wide ? m_widePoolNodes.getCudaPtr() : m_poolNodes.getCudaPtr();
    const int64_t nodesBytes = wide ? m_widePoolResult.nodesBytes : m_poolNodes.getSize();
    const void* d_woop = m_poolTriWoop.getCudaPtr();
    const int64_t woopBytes = m_poolTriWoop.getSize();
    const int32_t* d_index = (const int32_t*)m_poolTriIndex.getCudaPtr();
    if (m_hasMotion) {
        NtrInstanceMotion motion;
        motion.d_motionKeys = m_motionKeys.getCudaPtr();
        motion.motionKeysBytes = m_motionKeys.getSize();
        motion.d_rayTimes = m_rayTimes ? (const float*)m_rayTimes->getCudaPtr() : NULL;
        motion.time = m_time;
        motion.pad = 0.0f;
        rc = wide ? ntr_trace_instanced_wide_motion(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records,
                                                    m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &motion, &seconds, NULL)
                  : ntr_trace_instanced_motion(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records,
                                               m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &motion, &seconds, NULL);
    } else if (wide && m_traceWideFast)
        rc = ntr_trace_instanced_wide_fast(numRays, anyHit, d_rays, d_seed, seedInstance, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink,
                                           d_records, m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis,
                                           currentWideFastFlags(), &seconds, NULL);
    else if (wide && world)
        rc = ntr_trace_instanced_wide_seeded(numRays, anyHit, d_rays, d_seed, seedInstance, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink,
                                             d_records, m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &seconds, NULL);
    else if (wide)
        rc = ntr_trace_instanced_wide(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records, m_numInstances,
                                      d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &seconds, NULL);
    else if (m_traceFast)
        rc = ntr_trace_instanced_fast(numRays, anyHit, d_rays, d_seed, seedInstance, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink,
                                      d_records, m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, currentFastFlags(),
                                      &seconds, NULL);
    else if (world)
        rc = ntr_trace_instanced_seeded(numRays, anyHit, d_rays, d_seed, seedInstance, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink,
                                        d_records, m_numInstances, d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &seconds, NULL);
    else if (!masks && rayMask == 0xFFFFFFFFu)
        rc = ntr_trace_instanced(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records, m_numInstances, d_nodes,
                                 nodesBytes, d_woop, woopBytes, d_index, &seconds, NULL);
    else
        rc = ntr_trace_instanced_masked(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records, m_numInstances,
                                        d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &seconds, NULL);
    seconds += worldSeconds;
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    return seconds;
}

}  // namespace FW
