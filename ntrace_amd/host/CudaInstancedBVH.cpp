// CudaInstancedBVH.cpp -- a pool of BLASes, instances and their top-level tree over the ntr_tlas_*, ntr_pool_*, ntr_instanced_* and
// ntr_trace_instanced* entry points that the header names method by method; what is current is m_state's (InstancedState.hpp).
#include "CudaInstancedBVH.hpp"

#include <cstring>

namespace FW {

typedef InstancedState::Write W;
typedef InstancedState::Product P;

CudaInstancedBVH::CudaInstancedBVH(void) {}

// meshTriangles: the triangles of triVtxIndex; selectionSize: the number of selected BLASes of numBlas (blas NULL: all); selectedBLAS: the i-th
static S64 meshTriangles(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos)
{
    const S64 numTris = triVtxIndex.getSize() / (S64)(3 * sizeof(S32));
    if (numTris < 1 || numTris >= (1ll << 28) || vtxPos.getSize() < (S64)numVerts * (S64)(3 * sizeof(F32))) fail("CudaInstancedBVH: bad mesh buffers");
    return numTris;
}

static S32 selectionSize(const S32* blas, S32 num, S32 numBlas, const char* what)
{
    if (numBlas < 1) fail("CudaInstancedBVH: no BLASes to %s", what);
    if (!blas) num = numBlas;
    if (num < 1) fail("CudaInstancedBVH: no BLASes selected");
    return num;
}

static S32 selectedBLAS(const S32* blas, S32 i, S32 numBlas)
{
    const S32 b = blas ? blas[i] : i;
    if (b < 0 || b >= numBlas) fail("CudaInstancedBVH: BLAS index %d outside [0, %d)", b, numBlas);
    return b;
}

// a refit's scene box becomes the build result's
static void takeSceneBox(NtrTlasResult& result, const NtrTlasRefitResult& refit)
{
    std::memcpy(result.sceneMin, refit.sceneMin, sizeof(result.sceneMin));
    std::memcpy(result.sceneMax, refit.sceneMax, sizeof(result.sceneMax));
}

static void readFlags(const uint32_t* d_flags, U32& tlasFlags, U32& poolFlags)
{
    uint32_t t = 0, p = 0;
    if (ntr_instanced_flags_read(d_flags, &t, &p, NULL) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    tlasFlags = t;
    poolFlags = p;
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
    m_meshes.push_back(Mesh{0, 0});
    m_state.wrote(W::PoolTrees);
    return (S32)m_ranges.size() - 1;
}

void CudaInstancedBVH::buildBLASes(S32 numMeshes, const NtrPlocBatchMesh* meshes, Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, S32 radius)
{
    if (numMeshes < 1 || !meshes) fail("CudaInstancedBVH: no meshes");
    std::vector<NtrBlasRange> ranges((size_t)numMeshes);
    int64_t capN, capW, capI;
    if (ntr_ploc_batch_capacity(numMeshes, meshes, ranges.data(), &capN, &capW, &capI) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    const S64 numTris = meshTriangles(triVtxIndex, numVerts, vtxPos);
    m_ranges.clear();
    m_meshes.clear();
    clearWorld();                                    // the pool is replaced: whatever BLAS the world named is gone
    m_state.wrote(W::PoolTrees);
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
    for (S32 k = 0; k < numMeshes; k++) m_meshes[k] = Mesh{meshes[k].firstTri, meshes[k].numTris};
}

Buffer& CudaInstancedBVH::getBLASTrisBuffer(void)
{
    if (!m_state.has(P::BlasTris)) {
        static_assert(sizeof(Mesh) == sizeof(NtrBlasTris), "Mesh is NtrBlasTris");
        m_blasTris.resizeDiscard((S64)m_meshes.size() * sizeof(NtrBlasTris));
        if (!m_meshes.empty()) m_blasTris.set(m_meshes.data(), (S64)m_meshes.size() * sizeof(NtrBlasTris));
        m_state.made(P::BlasTris);
    }
    return m_blasTris;
}

S32 CudaInstancedBVH::getFirstMeshlessBLAS(void) const
{
    for (size_t k = 0; k < m_meshes.size(); k++)
        if (m_meshes[k].numTris < 1) return (S32)k;
    return -1;
}

// The selection (`num` as selectionSize gave it) as ntr_bvh_refit_batch's and ntr_bvh_motion_refit_batch's entries
std::vector<NtrRefitBatchEntry> CudaInstancedBVH::refitEntries(const S32* blas, S32 num, F32 epsilon) const
{
    std::vector<NtrRefitBatchEntry> entries((size_t)num);
    for (S32 i = 0; i < num; i++) {
        const S32 b = selectedBLAS(blas, i, getNumBLAS());
        if (m_meshes[b].numTris < 1) fail("CudaInstancedBVH: BLAS %d came through addBLAS and has no mesh here: refit its CudaBVH and add it again", b);
        NtrRefitBatchEntry& e = entries[i];
        e.range = m_ranges[b];
        e.firstTri = m_meshes[b].firstTri;
        e.numTris = m_meshes[b].numTris;
        e.epsilon = epsilon;
        e.pad = 0;
    }
    return entries;
}

void CudaInstancedBVH::refitBLASes(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas, S32 num, F32 epsilon)
{
    num = selectionSize(blas, num, getNumBLAS(), "refit (call buildBLASes first)");
    const S64 numTris = meshTriangles(triVtxIndex, numVerts, vtxPos);
    const std::vector<NtrRefitBatchEntry> entries = refitEntries(blas, num, epsilon);
    m_state.wrote(W::PoolBoxes);                 // this method refits the binary pool only: widen() again, or call refitBLASesWide
    const int rc = ntr_bvh_refit_batch(num, entries.data(), m_poolNodes.getMutableCudaPtr(), m_poolNodes.getSize(),
                                       m_poolTriWoop.getMutableCudaPtr(), m_poolTriWoop.getSize(), (const int32_t*)m_poolTriIndex.getCudaPtr(),
                                       (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(), numVerts, (const float*)vtxPos.getCudaPtr(),
                                       NULL, &m_refitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
}

void CudaInstancedBVH::refitBLASesMotion(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos0, Buffer& vtxPos1, const S32* blas, S32 num, F32 epsilon)
{
    num = selectionSize(blas, num, getNumBLAS(), "refit (call buildBLASes first)");
    const S64 numTris = meshTriangles(triVtxIndex, numVerts, vtxPos0);
    meshTriangles(triVtxIndex, numVerts, vtxPos1);
    const std::vector<NtrRefitBatchEntry> entries = refitEntries(blas, num, epsilon);
    // BLASes that an earlier call made deforming stay so while their second key is still the pool's
    const bool keep = hasDeform() && m_deformFlags.size() == m_ranges.size();
    if (!keep) m_deformFlags.assign(m_ranges.size(), 0u);
    m_state.wrote(W::PoolBoxes);                 // key 0 is refitted in place, as refitBLASes: refit() or build() again
    m_state.wrote(W::PoolKey1);
    if (keep) {
        m_poolNodes1.resize(m_poolNodes.getSize());
        m_poolVertRows0.resize(m_poolTriWoop.getSize());
        m_poolVertRows1.resize(m_poolTriWoop.getSize());
    } else {
        m_poolNodes1.resizeDiscard(m_poolNodes.getSize());
        m_poolVertRows0.resizeDiscard(m_poolTriWoop.getSize());
        m_poolVertRows1.resizeDiscard(m_poolTriWoop.getSize());
    }
    m_hasDeform = false;
    const int rc = ntr_bvh_motion_refit_batch(num, entries.data(), m_poolNodes.getMutableCudaPtr(), m_poolNodes.getSize(),
                                              m_poolNodes1.getMutableCudaPtr(), m_poolTriWoop.getMutableCudaPtr(), m_poolTriWoop.getSize(),
                                              (const int32_t*)m_poolTriIndex.getCudaPtr(), m_poolVertRows0.getMutableCudaPtr(),
                                              m_poolVertRows1.getMutableCudaPtr(), (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(),
                                              numVerts, (const float*)vtxPos0.getCudaPtr(), (const float*)vtxPos1.getCudaPtr(), NULL,
                                              &m_blasMotionRefitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    for (S32 i = 0; i < num; i++) m_deformFlags[(size_t)selectedBLAS(blas, i, getNumBLAS())] = 1u;
    m_blasDeforming.resizeDiscard((S64)m_deformFlags.size() * sizeof(U32));
    m_blasDeforming.set(m_deformFlags.data(), (S64)m_deformFlags.size() * sizeof(U32));
    m_hasDeform = true;
    m_state.made(P::PoolDeform);
}

void CudaInstancedBVH::clearDeform(void)
{
    // the pool stays refitted to key 0 and the TLAS's boxes still bound the sweep: isBuilt() stays, as after clearMotion()
    m_hasDeform = false;
    m_deformFlags.assign(m_ranges.size(), 0u);
    m_state.wrote(W::PoolKey1);
    m_state.lost(P::PoolDeform);
}

void CudaInstancedBVH::selectRanges(const S32* blas, S32 num, std::vector<NtrBlasRange>& out, const char* what) const
{
    num = selectionSize(blas, num, getNumBLAS(), what);
    out.resize((size_t)num);
    for (S32 i = 0; i < num; i++) out[(size_t)i] = m_ranges[(size_t)selectedBLAS(blas, i, getNumBLAS())];
}

void CudaInstancedBVH::optimizeBLASes(const S32* blas, S32 num, S32 passes)
{
    std::vector<NtrBlasRange> sel;
    selectRanges(blas, num, sel, "optimise");
    m_state.wrote(W::PoolInnerBoxes);            // the binary pool's topology changes: widen() again (isBuilt() stays, see the header)
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
        m_state.wrote(W::InstanceCount);             // an unchanged count keeps the TLAS's topology for refit() ...
        m_instanceMasks.resizeDiscard(0);            // ... and the instance masks: with another count they would name other instances
        clearMotion();                               // ... and key 1 of the motion
    }
    m_numInstances = num;
    m_state.wrote(W::Instances);
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
        m_state.wrote(W::InstanceCount);             // as setInstances: an unchanged count keeps the topology, the masks and key 1
        m_instanceMasks.resizeDiscard(0);
        clearMotion();
    }
    m_numInstances = num;
    m_state.wrote(W::Instances);
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
    m_state.wrote(W::World);
    writeWorldRecord();                              // the TLAS never sees the world: isBuilt() stays
}

void CudaInstancedBVH::clearWorld(void)
{
    if (m_world < 0) return;
    m_world = -1;
    m_state.wrote(W::World);
    m_instances.resize((S64)m_numInstances * sizeof(NtrInstance));
}

void CudaInstancedBVH::setInstanceMasks(const U32* masks)
{
    if (m_numInstances < 1) fail("CudaInstancedBVH: no instances to mask (call setInstances first)");
    if (!masks) { m_instanceMasks.resizeDiscard(0); return; }
    m_instanceMasks.resizeDiscard((S64)m_numInstances * sizeof(U32));
    m_instanceMasks.set(masks, (S64)m_numInstances * sizeof(U32));   // the TLAS knows nothing of visibility: isBuilt() stays
}

void CudaInstancedBVH::build(S32 radius)
{
    if (m_ranges.empty() || m_numInstances < 1) fail("CudaInstancedBVH: nothing to build");
    int64_t capN, capR;
    if (ntr_tlas_capacity(m_numInstances, &capN, &capR) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_state.wrote(W::TlasTopology);              // with it the records, without moving flags, and boxes of key 0 alone
    m_state.wrote(W::TlasBoxes);
    m_tlasNodes.resizeDiscard(capN);
    m_records.resizeDiscard(capR);
    const int rc = ntr_tlas_build(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                  m_poolNodes.getCudaPtr(), m_poolNodes.getSize(), radius, m_tlasNodes.getMutableCudaPtr(), capN,
                                  m_records.getMutableCudaPtr(), capR, &m_result, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    if (m_result.nodesBytes) m_tlasNodes.resize(m_result.nodesBytes);   // (N == 1 has no node: the buffer keeps its one unused slot)
    m_state.made(P::TlasTopology);
    m_state.made(P::TlasBoxes);
}

void CudaInstancedBVH::refit(void)
{
    if (!m_state.mayRefit() || m_numInstances < 1)
        fail("CudaInstancedBVH: no TLAS to refit: call build() first, and again after the instance count or the BLASes have changed");
    m_state.wrote(W::TlasBoxes);                 // as build(): the moving flags are cleared, the scene is frozen at key 0
    const int rc = ntr_tlas_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                  m_poolNodes.getCudaPtr(), m_poolNodes.getSize(), m_result.nodesBytes ? m_tlasNodes.getMutableCudaPtr() : NULL,
                                  m_result.nodesBytes, m_result.rootLink, m_records.getMutableCudaPtr(), m_records.getSize(), NULL,
                                  &m_tlasRefitResult, NULL);
    if (rc != NTR_OK) {
        m_state.lost(P::TlasBoxes);              // a part of the tree kept stale boxes
        fail("CudaInstancedBVH: %s", ntr_last_error());
    }
    takeSceneBox(m_result, m_tlasRefitResult);
    m_state.made(P::TlasBoxes);
}

void CudaInstancedBVH::setMotionKey(S32 num, const F32* objectToWorld1)
{
    if (num < 1 || !objectToWorld1) fail("CudaInstancedBVH: no motion key");
    if (num != m_numInstances) fail("CudaInstancedBVH: the motion key names %d instances, setInstances %d", num, m_numInstances);
    m_instances1.resizeDiscard((S64)num * sizeof(NtrInstance));
    NtrInstance* inst = (NtrInstance*)m_instances1.getMutablePtrDiscard();
    std::memset(inst, 0, (size_t)num * sizeof(NtrInstance));   // of key 1 only objectToWorld is read
    for (S32 i = 0; i < num; i++) std::memcpy(inst[i].objectToWorld, objectToWorld1 + 12 * (size_t)i, sizeof(inst[i].objectToWorld));
    m_hasMotion = true;
    m_state.wrote(W::MotionKey);
}

void CudaInstancedBVH::setMotionKeyDevice(S32 num, Buffer& instances1)
{
    if (num < 1) fail("CudaInstancedBVH: no motion key");
    if (num != m_numInstances) fail("CudaInstancedBVH: the motion key names %d instances, setInstances %d", num, m_numInstances);
    if (instances1.getSize() < (S64)num * (S64)sizeof(NtrInstance)) fail("CudaInstancedBVH: the motion key's buffer is smaller than its count");
    m_instances1.resizeDiscard((S64)num * sizeof(NtrInstance));
    m_instances1.setRange(0, instances1, 0, (S64)num * sizeof(NtrInstance));
    m_hasMotion = true;
    m_state.wrote(W::MotionKey);
}

void CudaInstancedBVH::clearMotion(void)
{
    // the records keep their moving flags, which only the motion trace reads, and the boxes still bound the sweep: isBuilt() stays
    m_hasMotion = false;
    m_state.wrote(W::MotionKey);
    m_instances1.resizeDiscard(0);
}

void CudaInstancedBVH::refitMotion(void)
{
    const bool deform = hasDeform();
    if (!m_hasMotion && !deform) fail("CudaInstancedBVH: no motion key: call setMotionKey first");
    if (!isBuilt()) fail("CudaInstancedBVH: No TLAS!");
    const bool wasCurrent = !isMotionStale();
    m_state.wrote(W::TlasBoxes);                 // the binary boxes become the swept ones: as refit()
    m_motionKeys.resizeDiscard((S64)m_numInstances * 128);
    // with deforming BLASes the leaf boxes are the unions over both keys of the instances AND of the BLASes, and the records say which
    // instances' BLASes deform; without a motion key the instances' key 1 is key 0
    const int rc = deform
        ? ntr_tlas_deform_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(),
                                (const NtrInstance*)(m_hasMotion ? m_instances1 : m_instances).getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                m_poolNodes.getCudaPtr(), m_poolNodes1.getCudaPtr(), m_poolNodes.getSize(),
                                (const uint32_t*)m_blasDeforming.getCudaPtr(), m_result.nodesBytes ? m_tlasNodes.getMutableCudaPtr() : NULL,
                                m_result.nodesBytes, m_result.rootLink, m_records.getMutableCudaPtr(), m_records.getSize(),
                                m_motionKeys.getMutableCudaPtrDiscard(), m_motionKeys.getSize(), NULL, &m_deformRefitResult, NULL)
        : ntr_tlas_motion_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (const NtrInstance*)m_instances1.getCudaPtr(),
                                         (int32_t)m_ranges.size(), m_ranges.data(), m_poolNodes.getCudaPtr(), m_poolNodes.getSize(),
                                         m_result.nodesBytes ? m_tlasNodes.getMutableCudaPtr() : NULL, m_result.nodesBytes, m_result.rootLink,
                                         m_records.getMutableCudaPtr(), m_records.getSize(), m_motionKeys.getMutableCudaPtrDiscard(),
                                         m_motionKeys.getSize(), NULL, &m_motionRefitResult, NULL);
    m_motionRefits++;
    if (rc != NTR_OK) {
        m_state.lost(P::TlasBoxes);              // a part of the tree kept stale boxes
        if (wasCurrent) m_state.made(P::MotionRefit);   // outside the table: a failed call leaves isMotionStale() as it was
        fail("CudaInstancedBVH: %s", ntr_last_error());
    }
    if (deform) m_motionRefitResult = m_deformRefitResult.motion;
    takeSceneBox(m_result, m_motionRefitResult.refit);
    m_state.made(P::MotionRefit);
}

void CudaInstancedBVH::widen(void)
{
    if (!isBuilt()) fail("CudaInstancedBVH: no TLAS to widen: call build() or refit() first");
    const int32_t numBlas = (int32_t)m_ranges.size();
    m_state.wrote(W::WideTlas);                  // wide boxes are written; the wide records will have no moving flags
    if (!isWidePoolCurrent()) {
        m_state.wrote(W::WidePool);
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
        m_state.made(P::WidePool);
    }
    int64_t capT = 0;
    if (m_result.rootLink == 0 && ntr_bvh_widen_capacity(m_result.nodesBytes, &capT) != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_wideTlasNodes.resizeDiscard(capT ? capT : 128);
    m_wideRecords.resizeDiscard((S64)m_numInstances * 64);
    const int rc = ntr_tlas_widen(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), m_result.rootLink == 0 ? m_tlasNodes.getCudaPtr() : NULL,
                                  m_result.nodesBytes, m_result.rootLink, numBlas, m_ranges.data(), m_wideRanges.data(),
                                  m_result.rootLink == 0 ? m_wideTlasNodes.getMutableCudaPtr() : NULL, capT, m_wideRecords.getMutableCudaPtr(),
                                  m_wideRecords.getSize(), &m_wideResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_state.made(P::WideTlas);
    m_state.made(P::WideTopology);
}

void CudaInstancedBVH::refitBLASesWide(Buffer& triVtxIndex, S32 numVerts, Buffer& vtxPos, const S32* blas, S32 num, F32 epsilon)
{
    if (!isWidePoolCurrent()) fail("CudaInstancedBVH: no current wide pool to refit: call widen() first, and again after refitBLASes, buildBLASes or addBLAS");
    if (!blas) num = (S32)m_ranges.size();
    refitBLASes(triVtxIndex, numVerts, vtxPos, blas, num, epsilon);   // the binary pool stays current; the selection is checked there
    std::vector<NtrWideRefitEntry> entries((size_t)num);
    for (S32 i = 0; i < num; i++) {
        const S32 b = selectedBLAS(blas, i, getNumBLAS());
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
    const S64 numTris = meshTriangles(triVtxIndex, numVerts, vtxPos);
    m_state.wrote(W::WidePool);
    const int rc = ntr_pool_wide_refit(num, entries.data(), m_widePoolNodes.getMutableCudaPtr(), m_widePoolResult.nodesBytes,
                                       m_poolTriWoop.getMutableCudaPtr(), m_poolTriWoop.getSize(), (const int32_t*)m_poolTriIndex.getCudaPtr(),
                                       (int32_t)numTris, (const int32_t*)triVtxIndex.getCudaPtr(), numVerts, (const float*)vtxPos.getCudaPtr(),
                                       0 /* the binary refit has written the rows */, NULL, &m_wideBlasRefitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_state.made(P::WidePool);                   // (refitBLASes dropped it: the wide boxes are the new ones again)
}

void CudaInstancedBVH::refitWide(void)
{
    if (!m_state.mayRefitWide() || m_numInstances < 1)
        fail("CudaInstancedBVH: no wide TLAS to refit: call build() and widen() first, and again after the instance count or the BLASes have changed");
    if (!isWidePoolCurrent()) fail("CudaInstancedBVH: the wide pool is not current: call refitBLASesWide() in place of refitBLASes(), or widen()");
    refit();                                     // the binary TLAS and records stay current
    m_state.wrote(W::WideTlas);                  // word 15 = 0 everywhere: the wide trees are frozen at key 0
    const int rc = ntr_tlas_wide_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                       m_wideRanges.data(), m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                       m_wideResult.nodesBytes ? m_wideTlasNodes.getMutableCudaPtr() : NULL, m_wideResult.nodesBytes,
                                       m_result.rootLink, m_wideRecords.getMutableCudaPtr(), m_wideRecords.getSize(), NULL,
                                       &m_wideTlasRefitResult, NULL);
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_state.made(P::WideTlas);
}

void CudaInstancedBVH::refitMotionWide(void)
{
    if (!m_state.mayRefitWide() || m_numInstances < 1)
        fail("CudaInstancedBVH: no wide TLAS for the motion refit: call build() and widen() first, and again after the instance count or the BLASes "
             "have changed");
    if (!isWidePoolCurrent()) fail("CudaInstancedBVH: the wide pool is not current: call refitBLASesWide() in place of refitBLASes(), or widen()");
    refitMotion();                               // the binary TLAS, its records and the motion keys stay current
    m_state.wrote(W::WideTlas);
    const int rc = ntr_tlas_wide_motion_refit(m_numInstances, (const NtrInstance*)m_instances.getCudaPtr(),
                                              (const NtrInstance*)m_instances1.getCudaPtr(), (int32_t)m_ranges.size(), m_ranges.data(),
                                              m_wideRanges.data(), m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                              m_wideResult.nodesBytes ? m_wideTlasNodes.getMutableCudaPtr() : NULL, m_wideResult.nodesBytes,
                                              m_result.rootLink, m_wideRecords.getMutableCudaPtr(), m_wideRecords.getSize(),
                                              m_motionKeys.getMutableCudaPtr(), m_motionKeys.getSize(), NULL, &m_motionWideRefitResult, NULL);
    m_motionWideRefits++;
    if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
    m_state.made(P::WideTlas);
    m_state.made(P::WideMotionRefit);
}

const uint32_t* CudaInstancedBVH::currentFastFlags(void)
{
    if (isFastFlagsStale()) {
        // on the trace's stream, ahead of it: asynchronous, nothing is read back
        m_fastFlags.resizeDiscard(4 * sizeof(U32));
        const int rc = ntr_instanced_validate(m_result.nodesBytes ? m_tlasNodes.getCudaPtr() : NULL, m_result.nodesBytes, m_poolNodes.getCudaPtr(),
                                              m_poolNodes.getSize(), (uint32_t*)m_fastFlags.getMutableCudaPtr(), NULL);
        if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_state.made(P::FastFlags);
        m_fastValidations++;
    }
    return (const uint32_t*)m_fastFlags.getCudaPtr();
}

void CudaInstancedBVH::getFastFlags(U32& tlasFlags, U32& poolFlags)
{
    if (!isBuilt()) fail("CudaInstancedBVH: No TLAS!");
    readFlags(currentFastFlags(), tlasFlags, poolFlags);
}

const uint32_t* CudaInstancedBVH::currentWideFastFlags(void)
{
    if (isWideFastFlagsStale()) {
        // over the wide buffers themselves: after the all-wide update path the binary boxes say nothing about them
        m_wideFastFlags.resizeDiscard(4 * sizeof(U32));
        const int rc = ntr_instanced_wide_validate(m_wideResult.nodesBytes ? m_wideTlasNodes.getCudaPtr() : NULL, m_wideResult.nodesBytes,
                                                   m_widePoolNodes.getCudaPtr(), m_widePoolResult.nodesBytes,
                                                   (uint32_t*)m_wideFastFlags.getMutableCudaPtr(), NULL);
        if (rc != NTR_OK) fail("CudaInstancedBVH: %s", ntr_last_error());
        m_state.made(P::WideFastFlags);
        m_wideFastValidations++;
    }
    return (const uint32_t*)m_wideFastFlags.getCudaPtr();
}

void CudaInstancedBVH::getWideFastFlags(U32& tlasFlags, U32& poolFlags)
{
    if (!isWide()) fail("CudaInstancedBVH: the wide trees are not current: call widen() first");
    readFlags(currentWideFastFlags(), tlasFlags, poolFlags);
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
    const bool deform = hasDeform();
    if (deform) {
        // deforming BLASes exist over the binary trees only, without FAST flags and without a seed: nothing is ignored silently
        if (m_traceWideMotion)
            fail("CudaInstancedBVH: deforming BLASes (refitBLASesMotion) are not combinable with setTraceWideMotion: clearDeform() or setTraceWideMotion(false)");
        if (m_traceWide) fail("CudaInstancedBVH: deforming BLASes (refitBLASesMotion) are not combinable with setTraceWide: clearDeform() or setTraceWide(false)");
        if (m_traceWideFast) fail("CudaInstancedBVH: deforming BLASes (refitBLASesMotion) are not combinable with setTraceWideFast: clearDeform() or setTraceWideFast(false)");
        if (m_traceFast) fail("CudaInstancedBVH: deforming BLASes (refitBLASesMotion) are not combinable with setTraceFast: clearDeform() or setTraceFast(false)");
        if (m_world >= 0) fail("CudaInstancedBVH: deforming BLASes (refitBLASesMotion) are not combinable with setWorld: clearDeform() or clearWorld()");
    }
    if (!isBuilt()) fail("CudaInstancedBVH: No TLAS!");
    const bool timed = m_hasMotion || deform;    // the rays carry times
    if (timed && m_rayTimes && m_rayTimes->getSize() < (S64)numRays * (S64)sizeof(F32))
        fail("CudaInstancedBVH: setRayTimes' buffer holds fewer than %d times", numRays);
    if (m_hasMotion && m_traceWide) {            // (m_traceWideMotion: checked above; never with deform) both trees, the wide one in place, exactly once
        if (isMotionWideStale()) refitMotionWide();
    } else if (timed && isMotionStale()) refitMotion();
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
    const NtrInstanceVisibility vis = {masks ? (const uint32_t*)m_instanceMasks.getCudaPtr() : NULL, NULL /* d_rayMasks */, rayMask, 0};
    // the trees of the state: the 4-wide buffers or the binary ones, over the pool's one set of Woop rows
    const void* d_tlas = !wide ? m_tlasNodes.getCudaPtr() : m_wideResult.nodesBytes ? m_wideTlasNodes.getCudaPtr() : NULL;
    const int64_t tlasBytes = wide ? m_wideResult.nodesBytes : m_result.nodesBytes;
    const void* d_records = wide ? m_wideRecords.getCudaPtr() : m_records.getCudaPtr();
    const void* d_nodes = wide ? m_widePoolNodes.getCudaPtr() : m_poolNodes.getCudaPtr();
    const int64_t nodesBytes = wide ? m_widePoolResult.nodesBytes : m_poolNodes.getSize();
    const void* d_woop = m_poolTriWoop.getCudaPtr();
    const int64_t woopBytes = m_poolTriWoop.getSize();
    const int32_t* d_index = (const int32_t*)m_poolTriIndex.getCudaPtr();
    if (deform) {
        const NtrInstanceMotion motion = {m_motionKeys.getCudaPtr(), m_motionKeys.getSize(),
                                          m_rayTimes ? (const float*)m_rayTimes->getCudaPtr() : NULL, m_time, 0.0f};
        const NtrInstanceDeform df = {m_poolNodes1.getCudaPtr(), m_poolVertRows0.getCudaPtr(), m_poolVertRows1.getCudaPtr()};
        rc = ntr_trace_instanced_deform(numRays, anyHit, d_rays, d_results, d_ids, d_tlas, tlasBytes, m_result.rootLink, d_records, m_numInstances,
                                        d_nodes, nodesBytes, d_woop, woopBytes, d_index, &vis, &motion, &df, &seconds, NULL);
    } else if (m_hasMotion) {
        const NtrInstanceMotion motion = {m_motionKeys.getCudaPtr(), m_motionKeys.getSize(),
                                          m_rayTimes ? (const float*)m_rayTimes->getCudaPtr() : NULL, m_time, 0.0f};
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
