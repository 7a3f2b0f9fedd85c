// instanced_deform_frame_host_test.cpp -- the host mirror's motion-blurred frames over deforming BLASes (InstancedRenderer::setDeformGeometry /
// clearDeformGeometry under setMotionBlur).  `cpu`: setDeformGeometry refuses a missing geometry and a short buffer, and
// beginFrame's "no motion key" refusal for a scene that neither moves nor deforms, without a device.  `gpu <dir>`: the scene of the seeded
// trace's tests, which the test driver writes into <dir>, with a second key of the vertices and of the transforms; beginFrame's refusal
// without setDeformGeometry; primary, AO and diffuse frames of 64 x 32 with 4 samples over the deforming-only scene and over the moving-and-
// deforming one equal the same C-ABI calls on the test's own buffers byte for byte -- times, records, normals, secondary rays, secondary
// times, resolved records, pixels; the caller's flags and times pointer come back; after refitBLASes (hasDeform() drops) the blurred frame
// is the motion path's.  Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"
#include "Random.hpp"
#include "bvh/Platform.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

template <class Call>
static bool refused(Call call, const char* word)
{
    try { call(); } catch (const FatalError& e) {
        if (std::strstr(e.message.c_str(), word)) return true;
        std::printf("refused with another message: %s\n", e.message.c_str());
    }
    return false;
}

template <class T>
static std::vector<T> load(const std::string& dir, const char* name)
{
    const std::string path = dir + "/" + name;
    std::vector<T> out;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); g_failed++; return out; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)bytes / sizeof(T));
    if (std::fread(out.data(), 1, (size_t)bytes, f) != (size_t)bytes) { std::printf("short read of %s\n", path.c_str()); g_failed++; }
    std::fclose(f);
    return out;
}

static CameraView camera(int w, int h)
{
    CameraView cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position = Vec3f(0.5f, 0.75f, -34.0f);
    F32* m = cam.nscreenToWorld.m;
    m[0] = 0.4f;  m[3] = cam.position.x;
    m[5] = -0.2f; m[7] = cam.position.y;
    m[11] = cam.position.z + 1.0f;
    m[15] = 1.0f;
    cam.cameraFar = 200.0f;
    cam.width = w;
    cam.height = h;
    return cam;
}

static void cpuTests()
{
    const float m[24] = {2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const S32 which[2] = {0, 1};
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)};
    Scene scene(2, tris, 4, verts);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CudaInstancedBVH a;
    CHECK(a.addBLAS(sah) == 0 && a.addBLAS(sah) == 1);
    a.setInstances(2, m, which);
    InstancedRenderer r(a);
    Buffer tri, pos, pos1, small;
    tri.resizeDiscard(24);
    pos.resizeDiscard(48);
    pos1.resizeDiscard(48);
    small.resizeDiscard(47);
    // the closing vertices are as many as the opening ones: setGeometry first, and no fewer bytes than numVerts * 12
    CHECK(refused([&] { r.setDeformGeometry(pos1); }, "call setGeometry() first"));
    r.setGeometry(tri, 4, pos);
    CHECK(refused([&] { r.setDeformGeometry(small); }, "fewer than 4 vertices"));
    r.setDeformGeometry(pos1);
    // a scene that neither moves nor deforms: the "no motion key" refusal, with or without the closing vertices
    const CameraView cam = camera(64, 32);
    r.setMotionBlur(true, 7, 0.25f, 0.75f);
    CHECK(!a.hasDeform() && !a.hasMotion());
    CHECK(refused([&] { r.beginFrame(cam, 64, 32); }, "setMotionKey"));
    r.clearDeformGeometry();
    CHECK(refused([&] { r.beginFrame(cam, 64, 32); }, "setMotionKey"));
    r.setMotionBlur(false);
    CHECK(refused([&] { r.beginFrame(cam, 64, 32); }, "came through addBLAS"));   // off: the frame's other refusals are what they were
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the closing vertices are bookkeeping only\n");
}

static bool same(Buffer& a, Buffer& b, S64 bytes)
{
    return a.getSize() >= bytes && b.getSize() >= bytes && std::memcmp(a.getPtr(), b.getPtr(), (size_t)bytes) == 0;
}

// What a frame leaves behind, copied out of the mirror
struct Frame {
    std::vector<U8> primaryRecords, resolved, normals, pixels;
};

// One frame through the mirror with the blur on, every buffer against the same C-ABI calls over the test's own buffers
// (deform: the CudaInstancedBVH hasDeform(), so the calls are ntr_trace_instanced_deform and ntr_instanced_hit_attributes_deform; else the
// motion path's)
static void blurredFrame(InstancedRenderer& r, CudaInstancedBVH& a, Buffer& tri, S32 numVerts, Buffer& pos, Buffer& pos1, bool deform,
                         InstancedRenderer::RayType type, int W, int H, int NS, F32 radius, U32 seed, F32 open, F32 close, Buffer& mat, Buffer& shaded,
                         Frame* out, const char* what)
{
    CHECK(a.hasDeform() == deform);
    const int n = W * H, m = n * NS, N = a.getNumInstances();
    const CameraView cam = camera(W, H);
    const bool primaryOnly = type == InstancedRenderer::RayType_Primary;
    r.setParams(type, radius, NS);
    r.setMotionBlur(true, seed, open, close);
    Buffer callers;                                  // the caller's own times pointer must survive the frame
    a.setRayTimes(&callers);
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0x5a);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch());
    RayBuffer* batch = r.getBatchRays();
    CHECK(batch && (batch == &r.getPrimaryRays()) == primaryOnly && batch->getSize() == (primaryOnly ? n : m));
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pixels, mat, shaded);
    CHECK(a.getRayTimes() == &callers && !a.isMotionStale());
    CHECK(!a.getTraceWide() && !a.getTraceFast() && !a.getTraceWideFast() && !a.getTraceWideMotion());
    a.setRayTimes(NULL);

    // the C-ABI, step by step, over the mirror's tree (which its motion refit has written) and buffers of the test's own
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);
    Buffer times, results, ids, resolved, normals;
    times.resizeDiscard((S64)n * 4);
    CHECK(ntr_ray_times_primary(n, (const int32_t*)p.getSlotToIDBuffer().getCudaPtr(), seed, open, close, (float*)times.getMutableCudaPtr(), NULL) == NTR_OK);
    CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
    CHECK(same(times, r.getPrimaryTimeBuffer(), (S64)n * 4) && r.getPrimaryTimeBuffer().getSize() == (S64)n * 4);
    const NtrTlasResult& tr = a.getBuildResult();
    NtrInstanceMotion motion;
    motion.d_motionKeys = a.getMotionKeyBuffer().getCudaPtr();
    motion.motionKeysBytes = a.getMotionKeyBuffer().getSize();
    motion.time = 0.0f;
    motion.pad = 0.0f;
    NtrInstancedGeometry g;
    g.numInstances = N;
    g.numBlas = a.getNumBLAS();
    g.numTrisTotal = (int32_t)(tri.getSize() / 12);
    g.numVerts = numVerts;
    g.d_instances = (const NtrInstance*)a.getInstanceBuffer().getCudaPtr();
    g.d_blasTris = (const NtrBlasTris*)a.getBLASTrisBuffer().getCudaPtr();
    g.d_triVtxIndex = (const int32_t*)tri.getCudaPtr();
    g.d_vtxPos = (const float*)pos.getCudaPtr();
    NtrInstancedDeformGeometry dg;
    dg.d_vtxPos1 = (const float*)pos1.getCudaPtr();
    dg.d_blasDeforming = (const uint32_t*)a.getBLASDeformingBuffer().getCudaPtr();
    auto trace = [&](RayBuffer& rays, int count, int anyHit, Buffer& t, Buffer& res, Buffer& id) {
        res.resizeDiscard((S64)count * 16);
        res.clear(0x5a);
        id.resizeDiscard((S64)count * 4);
        motion.d_rayTimes = (const float*)t.getCudaPtr();
        float seconds = 0.0f;
        const NtrInstanceDeform df = {a.getPoolNode1Buffer().getCudaPtr(), a.getPoolVertRowBuffer(0).getCudaPtr(), a.getPoolVertRowBuffer(1).getCudaPtr()};
        CHECK(ntr_trace_instanced_deform(count, anyHit, (const NtrRay*)rays.getRayBuffer().getCudaPtr(), (NtrRayResult*)res.getMutableCudaPtr(),
                                         (int32_t*)id.getMutableCudaPtr(), a.getTLASNodeBuffer().getCudaPtr(), tr.nodesBytes, tr.rootLink,
                                         a.getRecordBuffer().getCudaPtr(), N, a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(),
                                         a.getPoolTriWoopBuffer().getCudaPtr(), a.getPoolTriWoopBuffer().getSize(),
                                         (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), NULL, &motion, deform ? &df : NULL /* the motion trace */,
                                         &seconds, NULL) == NTR_OK);
    };
    auto attributes = [&](Buffer& res, Buffer& id, Buffer& t, int count, Buffer& outRes, Buffer* outNormals) {
        outRes.resizeDiscard((S64)count * 16);
        if (outNormals) outNormals->resizeDiscard((S64)count * 16);
        motion.d_rayTimes = (const float*)t.getCudaPtr();
        CHECK(ntr_instanced_hit_attributes_deform(count, (const NtrRayResult*)res.getCudaPtr(), (const int32_t*)id.getCudaPtr(), &g, &motion,
                                                  deform ? &dg : NULL /* the motion call */, (NtrRayResult*)outRes.getMutableCudaPtr(),
                                                  outNormals ? (float*)outNormals->getMutableCudaPtr() : NULL, NULL) == NTR_OK);
        CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
    };
    trace(p, n, 0, times, results, ids);
    attributes(results, ids, times, n, resolved, &normals);
    CHECK(same(results, p.getResultBuffer(), (S64)n * 16));
    CHECK(same(resolved, r.getPrimaryResolvedBuffer(), (S64)n * 16));
    if (deform) {   // the motion call on the same records: the same ids, and key 0's normals, which are not the posed triangles'
        Buffer resolved0, normals0;
        resolved0.resizeDiscard((S64)n * 16);
        normals0.resizeDiscard((S64)n * 16);
        motion.d_rayTimes = (const float*)times.getCudaPtr();
        CHECK(ntr_instanced_hit_attributes_motion(n, (const NtrRayResult*)results.getCudaPtr(), (const int32_t*)ids.getCudaPtr(), &g, &motion,
                                                  (NtrRayResult*)resolved0.getMutableCudaPtr(), (float*)normals0.getMutableCudaPtr(), NULL) == NTR_OK);
        CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
        CHECK(same(resolved0, resolved, (S64)n * 16) && !same(normals0, normals, (S64)n * 16));
    }
    Buffer pixDirect;
    pixDirect.resizeDiscard((S64)n * 4);
    pixDirect.clear(0x5a);
    int occluded = -1;
    if (primaryOnly) {
        CHECK(&r.getBatchTimeBuffer() == &r.getPrimaryTimeBuffer());
        CHECK(ntr_reconstruct(0, 1, 0, n, (const int32_t*)p.getSlotToIDBuffer().getCudaPtr(), (const NtrRayResult*)resolved.getCudaPtr(),
                              (const int32_t*)p.getIDToSlotBuffer().getCudaPtr(), (const NtrRayResult*)resolved.getCudaPtr(),
                              (const uint32_t*)mat.getCudaPtr(), (const uint32_t*)shaded.getCudaPtr(), (uint32_t*)pixDirect.getMutableCudaPtr(),
                              NULL) == NTR_OK);
    } else {
        CHECK(same(normals, r.getPrimaryNormalBuffer(), (S64)n * 16));
        const bool diffuse = type == InstancedRenderer::RayType_Diffuse;
        RayBuffer s;
        s.resize(m);
        CHECK(ntr_raygen_ao_normals((NtrRay*)s.getRayBuffer().getMutableCudaPtr(), (int32_t*)s.getIDToSlotBuffer().getMutableCudaPtr(),
                                    (int32_t*)s.getSlotToIDBuffer().getMutableCudaPtr(), (const NtrRay*)p.getRayBuffer().getCudaPtr(),
                                    (const NtrRayResult*)results.getCudaPtr(), (const float*)normals.getCudaPtr(), 0, n, NS,
                                    diffuse ? cam.cameraFar : radius, Random(0).getU32(), NULL) == NTR_OK);
        Buffer stimes, sresults, sids, sresolved;
        stimes.resizeDiscard((S64)m * 4);
        CHECK(ntr_ray_times_secondary((const float*)times.getCudaPtr(), 0, n, NS, (float*)stimes.getMutableCudaPtr(), NULL) == NTR_OK);
        CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
        CHECK(same(s.getRayBuffer(), batch->getRayBuffer(), (S64)m * 32) && same(s.getIDToSlotBuffer(), batch->getIDToSlotBuffer(), (S64)m * 4));
        CHECK(same(stimes, r.getBatchTimeBuffer(), (S64)m * 4) && r.getBatchTimeBuffer().getSize() == (S64)m * 4);
        trace(s, m, diffuse ? 0 : 1, stimes, sresults, sids);
        attributes(sresults, sids, stimes, m, sresolved, NULL);
        CHECK(same(sresults, batch->getResultBuffer(), (S64)m * 16));
        CHECK(same(sresolved, r.getBatchResolvedBuffer(), (S64)m * 16));
        CHECK(ntr_reconstruct((int)type, NS, 0, n, (const int32_t*)p.getSlotToIDBuffer().getCudaPtr(), (const NtrRayResult*)resolved.getCudaPtr(),
                              (const int32_t*)s.getIDToSlotBuffer().getCudaPtr(), (const NtrRayResult*)sresolved.getCudaPtr(),
                              (const uint32_t*)mat.getCudaPtr(), (const uint32_t*)shaded.getCudaPtr(), (uint32_t*)pixDirect.getMutableCudaPtr(),
                              NULL) == NTR_OK);
        const NtrRayResult* sr = (const NtrRayResult*)sresolved.getPtr();
        occluded = 0;
        for (int i = 0; i < m; i++) occluded += sr[i].id >= 0 ? 1 : 0;
        CHECK(occluded > 0 && occluded < m);
    }
    CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
    CHECK(same(pixels, pixDirect, (S64)n * 4));
    CHECK(!r.nextBatch());
    const NtrRayResult* pr = (const NtrRayResult*)resolved.getPtr();
    int hits = 0;
    for (int i = 0; i < n; i++) hits += pr[i].id >= 0 ? 1 : 0;
    CHECK(hits > 0);
    if (out) {
        out->primaryRecords.assign(results.getPtr(), results.getPtr() + (size_t)n * 16);
        out->resolved.assign(resolved.getPtr(), resolved.getPtr() + (size_t)n * 16);
        out->normals.assign(normals.getPtr(), normals.getPtr() + (size_t)n * 16);
        out->pixels.assign(pixels.getPtr(), pixels.getPtr() + (size_t)n * 4);
    }
    std::printf("%s: the blurred frame equals the C-ABI, %d primary hits, %d secondary rays hit\n", what, hits, occluded);
}

// One AO frame with the blur off -> what it left
static void plainFrame(InstancedRenderer& r, int W, int H, int NS, F32 radius, Buffer& mat, Buffer& shaded, Frame& out)
{
    const int n = W * H;
    r.setParams(InstancedRenderer::RayType_AO, radius, NS);
    r.setMotionBlur(false);
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0x5a);
    r.beginFrame(camera(W, H), W, H);
    CHECK(r.nextBatch());
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pixels, mat, shaded);
    CHECK(!r.nextBatch());
    const U8* a = r.getPrimaryRays().getResultBuffer().getPtr();
    out.primaryRecords.assign(a, a + (size_t)n * 16);
    a = r.getPrimaryResolvedBuffer().getPtr();
    out.resolved.assign(a, a + (size_t)n * 16);
    a = r.getPrimaryNormalBuffer().getPtr();
    out.normals.assign(a, a + (size_t)n * 16);
    out.pixels.assign(pixels.getPtr(), pixels.getPtr() + (size_t)n * 4);
}

static bool equal(const Frame& a, const Frame& b)
{
    return a.primaryRecords == b.primaryRecords && a.resolved == b.resolved && a.normals == b.normals && a.pixels == b.pixels;
}

static void gpuTests(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
    std::vector<float> vtx = load<float>(dir, "pos.bin");
    std::vector<float> vtx1 = load<float>(dir, "pos1.bin");
    std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
    std::vector<float> xf = load<float>(dir, "transforms.bin");
    std::vector<float> xf1 = load<float>(dir, "transforms1.bin");
    std::vector<S32> which = load<S32>(dir, "blas.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size();
    CHECK(numTris > 0 && B == 3 && N == 32 && (S32)xf.size() == 12 * N && xf1.size() == xf.size() && vtx1.size() == vtx.size());
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12), pos1(vtx1.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[(size_t)i] = 0xff000000u | (U32)((U32)i * 2654435761u >> 8);
        sc[(size_t)i] = 0xff000000u | (U32)((U32)(i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);

    CudaInstancedBVH a;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    const int W = 64, H = 32, NS = 4;
    const F32 radius = 2.0f;
    const CameraView cam = camera(W, H);
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    Frame today, off, only, only9, both, after;
    plainFrame(r, W, H, NS, radius, mat, shaded, today);

    // BLASes 1 and 2 deform, no instance moves.  Without the closing vertices the blur stays refused, and the message names the remedy
    const S32 sel[2] = {1, 2};
    a.refitBLASesMotion(tri, numVerts, pos, pos1, sel, 2);
    a.refit();
    CHECK(a.hasDeform() && !a.hasMotion());
    r.setMotionBlur(true);
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "not combinable with deforming BLASes"));
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "setDeformGeometry"));
    Buffer small;
    small.resizeDiscard((S64)numVerts * 12 - 1);
    CHECK(refused([&] { r.setDeformGeometry(small); }, "fewer than"));
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "not combinable with deforming BLASes"));   // (a refused buffer is not kept)
    r.setDeformGeometry(pos1);

    // a scene that only deforms renders blurred frames: refitMotion() passes key 0 twice
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_Primary, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, NULL, "deforming only, primary");
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_AO, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, &only, "deforming only, AO");
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_AO, W, H, NS, radius, 9, 0.125f, 0.875f, mat, shaded, &only9,
                 "deforming only, AO, seed 9, shutter [1/8, 7/8]");
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_Diffuse, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, NULL, "deforming only, diffuse");
    CHECK(!a.hasMotion() && !equal(only, today) && !equal(only, only9) && only.normals != today.normals);   // something deforms in the picture

    // the instances move too
    a.setMotionKey(N, xf1.data());
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_Primary, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, NULL, "moving and deforming, primary");
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_AO, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, &both, "moving and deforming, AO");
    blurredFrame(r, a, tri, numVerts, pos, pos1, true, InstancedRenderer::RayType_Diffuse, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, NULL, "moving and deforming, diffuse");
    CHECK(!equal(both, only) && both.normals != only.normals);

    // without the closing vertices the refusal is back; with them and the blur off the frame is key 0's with the scalar time, as before
    r.clearDeformGeometry();
    r.setMotionBlur(true);
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "not combinable with deforming BLASes"));
    r.setDeformGeometry(pos1);
    a.setTime(0.0f);
    a.setRayTimes(NULL);
    plainFrame(r, W, H, NS, radius, mat, shaded, off);
    CHECK(a.hasDeform() && equal(off, today));

    // a plain refit of the pool drops the deformation: the next blurred frame is the motion path's
    a.refitBLASes(tri, numVerts, pos);
    a.refit();
    CHECK(!a.hasDeform() && a.hasMotion());
    blurredFrame(r, a, tri, numVerts, pos, pos1, false, InstancedRenderer::RayType_AO, W, H, NS, radius, 0, 0.0f, 1.0f, mat, shaded, &after, "after refitBLASes, AO");
    CHECK(!equal(after, both) && after.normals != both.normals);
    // and with neither a motion key nor a deformation there is nothing to blur
    a.clearMotion();
    r.setMotionBlur(true);
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "setMotionKey"));
    r.setMotionBlur(false);
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) gpuTests(argv[2]);
        else cpuTests();
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        g_failed++;
    }
    if (g_failed) { std::printf("instanced_deform_frame_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_deform_frame_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
