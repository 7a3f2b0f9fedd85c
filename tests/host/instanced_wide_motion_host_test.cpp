// instanced_wide_motion_host_test.cpp -- the host mirror's motion blur over the 4-wide trees (CudaInstancedBVH::setTraceWideMotion /
// refitMotionWide, InstancedRenderer::setWideMotion).  `cpu`: the switch is off by default, and off every refusal of motion
// with the wide, FAST and world forms is word for word what it was; on, setTraceWide is accepted and the others are still refused by
// name; refitMotionWide() without a widen() names widen().  `gpu <dir>`: the scene of the seeded trace's tests with a second key, which
// the test driver writes into <dir>: traceBatch takes the wide motion launch after exactly one refitMotionWide(), its records equal
// ntr_tlas_wide_motion_refit + ntr_trace_instanced_wide_motion on buffers of the test's own byte for byte, and staleness follows
// setMotionKey, setInstances, build, refit, refitWide and widen; then an AO frame on the turning cube of the motion frame tests, blurred,
// over the binary trees and over the wide ones.  Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"
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

// the whole message, word for word
template <class Call>
static bool refusedWith(Call call, const char* message)
{
    try { call(); } catch (const FatalError& e) {
        if (e.message == message) return true;
        std::printf("refused with another message: %s\n", e.message.c_str());
    }
    return false;
}

// what traceBatch says today when motion meets a form it is not combinable with (CudaInstancedBVH.cpp as of DESIGN.md 6aa)
static const char* const kWide = "CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceWide: clearMotion() or setTraceWide(false)";
static const char* const kWideFast =
    "CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceWideFast: clearMotion() or setTraceWideFast(false)";
static const char* const kFast = "CudaInstancedBVH: motion (setMotionKey) is not combinable with setTraceFast: clearMotion() or setTraceFast(false)";
static const char* const kWorld = "CudaInstancedBVH: motion (setMotionKey) is not combinable with setWorld: clearMotion() or clearWorld()";

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

static CameraView camera(int w, int h, const Vec3f& position, F32 halfWidth, F32 halfHeight)
{
    CameraView cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position = position;
    F32* m = cam.nscreenToWorld.m;
    m[0] = halfWidth;   m[3] = cam.position.x;
    m[5] = -halfHeight; m[7] = cam.position.y;
    m[11] = cam.position.z + 1.0f;
    m[15] = 1.0f;
    cam.cameraFar = 200.0f;
    cam.width = w;
    cam.height = h;
    return cam;
}

// every refusal of motion with another form, in today's order: the first switch that is on is the one named
static void refusalsAsToday(CudaInstancedBVH& a, RayBuffer& rays, S32 world, bool wideAccepted, const char* otherwise)
{
    Buffer ids;
    a.setTraceWide(true);
    if (wideAccepted) CHECK(refused([&] { a.traceBatch(rays, ids); }, otherwise));
    else CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kWide));
    a.setTraceWideFast(true);                        // wide and wide fast: wide is named first, unless it is accepted
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, wideAccepted ? kWideFast : kWide));
    a.setTraceWide(false);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kWideFast));
    a.setTraceFast(true);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kWideFast));
    a.setTraceWideFast(false);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kFast));
    a.setWorld(world);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kFast));
    a.setTraceFast(false);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, kWorld));
    a.setTraceWide(true);
    CHECK(refusedWith([&] { a.traceBatch(rays, ids); }, wideAccepted ? kWorld : kWide));   // a world stays refused over the wide trees
    a.setTraceWide(false);
    a.clearWorld();
}

static void cpuTests()
{
    CudaInstancedBVH a;
    CHECK(!a.getTraceWideMotion() && a.getMotionWideRefits() == 0 && a.isMotionWideStale());
    CHECK(a.getMotionWideRefitResult().numMoving == 0 && a.getMotionWideRefitResult().refit.numLeaves == 0);
    const float m[24] = {2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const float m1[24] = {2, 0, 0, 1.5f, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const S32 which[2] = {0, 1};
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)};
    Scene scene(2, tris, 4, verts);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CHECK(a.addBLAS(sah) == 0 && a.addBLAS(sah) == 1);
    a.setInstances(2, m, which);
    RayBuffer rays;
    rays.resize(64);
    // the switch alone changes nothing: without motion there is nothing to refuse
    a.setTraceWideMotion(true);
    CHECK(a.getTraceWideMotion());
    {
        Buffer ids;
        CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS"));
    }
    a.setTraceWideMotion(false);
    a.setMotionKey(2, m1);
    // off: word for word today's, in today's order
    refusalsAsToday(a, rays, 1, false, "");
    // on: setTraceWide is accepted (there is no TLAS here, and nothing is refitted without one); the others are still refused by name
    a.setTraceWideMotion(true);
    refusalsAsToday(a, rays, 1, true, "No TLAS");
    CHECK(a.getMotionRefits() == 0 && a.getMotionWideRefits() == 0);
    // without setTraceWide(true) the switch changes nothing
    {
        Buffer ids;
        CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS"));
    }
    // refitMotionWide() needs what refitWide() needs, and says so
    CHECK(refused([&] { a.refitMotionWide(); }, "widen()") && a.getMotionWideRefits() == 0 && a.getMotionRefits() == 0);
    // InstancedRenderer's switch
    InstancedRenderer r(a);
    CHECK(!r.getWideMotion());
    r.setWideMotion(true);
    CHECK(r.getWideMotion() && !r.getWide() && !r.getMotionBlur());
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the wide motion is bookkeeping only\n");
}

// traceBatch of the mirror on the wide motion path against ntr_tlas_wide_motion_refit + ntr_trace_instanced_wide_motion over buffers of
// the test's own.  expectRefit: the state is stale, and the first traceBatch refits both trees exactly once.  -> rays that hit
static int sameAsCapi(CudaInstancedBVH& a, RayBuffer& p, Buffer* times, F32 time, bool expectRefit, const char* what)
{
    const int n = p.getSize(), N = a.getNumInstances();
    CHECK(a.hasMotion() && a.getTraceWide() && a.getTraceWideMotion() && a.isMotionWideStale() == expectRefit);
    const S32 expectedWide = a.getMotionWideRefits() + (expectRefit ? 1 : 0), expectedBinary = a.getMotionRefits() + (expectRefit ? 1 : 0);
    a.setRayTimes(times);
    a.setTime(time);
    int hits = 0;
    std::vector<NtrBlasRange> ranges((size_t)a.getNumBLAS());
    std::vector<NtrWideBlasRange> wideRanges((size_t)a.getNumBLAS());
    for (S32 k = 0; k < a.getNumBLAS(); k++) { ranges[(size_t)k] = a.getBLASRange(k); wideRanges[(size_t)k] = a.getWideBLASRange(k); }
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        p.setNeedClosestHit(!anyHit);
        Buffer ids;
        p.getResultBuffer().clear(0x33);
        CHECK(a.traceBatch(p, ids) > 0.0f);
        CHECK(a.isBuilt() && a.isWide() && !a.isMotionStale() && !a.isMotionWideStale());
        CHECK(a.getMotionWideRefits() == expectedWide && a.getMotionRefits() == expectedBinary);
        std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
        // the C-ABI over copies of the mirror's refitted wide tree: the refit is idempotent, so the copies come out as they went in
        const int64_t wideBytes = a.getWideResult().nodesBytes;
        Buffer nodes, records, keys, results, cids;
        nodes.set(a.getWideTLASNodeBuffer());
        records.set(a.getWideRecordBuffer());
        keys.resizeDiscard((S64)N * 128);
        keys.clear(0xCD);
        results.resizeDiscard((S64)n * 16);
        results.clear(0x5a);
        cids.resizeDiscard((S64)n * 4);
        const NtrTlasResult& tr = a.getBuildResult();
        NtrTlasMotionRefitResult rr;
        CHECK(ntr_tlas_wide_motion_refit(N, (const NtrInstance*)a.getInstanceBuffer().getCudaPtr(),
                                         (const NtrInstance*)a.getMotionInstanceBuffer().getCudaPtr(), (int32_t)ranges.size(), ranges.data(),
                                         wideRanges.data(), a.getWidePoolNodeBuffer().getCudaPtr(), a.getWidePoolResult().nodesBytes,
                                         wideBytes ? nodes.getMutableCudaPtr() : NULL, wideBytes, tr.rootLink, records.getMutableCudaPtr(),
                                         records.getSize(), keys.getMutableCudaPtr(), keys.getSize(), NULL, &rr, NULL) == NTR_OK);
        CHECK(rr.numMoving == a.getMotionWideRefitResult().numMoving && rr.numMoving == a.getMotionRefitResult().numMoving && rr.numMoving > 0 &&
              rr.numMoving < N);
        CHECK(std::memcmp(nodes.getPtr(), a.getWideTLASNodeBuffer().getPtr(), (size_t)wideBytes) == 0);
        CHECK(std::memcmp(records.getPtr(), a.getWideRecordBuffer().getPtr(), (size_t)N * 64) == 0);
        CHECK(std::memcmp(keys.getPtr(), a.getMotionKeyBuffer().getPtr(), (size_t)N * 128) == 0);
        NtrInstanceMotion motion;
        motion.d_motionKeys = (const void*)keys.getCudaPtr();
        motion.motionKeysBytes = keys.getSize();
        motion.d_rayTimes = times ? (const float*)times->getCudaPtr() : NULL;
        motion.time = time;
        motion.pad = 0.0f;
        float seconds = 0.0f;
        CHECK(ntr_trace_instanced_wide_motion(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(), (NtrRayResult*)results.getMutableCudaPtr(),
                                              (int32_t*)cids.getMutableCudaPtr(), wideBytes ? nodes.getCudaPtr() : NULL, wideBytes, tr.rootLink,
                                              records.getCudaPtr(), N, a.getWidePoolNodeBuffer().getCudaPtr(), a.getWidePoolResult().nodesBytes,
                                              a.getPoolTriWoopBuffer().getCudaPtr(), a.getPoolTriWoopBuffer().getSize(),
                                              (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), NULL, &motion, &seconds, NULL) == NTR_OK);
        const bool same = std::memcmp(res.data(), results.getPtr(), (size_t)n * 16) == 0 && ids.getSize() == (S64)n * 4 &&
                          std::memcmp(ids.getPtr(), cids.getPtr(), (size_t)n * 4) == 0;
        if (!same) { std::printf("%s anyHit=%d: traceBatch differs from the C-ABI\n", what, anyHit); g_failed++; }
        const NtrRayResult* r = (const NtrRayResult*)res.data();
        for (int i = 0; i < n; i++) hits += r[i].id != -1 ? 1 : 0;
    }
    p.setNeedClosestHit(true);
    std::printf("%s: wide motion equals the C-ABI, %d hits, %d wide motion refit(s) so far\n", what, hits, a.getMotionWideRefits());
    return hits;
}

// What an AO frame leaves behind, copied out of the mirror
struct Frame {
    std::vector<NtrRayResult> primary, resolved, secondary;
    std::vector<S32> primaryIDs, secondaryIDs, slotToID;
    std::vector<U32> pixels;
    int selfHits, occluded;
};

template <class T>
static std::vector<T> copyOf(Buffer& b, size_t count)
{
    const T* p = (const T*)b.getPtr();
    return std::vector<T>(p, p + count);
}

static void aoFrame(InstancedRenderer& r, const CameraView& cam, int W, int H, int NS, Buffer& mat, Buffer& shaded, Frame& out)
{
    const int n = W * H, m = n * NS;
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0x5a);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch());
    CHECK(r.getBatchRays() && r.getBatchRays()->getSize() == m);
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pixels, mat, shaded);
    out.primary = copyOf<NtrRayResult>(r.getPrimaryRays().getResultBuffer(), (size_t)n);
    out.resolved = copyOf<NtrRayResult>(r.getPrimaryResolvedBuffer(), (size_t)n);
    out.primaryIDs = copyOf<S32>(r.getPrimaryInstanceIDBuffer(), (size_t)n);
    out.slotToID = copyOf<S32>(r.getPrimaryRays().getSlotToIDBuffer(), (size_t)n);
    out.secondary = copyOf<NtrRayResult>(r.getBatchResolvedBuffer(), (size_t)m);
    out.secondaryIDs = copyOf<S32>(r.getBatchInstanceIDBuffer(), (size_t)m);
    out.pixels = copyOf<U32>(pixels, (size_t)n);
    CHECK(!r.nextBatch());
    // the NS rays of primary slot i are the secondary slots [i NS, (i + 1) NS): a self hit starts on the turning cube and hits it
    out.selfHits = out.occluded = 0;
    for (int j = 0; j < m; j++) {
        if (out.secondary[(size_t)j].id < 0) continue;
        out.occluded++;
        if (out.primaryIDs[(size_t)(j / NS)] == 0 && out.primary[(size_t)(j / NS)].id >= 0 && out.secondaryIDs[(size_t)j] == 0) out.selfHits++;
    }
}

static bool sameRecord(const NtrRayResult& a, const NtrRayResult& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static void cubeFrames(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "cube_tri.bin");
    std::vector<float> vtx = load<float>(dir, "cube_pos.bin");
    std::vector<float> xf = load<float>(dir, "cube_transforms.bin");
    std::vector<float> xf1 = load<float>(dir, "cube_transforms1.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3;
    CHECK(numTris == 12 && numVerts == 8 && xf.size() == 24 && xf1.size() == 24);
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[(size_t)i] = 0xff000000u | (U32)((U32)(i + 1) * 2654435761u >> 8);
        sc[(size_t)i] = 0xff000000u | (U32)((U32)(i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);
    NtrPlocBatchMesh mesh;
    mesh.firstTri = 0;
    mesh.numTris = numTris;
    for (int q = 0; q < 3; q++) { mesh.sceneMin[q] = -0.5f; mesh.sceneMax[q] = 0.5f; }
    const S32 which[2] = {0, 0};
    CudaInstancedBVH a;
    a.buildBLASes(1, &mesh, tri, numVerts, pos);
    a.setInstances(2, xf.data(), which);
    a.build();
    a.setMotionKey(2, xf1.data());
    const int W = 64, H = 32, NS = 8, n = W * H;
    const CameraView cam = camera(W, H, Vec3f(0.5f, 1.0f, -14.0f), 0.9f, 0.45f);
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(InstancedRenderer::RayType_AO, 3.0f, NS);
    r.setMotionBlur(true, 0, 0.0f, 1.0f);
    Frame binary, wide;
    aoFrame(r, cam, W, H, NS, mat, shaded, binary);
    CHECK(a.getMotionRefits() == 1 && a.getMotionWideRefits() == 0);
    r.setWide(true);
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "setTraceWide:"));                     // without the new switch: today's refusal
    r.setWideMotion(true);
    aoFrame(r, cam, W, H, NS, mat, shaded, wide);
    CHECK(a.getMotionWideRefits() == 1 && a.isWide() && !a.isMotionWideStale() && !a.getTraceWide() && !a.getTraceWideMotion());
    // wherever the two traces' records agree, the frame is the same: resolved records, secondary records and pixels
    int primaryDiffer = 0, secondaryDiffer = 0, pixelsCompared = 0, hits = 0, moving = 0;
    for (int i = 0; i < n; i++) {
        hits += wide.primary[(size_t)i].id >= 0 ? 1 : 0;
        moving += wide.primary[(size_t)i].id >= 0 && wide.primaryIDs[(size_t)i] == 0 ? 1 : 0;
        if (!sameRecord(binary.primary[(size_t)i], wide.primary[(size_t)i]) || binary.primaryIDs[(size_t)i] != wide.primaryIDs[(size_t)i]) {
            primaryDiffer++;
            continue;
        }
        CHECK(sameRecord(binary.resolved[(size_t)i], wide.resolved[(size_t)i]) && binary.slotToID[(size_t)i] == wide.slotToID[(size_t)i]);
        bool all = true;
        for (int s = 0; s < NS; s++) {
            const size_t j = (size_t)i * NS + (size_t)s;
            // an AO ray's record is an any-hit record: the two trees may stop at different triangles, the answer hit / miss is one
            if ((binary.secondary[j].id >= 0) != (wide.secondary[j].id >= 0)) { secondaryDiffer++; all = false; }
        }
        if (!all) continue;
        pixelsCompared++;
        CHECK(binary.pixels[(size_t)binary.slotToID[(size_t)i]] == wide.pixels[(size_t)wide.slotToID[(size_t)i]]);
    }
    CHECK(hits > 0 && moving > 0 && wide.occluded > 0);
    CHECK(primaryDiffer * 100 <= n && secondaryDiffer * 100 <= n * NS);                    // the trees differ in ties and roundings only
    CHECK(binary.selfHits == 0 && wide.selfHits == 0);
    std::printf("cube AO frame %dx%d, %d samples, blurred: wide against binary: %d of %d primary records differ, %d of %d AO rays in hit or miss, "
                "%d pixels compared and equal; %d primary hits, %d on the turning cube; AO rays that hit the cube they start from: binary %d, wide %d\n",
                W, H, NS, primaryDiffer, n, secondaryDiffer, n * NS, pixelsCompared, hits, moving, binary.selfHits, wide.selfHits);
}

static void gpuTests(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
    std::vector<float> vtx = load<float>(dir, "pos.bin");
    std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
    std::vector<float> xf = load<float>(dir, "transforms.bin");
    std::vector<float> xf1 = load<float>(dir, "transforms1.bin");
    std::vector<S32> which = load<S32>(dir, "blas.bin");
    std::vector<S32> worldOf = load<S32>(dir, "world.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size(), world = worldOf[0];
    CHECK(numTris > 0 && B == 3 && N == 32 && (S32)xf.size() == 12 * N && xf1.size() == xf.size() && world >= 0 && world < B);
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12);

    CudaInstancedBVH a;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    const int W = 64, H = 32, n = W * H;
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.beginFrame(camera(W, H, Vec3f(0.5f, 0.75f, -34.0f), 0.4f, 0.2f), W, H);
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);
    std::vector<float> t((size_t)n);
    for (int i = 0; i < n; i++) t[(size_t)i] = (float)i / (float)(n - 1);
    t[1] = -1.0f; t[2] = 2.0f; t[3] = 0.0f / 0.0f;
    Buffer times(t.data(), (S64)n * 4);
    Buffer ids;

    a.setMotionKey(N, xf1.data());
    // the binary motion launch, for "without setTraceWide(true) the switch changes nothing"
    a.setRayTimes(&times);
    a.traceBatch(p, ids);
    CHECK(a.getMotionRefits() == 1 && a.getMotionWideRefits() == 0);
    std::vector<U8> binaryRecords((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
    a.setTraceWideMotion(true);
    p.getResultBuffer().clear(0x33);
    a.traceBatch(p, ids);
    CHECK(a.getMotionRefits() == 1 && a.getMotionWideRefits() == 0);
    CHECK(std::memcmp(binaryRecords.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);

    // the wide motion path: without a widen() the refit it needs says so
    a.setTraceWide(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "widen()") && a.getMotionWideRefits() == 0);
    CHECK(refused([&] { a.refitMotionWide(); }, "widen()"));
    a.widen();
    CHECK(a.isWide() && !a.isMotionStale() && a.isMotionWideStale());                    // the wide records have no moving flags yet
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "widen, per-ray times") > 0 && a.getMotionWideRefits() == 1);
    CHECK(sameAsCapi(a, p, NULL, 0.5f, false, "scalar time 0.5") > 0 && a.getMotionWideRefits() == 1);
    // staleness: every call that writes records or boxes of either tree
    a.setMotionKey(N, xf1.data());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "setMotionKey") > 0 && a.getMotionWideRefits() == 2);
    a.refit();
    CHECK(a.isMotionStale() && a.isMotionWideStale() && !a.isWide());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "refit") > 0 && a.getMotionWideRefits() == 3);
    a.refitWide();
    CHECK(a.isWide() && a.isMotionWideStale());
    CHECK(sameAsCapi(a, p, NULL, 0.8125f, true, "refitWide, scalar time") > 0 && a.getMotionWideRefits() == 4);
    a.widen();
    CHECK(!a.isMotionStale() && a.isMotionWideStale());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "widen again") > 0 && a.getMotionWideRefits() == 5);
    std::vector<float> moved(xf);
    for (S32 i = 0; i < N; i++) moved[12 * (size_t)i + 3] += 0.25f * (float)(i % 5);
    a.setInstances(N, moved.data(), which.data());
    CHECK(a.hasMotion() && a.isMotionWideStale() && !a.isBuilt());
    CHECK(refused([&] { a.traceBatch(p, ids); }, "No TLAS") && a.getMotionWideRefits() == 5);
    a.refit();
    a.refitMotionWide();                             // explicitly: the next traceBatch refits nothing
    CHECK(a.isBuilt() && a.isWide() && !a.isMotionStale() && !a.isMotionWideStale() && a.getMotionWideRefits() == 6);
    CHECK(sameAsCapi(a, p, &times, 0.0f, false, "setInstances + refit + refitMotionWide") > 0 && a.getMotionWideRefits() == 6);
    a.build();                                       // another topology: the wide tree has to be widened again
    CHECK(a.isMotionWideStale());
    CHECK(refused([&] { a.traceBatch(p, ids); }, "widen()") && a.getMotionWideRefits() == 6);
    a.widen();
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "build + widen") > 0 && a.getMotionWideRefits() == 7);
    // FAST and a world are still refused by name
    a.setRayTimes(NULL);
    a.setTraceWideFast(true);
    CHECK(refusedWith([&] { a.traceBatch(p, ids); }, kWideFast));
    a.setTraceWideFast(false);
    a.setTraceFast(true);
    CHECK(refusedWith([&] { a.traceBatch(p, ids); }, kFast));
    a.setTraceFast(false);
    a.setWorld(world);
    CHECK(refusedWith([&] { a.traceBatch(p, ids); }, kWorld));
    a.clearWorld();
    // the switch off again: today's refusal
    a.setTraceWideMotion(false);
    CHECK(refusedWith([&] { a.traceBatch(p, ids); }, kWide) && a.getMotionWideRefits() == 7);

    cubeFrames(dir);
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
    if (g_failed) { std::printf("instanced_wide_motion_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_wide_motion_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
