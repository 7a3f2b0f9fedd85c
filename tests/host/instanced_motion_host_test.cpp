// instanced_motion_host_test.cpp -- the host mirror's motion blur (CudaInstancedBVH::setMotionKey / refitMotion / setRayTimes / setTime;
// DESIGN.md 6aa).  `cpu`: the switches, the staleness rule and the refusals of the wide, FAST and world forms with motion, without a
// device.  `gpu <dir>`: the scene of the seeded trace's tests, which the test driver writes into <dir>, with a second key; through a
// build / refit / refitMotion loop refitMotion() + traceBatch with times equal ntr_tlas_motion_refit + ntr_trace_instanced_motion on
// buffers of the test's own byte for byte, closest hit and any hit, per-ray times and the scalar; every step that writes records marks
// the motion refit stale and the next traceBatch refits exactly once.  Compiled with plain g++ against libntrace_amd.so.
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
    CudaInstancedBVH a;
    CHECK(!a.hasMotion() && a.isMotionStale() && a.getMotionRefits() == 0);
    const float m[24] = {2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const float m1[24] = {2, 0, 0, 1.5f, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const S32 which[3] = {0, 1, 0};
    CHECK(refused([&] { a.setMotionKey(2, m1); }, "setInstances 0"));                        // no instances yet
    CHECK(refused([&] { a.refitMotion(); }, "no motion key"));
    // a pool of two host-built trees
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)};
    Scene scene(2, tris, 4, verts);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CHECK(a.addBLAS(sah) == 0 && a.addBLAS(sah) == 1);
    a.setInstances(2, m, which);
    CHECK(refused([&] { a.setMotionKey(3, m1); }, "names 3 instances") && refused([&] { a.setMotionKey(2, NULL); }, "no motion key") && !a.hasMotion());
    a.setMotionKey(2, m1);
    CHECK(a.hasMotion() && a.isMotionStale() && a.getMotionInstanceBuffer().getSize() == 2 * (S64)sizeof(NtrInstance));
    {
        const NtrInstance* k1 = (const NtrInstance*)a.getMotionInstanceBuffer().getPtr();
        CHECK(k1[0].objectToWorld[3] == 1.5f && k1[1].objectToWorld[3] == -4.0f && k1[0].worldToObject[0] == 0.0f);
    }
    CHECK(refused([&] { a.refitMotion(); }, "No TLAS") && a.getMotionRefits() == 0);
    RayBuffer rays;
    Buffer ids;
    rays.resize(64);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS") && a.getMotionRefits() == 0);   // nothing is refitted without a TLAS
    // not combinable: each switch is named, none is ignored, and the refusal comes before anything else is looked at
    a.setTraceWide(true);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "setTraceWide:"));
    a.setTraceWide(false);
    a.setTraceWideFast(true);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "setTraceWideFast"));
    a.setTraceWideFast(false);
    a.setTraceFast(true);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "setTraceFast"));
    a.setTraceFast(false);
    a.setWorld(1);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "setWorld"));
    a.clearMotion();
    CHECK(!a.hasMotion() && a.getMotionInstanceBuffer().getSize() == 0);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS"));                             // without motion the world is fine
    a.clearWorld();
    // the same count keeps key 1, another count clears it
    a.setMotionKey(2, m1);
    a.setInstances(2, m, which);
    CHECK(a.hasMotion() && a.isMotionStale());
    const float m3[36] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 5, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, -5, 0, 1, 0, 0, 0, 0, 1, 0};
    a.setInstances(3, m3, which);
    CHECK(!a.hasMotion());
    Buffer small;
    small.resizeDiscard(3 * (S64)sizeof(NtrInstance) - 4);
    CHECK(refused([&] { a.setMotionKeyDevice(3, small); }, "smaller than its count") && !a.hasMotion());
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the motion is bookkeeping only\n");
}

// traceBatch of the mirror against ntr_tlas_motion_refit + ntr_trace_instanced_motion over buffers of the test's own: the mirror's tree
// as it is before its motion refit is copied, refitted here, and traced.  -> rays that hit
static int sameAsCapi(CudaInstancedBVH& a, RayBuffer& p, Buffer* times, F32 time, bool expectRefit, const char* what)
{
    const int n = p.getSize(), N = a.getNumInstances();
    CHECK(a.hasMotion() && a.isMotionStale() == expectRefit);
    const S32 expected = a.getMotionRefits() + (expectRefit ? 1 : 0);   // stale: the first traceBatch refits, once
    a.setRayTimes(times);
    a.setTime(time);
    int hits = 0;
    std::vector<NtrBlasRange> ranges((size_t)a.getNumBLAS());
    for (S32 k = 0; k < a.getNumBLAS(); k++) ranges[(size_t)k] = a.getBLASRange(k);
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        p.setNeedClosestHit(!anyHit);
        Buffer ids;
        p.getResultBuffer().clear(0x33);
        CHECK(a.traceBatch(p, ids) > 0.0f);
        CHECK(!a.isMotionStale() && a.getMotionRefits() == expected);
        std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
        // the C-ABI over copies: the motion refit of the mirror's refitted tree changes no byte (it is idempotent), so the copies start
        // from the mirror's buffers
        Buffer nodes, records, keys, results, cids;
        nodes.set(a.getTLASNodeBuffer());
        records.set(a.getRecordBuffer());
        keys.resizeDiscard((S64)N * 128);
        keys.clear(0xCD);
        results.resizeDiscard((S64)n * 16);
        results.clear(0x5a);
        cids.resizeDiscard((S64)n * 4);
        const NtrTlasResult& tr = a.getBuildResult();
        NtrTlasMotionRefitResult rr;
        CHECK(ntr_tlas_motion_refit(N, (const NtrInstance*)a.getInstanceBuffer().getCudaPtr(), (const NtrInstance*)a.getMotionInstanceBuffer().getCudaPtr(),
                                    (int32_t)ranges.size(), ranges.data(), a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(),
                                    tr.nodesBytes ? nodes.getMutableCudaPtr() : NULL, tr.nodesBytes, tr.rootLink, records.getMutableCudaPtr(),
                                    records.getSize(), keys.getMutableCudaPtr(), keys.getSize(), NULL, &rr, NULL) == NTR_OK);
        CHECK(rr.numMoving == a.getMotionRefitResult().numMoving && rr.numMoving > 0 && rr.numMoving < N);
        CHECK(std::memcmp(nodes.getPtr(), a.getTLASNodeBuffer().getPtr(), (size_t)tr.nodesBytes) == 0);
        CHECK(std::memcmp(records.getPtr(), a.getRecordBuffer().getPtr(), (size_t)N * 64) == 0);
        CHECK(std::memcmp(keys.getPtr(), a.getMotionKeyBuffer().getPtr(), (size_t)N * 128) == 0);
        NtrInstanceMotion motion;
        motion.d_motionKeys = (const void*)keys.getCudaPtr();
        motion.motionKeysBytes = keys.getSize();
        motion.d_rayTimes = times ? (const float*)times->getCudaPtr() : NULL;
        motion.time = time;
        motion.pad = 0.0f;
        float seconds = 0.0f;
        CHECK(ntr_trace_instanced_motion(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(), (NtrRayResult*)results.getMutableCudaPtr(),
                                         (int32_t*)cids.getMutableCudaPtr(), nodes.getCudaPtr(), tr.nodesBytes, tr.rootLink, records.getCudaPtr(), N,
                                         a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(), a.getPoolTriWoopBuffer().getCudaPtr(),
                                         a.getPoolTriWoopBuffer().getSize(), (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), NULL, &motion,
                                         &seconds, NULL) == NTR_OK);
        const bool same = std::memcmp(res.data(), results.getPtr(), (size_t)n * 16) == 0 && ids.getSize() == (S64)n * 4 &&
                          std::memcmp(ids.getPtr(), cids.getPtr(), (size_t)n * 4) == 0;
        if (!same) { std::printf("%s anyHit=%d: traceBatch differs from the C-ABI\n", what, anyHit); g_failed++; }
        const NtrRayResult* r = (const NtrRayResult*)res.data();
        for (int i = 0; i < n; i++) hits += r[i].id != -1 ? 1 : 0;
    }
    p.setNeedClosestHit(true);
    std::printf("%s: motion equals the C-ABI, %d hits, %d motion refit(s) so far\n", what, hits, a.getMotionRefits());
    return hits;
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
    r.beginFrame(camera(W, H), W, H);
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);
    std::vector<float> t((size_t)n);
    for (int i = 0; i < n; i++) t[(size_t)i] = (float)i / (float)(n - 1);
    t[1] = -1.0f; t[2] = 2.0f; t[3] = 0.0f / 0.0f;
    Buffer times(t.data(), (S64)n * 4);

    // the static trace before any motion, for "the poses differ"
    Buffer ids0;
    a.traceBatch(p, ids0);
    std::vector<U8> still((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);

    a.setMotionKey(N, xf1.data());
    CHECK(a.isBuilt() && a.isMotionStale());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "build, per-ray times") > 0 && a.getMotionRefits() == 1);
    {
        Buffer ids;
        a.traceBatch(p, ids);
        CHECK(std::memcmp(still.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) != 0);          // something moved in the picture
    }
    CHECK(sameAsCapi(a, p, NULL, 0.5f, false, "scalar time 0.5") > 0 && a.getMotionRefits() == 1);
    a.setTime(0.0f);
    a.setRayTimes(NULL);
    {
        Buffer ids;
        a.traceBatch(p, ids);
        CHECK(std::memcmp(still.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);          // time 0 is key 0
    }
    // refit() clears the moving flags: stale, and the next traceBatch refits once
    a.refit();
    CHECK(a.hasMotion() && a.isMotionStale());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, "refit") > 0 && a.getMotionRefits() == 2);
    // the instances move: setInstances + refit, then an explicit refitMotion
    std::vector<float> moved(xf);
    for (S32 i = 0; i < N; i++) moved[12 * (size_t)i + 3] += 0.25f * (float)(i % 5);
    a.setInstances(N, moved.data(), which.data());
    CHECK(a.hasMotion() && a.isMotionStale() && !a.isBuilt());
    CHECK(refused([&] { a.refitMotion(); }, "No TLAS"));
    a.refit();
    a.refitMotion();
    CHECK(!a.isMotionStale() && a.getMotionRefits() == 3);
    CHECK(sameAsCapi(a, p, &times, 0.0f, false, "setInstances + refit + refitMotion") > 0 && a.getMotionRefits() == 3);
    // key 1 from a device buffer of NtrInstance: the same bytes as the host form
    {
        Buffer k1;
        k1.set(a.getMotionInstanceBuffer());
        a.setMotionKeyDevice(N, k1);
        CHECK(a.isMotionStale());
        CHECK(sameAsCapi(a, p, &times, 0.0f, true, "setMotionKeyDevice") > 0 && a.getMotionRefits() == 4);
    }
    a.build();
    CHECK(a.isMotionStale());
    CHECK(sameAsCapi(a, p, NULL, 0.8125f, true, "build again, scalar time") > 0 && a.getMotionRefits() == 5);
    // a times buffer that is too short, and the forms that are not combinable, on a built tree
    Buffer shortTimes(t.data(), (S64)n * 4 - 4);
    a.setRayTimes(&shortTimes);
    Buffer ids;
    CHECK(refused([&] { a.traceBatch(p, ids); }, "fewer than"));
    a.setRayTimes(NULL);
    a.setWorld(world);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "setWorld"));
    a.clearWorld();
    a.setTraceFast(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "setTraceFast"));
    a.setTraceFast(false);
    // clearMotion: the static trace again, over boxes that still bound the sweep -- the same records as after a plain refit
    a.clearMotion();
    a.traceBatch(p, ids);
    std::vector<U8> swept((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
    a.refit();
    a.traceBatch(p, ids);
    CHECK(std::memcmp(swept.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);
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
    if (g_failed) { std::printf("instanced_motion_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_motion_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
