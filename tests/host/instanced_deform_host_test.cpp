// instanced_deform_host_test.cpp -- the host mirror's deforming BLASes (CudaInstancedBVH::refitBLASesMotion / clearDeform / hasDeform /
// getDeformRefitResult).  `cpu`: the refusals that need no device.  `gpu <dir>`: the scene of the seeded trace's tests,
// which the test driver writes into <dir>, with a second key of the vertices and of the transforms; refitBLASesMotion + the lazy
// refitMotion() + traceBatch equal ntr_tlas_deform_refit + ntr_trace_instanced_deform on buffers of the test's own byte for byte, closest
// hit and any hit; hasDeform() drops after refitBLASes and optimizeBLASes; every form that is not combinable is refused by name.  The
// buffers and the records of one traced batch are written back into <dir>: the driver runs the numpy rule over them.  Compiled with plain
// g++ against libntrace_amd.so.
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

static void dump(const std::string& dir, const char* name, const void* p, size_t bytes)
{
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::printf("cannot write %s\n", path.c_str()); g_failed++; }
    if (f) std::fclose(f);
}
static void dump(const std::string& dir, const char* name, Buffer& b) { dump(dir, name, b.getPtr(), (size_t)b.getSize()); }

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
    CHECK(!a.hasDeform() && a.getDeformRefitResult().numDeforming == 0);
    Buffer tri, pos;
    tri.resizeDiscard(12);
    pos.resizeDiscard(36);
    CHECK(refused([&] { a.refitBLASesMotion(tri, 3, pos, pos); }, "no BLASes to refit"));
    // a pool of two host-built trees: they have no mesh here and cannot deform
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)};
    Scene scene(2, tris, 4, verts);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CHECK(a.addBLAS(sah) == 0 && a.addBLAS(sah) == 1);
    CHECK(refused([&] { a.refitBLASesMotion(tri, 3, pos, pos); }, "came through addBLAS") && !a.hasDeform());
    const S32 bad[1] = {2};
    CHECK(refused([&] { a.refitBLASesMotion(tri, 3, pos, pos, bad, 1); }, "BLAS index 2 outside"));
    Buffer small;
    small.resizeDiscard(8);
    CHECK(refused([&] { a.refitBLASesMotion(tri, 3, pos, small); }, "bad mesh buffers"));
    CHECK(refused([&] { a.refitMotion(); }, "no motion key"));           // nothing deforms: refitMotion is the motion one
    a.clearDeform();
    CHECK(!a.hasDeform());
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the deformation is bookkeeping only\n");
}

// traceBatch of the mirror against ntr_tlas_deform_refit + ntr_trace_instanced_deform over buffers of the test's own: the mirror's tree is
// copied, refitted here (the refit of a refitted tree changes no byte), and traced.  -> rays that hit
static int sameAsCapi(CudaInstancedBVH& a, RayBuffer& p, Buffer* times, F32 time, bool expectRefit, S32 deforming, const char* what,
                      const std::string* dumpDir = NULL)
{
    const int n = p.getSize(), N = a.getNumInstances();
    CHECK(a.hasDeform() && a.isMotionStale() == expectRefit);
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
        Buffer nodes, records, keys, results, cids;
        nodes.set(a.getTLASNodeBuffer());
        records.set(a.getRecordBuffer());
        keys.resizeDiscard((S64)N * 128);
        keys.clear(0xCD);
        results.resizeDiscard((S64)n * 16);
        results.clear(0x5a);
        cids.resizeDiscard((S64)n * 4);
        const NtrTlasResult& tr = a.getBuildResult();
        Buffer& inst1 = a.hasMotion() ? a.getMotionInstanceBuffer() : a.getInstanceBuffer();
        NtrTlasDeformRefitResult rr;
        CHECK(ntr_tlas_deform_refit(N, (const NtrInstance*)a.getInstanceBuffer().getCudaPtr(), (const NtrInstance*)inst1.getCudaPtr(),
                                    (int32_t)ranges.size(), ranges.data(), a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNode1Buffer().getCudaPtr(),
                                    a.getPoolNodeBuffer().getSize(), (const uint32_t*)a.getBLASDeformingBuffer().getCudaPtr(),
                                    tr.nodesBytes ? nodes.getMutableCudaPtr() : NULL, tr.nodesBytes, tr.rootLink, records.getMutableCudaPtr(),
                                    records.getSize(), keys.getMutableCudaPtr(), keys.getSize(), NULL, &rr, NULL) == NTR_OK);
        CHECK(rr.numDeforming == a.getDeformRefitResult().numDeforming && rr.numDeforming == deforming);
        CHECK(rr.motion.numMoving == a.getMotionRefitResult().numMoving && (rr.motion.numMoving > 0) == a.hasMotion());
        CHECK(std::memcmp(nodes.getPtr(), a.getTLASNodeBuffer().getPtr(), (size_t)tr.nodesBytes) == 0);
        CHECK(std::memcmp(records.getPtr(), a.getRecordBuffer().getPtr(), (size_t)N * 64) == 0);
        CHECK(std::memcmp(keys.getPtr(), a.getMotionKeyBuffer().getPtr(), (size_t)N * 128) == 0);
        NtrInstanceMotion motion;
        motion.d_motionKeys = (const void*)keys.getCudaPtr();
        motion.motionKeysBytes = keys.getSize();
        motion.d_rayTimes = times ? (const float*)times->getCudaPtr() : NULL;
        motion.time = time;
        motion.pad = 0.0f;
        const NtrInstanceDeform df = {a.getPoolNode1Buffer().getCudaPtr(), a.getPoolVertRowBuffer(0).getCudaPtr(), a.getPoolVertRowBuffer(1).getCudaPtr()};
        float seconds = 0.0f;
        CHECK(ntr_trace_instanced_deform(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(), (NtrRayResult*)results.getMutableCudaPtr(),
                                         (int32_t*)cids.getMutableCudaPtr(), nodes.getCudaPtr(), tr.nodesBytes, tr.rootLink, records.getCudaPtr(), N,
                                         a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(), a.getPoolTriWoopBuffer().getCudaPtr(),
                                         a.getPoolTriWoopBuffer().getSize(), (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), NULL, &motion,
                                         &df, &seconds, NULL) == NTR_OK);
        const bool same = std::memcmp(res.data(), results.getPtr(), (size_t)n * 16) == 0 && ids.getSize() == (S64)n * 4 &&
                          std::memcmp(ids.getPtr(), cids.getPtr(), (size_t)n * 4) == 0;
        if (!same) { std::printf("%s anyHit=%d: traceBatch differs from the C-ABI\n", what, anyHit); g_failed++; }
        const NtrRayResult* r = (const NtrRayResult*)res.data();
        for (int i = 0; i < n; i++) hits += r[i].id != -1 ? 1 : 0;
        if (dumpDir && !anyHit) {   // what the numpy rule needs to trace the same batch
            dump(*dumpDir, "out_tlas.bin", a.getTLASNodeBuffer());
            dump(*dumpDir, "out_records.bin", a.getRecordBuffer());
            dump(*dumpDir, "out_keys.bin", a.getMotionKeyBuffer());
            dump(*dumpDir, "out_nodes.bin", a.getPoolNodeBuffer());
            dump(*dumpDir, "out_nodes1.bin", a.getPoolNode1Buffer());
            dump(*dumpDir, "out_woop.bin", a.getPoolTriWoopBuffer());
            dump(*dumpDir, "out_index.bin", a.getPoolTriIndexBuffer());
            dump(*dumpDir, "out_vrows0.bin", a.getPoolVertRowBuffer(0));
            dump(*dumpDir, "out_vrows1.bin", a.getPoolVertRowBuffer(1));
            dump(*dumpDir, "out_rays.bin", p.getRayBuffer());
            dump(*dumpDir, "out_results.bin", res.data(), res.size());
            dump(*dumpDir, "out_ids.bin", ids);
            if (times) dump(*dumpDir, "out_times.bin", *times);
            dump(*dumpDir, "out_ranges.bin", ranges.data(), ranges.size() * sizeof(NtrBlasRange));
        }
    }
    p.setNeedClosestHit(true);
    std::printf("%s: deform equals the C-ABI, %d hits, %d motion refit(s) so far\n", what, hits, a.getMotionRefits());
    return hits;
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
    std::vector<S32> worldOf = load<S32>(dir, "world.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size(), world = worldOf[0];
    CHECK(numTris > 0 && B == 3 && N == 32 && (S32)xf.size() == 12 * N && xf1.size() == xf.size() && vtx1.size() == vtx.size());
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12), pos1(vtx1.data(), (S64)numVerts * 12);

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
    S32 perBlas[3] = {0, 0, 0};
    for (S32 i = 0; i < N; i++) perBlas[which[(size_t)i]]++;

    Buffer ids0;
    a.traceBatch(p, ids0);
    std::vector<U8> still((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);

    // BLAS 1 deforms, no instance moves: key 0 is passed twice.  The pool's key 0 was refitted, so the TLAS is stale until refit()
    const S32 one[1] = {1};
    a.refitBLASesMotion(tri, numVerts, pos, pos1, one, 1);
    CHECK(a.hasDeform() && !a.isBuilt() && !a.hasMotion());
    Buffer ids;
    CHECK(refused([&] { a.traceBatch(p, ids); }, "No TLAS"));
    a.refit();
    CHECK(a.isBuilt() && a.isMotionStale() && a.hasDeform());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, perBlas[1], "one BLAS deforms, nothing moves") > 0 && a.getMotionRefits() == 1);
    a.setRayTimes(NULL);
    a.setTime(0.5f);
    a.traceBatch(p, ids);
    CHECK(std::memcmp(still.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) != 0);              // something deformed in the picture
    a.setTime(0.0f);
    a.traceBatch(p, ids);
    CHECK(std::memcmp(still.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);              // time 0 is key 0
    // the instances move too: the four-box leaves
    a.setMotionKey(N, xf1.data());
    CHECK(a.isMotionStale() && a.hasDeform());
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, perBlas[1], "and the instances move", &dir) > 0 && a.getMotionRefits() == 2);
    CHECK(sameAsCapi(a, p, NULL, 0.8125f, false, perBlas[1], "scalar time") > 0 && a.getMotionRefits() == 2);
    // a second call keeps the first one's BLAS deforming
    const S32 two[1] = {2};
    a.refitBLASesMotion(tri, numVerts, pos, pos1, two, 1);
    CHECK(a.hasDeform() && !a.isBuilt());
    a.refit();
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, perBlas[1] + perBlas[2], "a second BLAS deforms") > 0 && a.getMotionRefits() == 3);
    // every form that is not combinable is refused by name, on a built tree
    a.setTraceWideMotion(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "not combinable with setTraceWideMotion"));
    a.setTraceWideMotion(false);
    a.setTraceWide(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "not combinable with setTraceWide:"));
    a.setTraceWide(false);
    a.clearMotion();
    a.setTraceWideFast(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "are not combinable with setTraceWideFast"));
    a.setTraceWideFast(false);
    a.setTraceFast(true);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "are not combinable with setTraceFast"));
    a.setTraceFast(false);
    a.setWorld(world);
    CHECK(refused([&] { a.traceBatch(p, ids); }, "are not combinable with setWorld"));
    a.clearWorld();
    r.setMotionBlur(true, 7u, 0.0f, 1.0f);
    CHECK(refused([&] { r.beginFrame(camera(W, H), W, H); }, "not combinable with deforming BLASes"));
    r.setMotionBlur(false, 7u, 0.0f, 1.0f);
    CHECK(a.hasDeform());
    // a plain refit of the pool leaves the second key stale: hasDeform() drops and the scene is key 0's; so does an optimize
    a.refitBLASes(tri, numVerts, pos);
    CHECK(!a.hasDeform() && !a.isBuilt());
    a.refit();
    a.setTime(0.5f);
    a.traceBatch(p, ids);
    CHECK(std::memcmp(still.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);              // frozen at key 0 whatever the time
    a.refitBLASesMotion(tri, numVerts, pos, pos1);                                                    // all of them
    CHECK(a.hasDeform());
    a.optimizeBLASes();
    CHECK(!a.hasDeform());
    a.refitBLASesMotion(tri, numVerts, pos, pos1);
    a.refit();
    CHECK(sameAsCapi(a, p, &times, 0.0f, true, N, "every BLAS deforms") > 0);
    a.clearDeform();
    CHECK(!a.hasDeform() && a.isBuilt() && a.isMotionStale());
    a.setTime(0.5f);
    a.traceBatch(p, ids);                                                                             // the static trace over swept boxes
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
    if (g_failed) { std::printf("instanced_deform_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_deform_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
