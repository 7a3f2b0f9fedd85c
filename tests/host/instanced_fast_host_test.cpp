// instanced_fast_host_test.cpp -- the host mirror's FAST switch (CudaInstancedBVH::setTraceFast, InstancedRenderer::setFast; DESIGN.md
// 6w).  `cpu`: the switch and the staleness flag without a device.  `gpu <dir>`: the scene of the seeded trace's tests, which the test
// driver writes into <dir>; through a build / refit / refitBLASes / optimizeBLASes / setWorld / clearWorld loop every step marks the
// flags stale, the next fast traceBatch validates exactly once and the one after it not at all, and traceBatch with the switch on equals
// traceBatch with it off byte for byte, closest hit and any hit, with and without masks and a world; a vertex moved to 2^70 takes
// FASTDIV from both levels and changes no record; the wide path ignores the switch; primary and AO frames of InstancedRenderer with
// setFast(true) equal the frames without it word for word.  Compiled with plain g++ against libntrace_amd.so.
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

// a pinhole camera on the -z side looking along +z: nscreen (nx, ny, 0, 1) -> a world point one unit in front of the eye
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
    CHECK(!a.getTraceFast() && a.isFastFlagsStale() && a.getFastValidations() == 0);
    a.setTraceFast(true);
    CHECK(a.getTraceFast() && a.isFastFlagsStale());
    a.setTraceFast(false);
    CHECK(!a.getTraceFast());
    U32 t = 7, p = 7;
    CHECK(refused([&] { a.getFastFlags(t, p); }, "No TLAS") && t == 7 && p == 7);
    RayBuffer rays;
    Buffer ids;
    rays.resize(64);
    a.setTraceFast(true);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS") && a.getFastValidations() == 0);   // nothing is validated without a TLAS
    InstancedRenderer r(a);
    CHECK(!r.getFast());
    r.setFast(true);
    CHECK(r.getFast() && a.getTraceFast());
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the switch is bookkeeping only\n");
}

struct Frame {
    std::vector<U8>  primary;       // resolved primary records
    std::vector<U32> pixels;
    std::vector<U8>  aoHit;         // per AO slot, in batch order: the record is a hit
    int hits;
};

static Frame render(CudaInstancedBVH& bvh, Buffer& tri, S32 numVerts, Buffer& pos, Buffer& mat, Buffer& shaded, InstancedRenderer::RayType type, bool fast,
                    bool wide, int W, int H, int NS)
{
    Frame f;
    const int n = W * H;
    InstancedRenderer r(bvh);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(type, 3.0f, NS);
    r.setFast(fast);
    r.setWide(wide);
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0);
    r.beginFrame(camera(W, H), W, H);
    while (r.nextBatch()) {
        CHECK(r.traceBatch() > 0.0f);
        r.updateResult(pixels, mat, shaded);
        if (type != InstancedRenderer::RayType_Primary) {
            const S32 k = r.getBatchRays()->getSize();
            const NtrRayResult* res = (const NtrRayResult*)r.getBatchResolvedBuffer().getPtr();
            for (S32 i = 0; i < k; i++) f.aoHit.push_back(res[i].id != -1 ? 1 : 0);
        }
    }
    const U8* p = (const U8*)r.getPrimaryResolvedBuffer().getPtr();
    f.primary.assign(p, p + (size_t)n * 16);
    const U32* px = (const U32*)pixels.getPtr();
    f.pixels.assign(px, px + n);
    f.hits = r.getTotalNumRays();
    return f;
}

// traceBatch with the switch on against traceBatch with it off on the same object: records and instance ids, both hit modes, two ray
// masks.  The first fast trace after a step that rewrote boxes validates, the later ones do not.  -> rays that hit
static int sameAsPlain(CudaInstancedBVH& a, RayBuffer& p, const char* what)
{
    const int n = p.getSize();
    int hits = 0;
    CHECK(a.isFastFlagsStale());
    const S32 before = a.getFastValidations();
    for (int anyHit = 0; anyHit < 2; anyHit++)
        for (U32 rayMask : {0xFFFFFFFFu, 2u}) {
            p.setNeedClosestHit(!anyHit);
            Buffer idsFast, idsPlain;
            a.setTraceFast(true);
            p.getResultBuffer().clear(0x33);
            CHECK(a.traceBatch(p, idsFast, rayMask) > 0.0f);
            CHECK(!a.isFastFlagsStale() && a.getFastValidations() == before + 1);
            std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
            a.setTraceFast(false);
            p.getResultBuffer().clear(0x5a);
            CHECK(a.traceBatch(p, idsPlain, rayMask) > 0.0f);
            const bool same = std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0 &&
                              idsFast.getSize() == (S64)n * 4 && std::memcmp(idsFast.getPtr(), idsPlain.getPtr(), (size_t)n * 4) == 0;
            if (!same) { std::printf("%s anyHit=%d rayMask=%08x: fast differs from plain\n", what, anyHit, rayMask); g_failed++; }
            const NtrRayResult* r = (const NtrRayResult*)res.data();
            for (int i = 0; i < n; i++) hits += r[i].id != -1 ? 1 : 0;
        }
    p.setNeedClosestHit(true);
    std::printf("%s: fast equals plain, %d hits, %d validation(s) so far\n", what, hits, a.getFastValidations());
    return hits;
}

static void gpuTests(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
    std::vector<float> vtx = load<float>(dir, "pos.bin");
    std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
    std::vector<float> xf = load<float>(dir, "transforms.bin");
    std::vector<S32> which = load<S32>(dir, "blas.bin");
    std::vector<S32> worldOf = load<S32>(dir, "world.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size(), world = worldOf[0];
    CHECK(numTris > 0 && B == 3 && N == 32 && (S32)xf.size() == 12 * N && world >= 0 && world < B);
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[i] = 0xff000000u | (U32)(i * 2654435761u >> 8);
        sc[i] = 0xff000000u | (U32)((i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);

    CudaInstancedBVH a;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    CHECK(a.isFastFlagsStale() && a.getFastValidations() == 0);
    const int W = 64, H = 32, NS = 4, n = W * H;
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.beginFrame(camera(W, H), W, H);                                                       // (not fast: nothing is validated)
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n && a.getFastValidations() == 0 && a.isFastFlagsStale());

    CHECK(sameAsPlain(a, p, "build") > 0);
    U32 tf = 0, pf = 0;
    a.getFastFlags(tf, pf);                                                                 // current: no further validation
    std::printf("granted flags after build: top level %u, pool %u\n", tf, pf);
    CHECK(a.getFastValidations() == 1 && tf == 15u && (pf & NTR_BVH_FASTDIV) != 0);
    const U32 poolBuilt = pf;
    // masks are not geometry: nothing goes stale
    std::vector<U32> masks((size_t)N);
    for (S32 i = 0; i < N; i++) masks[i] = (i % 3 == 0) ? 0x80000001u : (i % 3 == 1 ? 2u : 3u);
    a.setInstanceMasks(masks.data());
    CHECK(!a.isFastFlagsStale());
    // the instances move: setInstances alone rewrites no node box, refit() does
    std::vector<float> moved(xf);
    for (S32 i = 0; i < N; i++) moved[12 * (size_t)i + 3] += 0.25f * (float)(i % 5);
    a.setInstances(N, moved.data(), which.data());
    CHECK(!a.isFastFlagsStale() && !a.isBuilt());
    a.refit();
    CHECK(sameAsPlain(a, p, "refit, masked") > 0 && a.getFastValidations() == 2);
    a.setInstanceMasks(NULL);
    // the vertices move
    std::vector<float> v2(vtx);
    for (size_t i = 0; i < v2.size(); i++) v2[i] *= 1.0f + 0.05f * (float)(i % 7) / 7.0f;
    Buffer pos2(v2.data(), (S64)numVerts * 12);
    a.refitBLASes(tri, numVerts, pos2);
    CHECK(a.isFastFlagsStale());
    a.refit();
    CHECK(sameAsPlain(a, p, "refitBLASes + refit") > 0 && a.getFastValidations() == 3);
    a.optimizeBLASes();
    CHECK(a.isBuilt());
    CHECK(sameAsPlain(a, p, "optimizeBLASes") > 0 && a.getFastValidations() == 4);
    a.getFastFlags(tf, pf);
    CHECK(tf == 15u && pf == poolBuilt && a.getFastValidations() == 4);
    // a static world: the seeded fast entry point against ntr_trace_bvh + ntr_trace_instanced_seeded
    a.setWorld(world);
    CHECK(a.isFastFlagsStale());
    CHECK(sameAsPlain(a, p, "setWorld") > 0 && a.getFastValidations() == 5);
    {
        Buffer ids;
        a.setTraceFast(true);
        a.traceBatch(p, ids);
        a.setTraceFast(false);
        const S32* id = (const S32*)ids.getPtr();
        int inWorld = 0, inInstance = 0;
        for (int i = 0; i < n; i++) { inWorld += id[i] == N ? 1 : 0; inInstance += (id[i] >= 0 && id[i] < N) ? 1 : 0; }
        CHECK(inWorld > 0 && inInstance > 0 && a.getFastValidations() == 5);
    }
    // frames with setFast equal the frames without it, word for word; the caller's switch comes back
    for (int withWorld = 1; withWorld >= 0; withWorld--) {
        if (!withWorld) { a.clearWorld(); CHECK(a.isFastFlagsStale()); }
        const Frame pf0 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_Primary, false, false, W, H, NS);
        const Frame pf1 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_Primary, true, false, W, H, NS);
        const Frame af0 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_AO, false, false, W, H, NS);
        const Frame af1 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_AO, true, false, W, H, NS);
        int lit = 0;
        for (int i = 0; i < n; i++) lit += pf1.pixels[(size_t)i] != 0u ? 1 : 0;
        const bool same = pf0.primary == pf1.primary && pf0.pixels == pf1.pixels && af0.primary == af1.primary && af0.pixels == af1.pixels &&
                          af0.aoHit == af1.aoHit && pf0.hits == pf1.hits && af0.hits == af1.hits;
        std::printf("frames %dx%d, %d samples, %s: fast %s plain; %d lit pixels, %zu AO rays\n", W, H, NS, withWorld ? "with a world" : "no world",
                    same ? "equals" : "DIFFERS FROM", lit, af1.aoHit.size());
        CHECK(same && lit > n / 8 && !af1.aoHit.empty() && af1.hits > 0);
        CHECK(!a.getTraceFast() && !a.isFastFlagsStale() && a.getFastValidations() == (withWorld ? 5 : 6));
    }
    // a vertex at 2^70: the pool loses FASTDIV, and so does the top level (instances of that BLAS are scaled by 0.004); no record changes
    std::vector<float> v3(v2);
    v3[3 * (size_t)triIdx[3 * (size_t)meshes[1].firstTri]] = 0x1p70f;
    Buffer pos3(v3.data(), (S64)numVerts * 12);
    a.refitBLASes(tri, numVerts, pos3);
    a.refit();
    sameAsPlain(a, p, "a vertex at 2^70");
    a.getFastFlags(tf, pf);
    std::printf("granted flags with a vertex at 2^70: top level %u, pool %u\n", tf, pf);
    CHECK((pf & NTR_BVH_FASTDIV) == 0 && (tf & NTR_BVH_FASTDIV) == 0 && a.getFastValidations() == 7);
    a.refitBLASes(tri, numVerts, pos2);
    a.refit();
    CHECK(sameAsPlain(a, p, "the vertex back") > 0);
    a.getFastFlags(tf, pf);
    CHECK(tf == 15u && pf == poolBuilt && a.getFastValidations() == 8);
    // the wide path ignores the switch
    a.widen();
    a.setTraceWide(true);
    a.setTraceFast(true);
    a.refit();
    a.widen();
    CHECK(a.isWide() && a.isFastFlagsStale());
    {
        Buffer ids;
        CHECK(a.traceBatch(p, ids) > 0.0f && a.isFastFlagsStale() && a.getFastValidations() == 8);
    }
    a.setTraceWide(false);
    a.setTraceFast(false);
    // buildBLASes and addBLAS mark the flags stale as well
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    CHECK(sameAsPlain(a, p, "buildBLASes + build") > 0 && a.getFastValidations() == 9);
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
    if (g_failed) { std::printf("instanced_fast_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_fast_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
