// instanced_wide_fast_host_test.cpp -- the host mirror's FAST switch for the wide path (CudaInstancedBVH::setTraceWideFast,
// InstancedRenderer::setWideFast).  `cpu`: the switch and the staleness flag without a device.  `gpu <dir>`: the scene of the
// seeded trace's tests, which the test driver writes into <dir>; through a widen / refitWide / refitBLASesWide / setWorld / clearWorld
// loop every step marks the wide flags stale, the next wide fast traceBatch validates exactly once and the one after it not at all, and
// wide traceBatch with the switch on equals wide traceBatch with it off byte for byte, closest hit and any hit, with and without masks
// and a world; a vertex moved to 2^70 takes FASTDIV from both wide levels and changes no record; setTraceFast alone is still ignored on
// the wide path; primary and AO frames of InstancedRenderer with setWide(true) and setWideFast(true) equal the wide frames without it
// word for word.  Compiled with plain g++ against libntrace_amd.so.
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
    CHECK(!a.getTraceWideFast() && a.isWideFastFlagsStale() && a.getWideFastValidations() == 0);
    a.setTraceWideFast(true);
    CHECK(a.getTraceWideFast() && a.isWideFastFlagsStale() && !a.getTraceFast());
    a.setTraceWideFast(false);
    CHECK(!a.getTraceWideFast());
    U32 t = 7, p = 7;
    CHECK(refused([&] { a.getWideFastFlags(t, p); }, "widen") && t == 7 && p == 7);
    RayBuffer rays;
    Buffer ids;
    rays.resize(64);
    a.setTraceWide(true);
    a.setTraceWideFast(true);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS") && a.getWideFastValidations() == 0);   // nothing is validated without a TLAS
    InstancedRenderer r(a);
    CHECK(!r.getWideFast());
    r.setWideFast(true);
    CHECK(r.getWideFast() && !r.getFast());
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the switch is bookkeeping only\n");
}

struct Frame {
    std::vector<U8>  primary;       // resolved primary records
    std::vector<U32> pixels;
    std::vector<U8>  aoHit;         // per AO slot, in batch order: the record is a hit
    int hits;
};

// a wide frame (setWide(true)), with or without the wide FAST switch
static Frame render(CudaInstancedBVH& bvh, Buffer& tri, S32 numVerts, Buffer& pos, Buffer& mat, Buffer& shaded, InstancedRenderer::RayType type,
                    bool wideFast, int W, int H, int NS)
{
    Frame f;
    const int n = W * H;
    InstancedRenderer r(bvh);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(type, 3.0f, NS);
    r.setWide(true);
    r.setWideFast(wideFast);
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

// wide traceBatch with the switch on against wide traceBatch with it off on the same object: records and instance ids, both hit modes,
// two ray masks.  The first wide fast trace after a step that rewrote wide boxes validates, the later ones do not.  -> rays that hit
static int sameAsWide(CudaInstancedBVH& a, RayBuffer& p, const char* what)
{
    const int n = p.getSize();
    int hits = 0;
    CHECK(a.isWide() && a.getTraceWide() && a.isWideFastFlagsStale());
    const S32 before = a.getWideFastValidations(), binaryBefore = a.getFastValidations();
    for (int anyHit = 0; anyHit < 2; anyHit++)
        for (U32 rayMask : {0xFFFFFFFFu, 2u}) {
            p.setNeedClosestHit(!anyHit);
            Buffer idsFast, idsPlain;
            a.setTraceWideFast(true);
            p.getResultBuffer().clear(0x33);
            CHECK(a.traceBatch(p, idsFast, rayMask) > 0.0f);
            CHECK(!a.isWideFastFlagsStale() && a.getWideFastValidations() == before + 1);
            std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
            a.setTraceWideFast(false);
            p.getResultBuffer().clear(0x5a);
            CHECK(a.traceBatch(p, idsPlain, rayMask) > 0.0f);
            const bool same = std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0 &&
                              idsFast.getSize() == (S64)n * 4 && std::memcmp(idsFast.getPtr(), idsPlain.getPtr(), (size_t)n * 4) == 0;
            if (!same) { std::printf("%s anyHit=%d rayMask=%08x: wide fast differs from wide\n", what, anyHit, rayMask); g_failed++; }
            const NtrRayResult* r = (const NtrRayResult*)res.data();
            for (int i = 0; i < n; i++) hits += r[i].id != -1 ? 1 : 0;
        }
    p.setNeedClosestHit(true);
    CHECK(a.getFastValidations() == binaryBefore);                                          // the binary flags are not this path's business
    std::printf("%s: wide fast equals wide, %d hits, %d validation(s) so far\n", what, hits, a.getWideFastValidations());
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
    a.widen();
    a.setTraceWide(true);
    CHECK(a.isWide() && a.isWideFastFlagsStale() && a.getWideFastValidations() == 0);
    const int W = 64, H = 32, NS = 4, n = W * H;
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.beginFrame(camera(W, H), W, H);                                                       // (not fast: nothing is validated)
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n && a.getWideFastValidations() == 0 && a.isWideFastFlagsStale());

    S32 v = 0;                                                                              // validations expected so far
    CHECK(sameAsWide(a, p, "widen") > 0 && a.getWideFastValidations() == ++v);
    U32 tf = 0, pf = 0;
    a.getWideFastFlags(tf, pf);                                                             // current: no further validation
    std::printf("granted wide flags after widen: top level %u, pool %u\n", tf, pf);
    CHECK(a.getWideFastValidations() == v && tf == 15u && (pf & NTR_BVH_FASTDIV) != 0);
    const U32 poolBuilt = pf;
    // setTraceFast alone is still ignored on the wide path: no validation of either kind, the wide records
    {
        Buffer idsA, idsB;
        a.setTraceFast(true);
        p.getResultBuffer().clear(0x33);
        CHECK(a.traceBatch(p, idsA) > 0.0f && a.getFastValidations() == 0 && a.getWideFastValidations() == v);
        std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
        a.setTraceFast(false);
        p.getResultBuffer().clear(0x5a);
        CHECK(a.traceBatch(p, idsB) > 0.0f);
        CHECK(std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0 && std::memcmp(idsA.getPtr(), idsB.getPtr(), (size_t)n * 4) == 0);
    }
    // masks are not geometry: nothing goes stale
    std::vector<U32> masks((size_t)N);
    for (S32 i = 0; i < N; i++) masks[i] = (i % 3 == 0) ? 0x80000001u : (i % 3 == 1 ? 2u : 3u);
    a.setInstanceMasks(masks.data());
    CHECK(!a.isWideFastFlagsStale());
    // the instances move: setInstances alone rewrites no box, refitWide() does
    std::vector<float> moved(xf);
    for (S32 i = 0; i < N; i++) moved[12 * (size_t)i + 3] += 0.25f * (float)(i % 5);
    a.setInstances(N, moved.data(), which.data());
    CHECK(!a.isWideFastFlagsStale());
    a.refitWide();
    CHECK(sameAsWide(a, p, "refitWide, masked") > 0 && a.getWideFastValidations() == ++v);
    a.setInstanceMasks(NULL);
    // the vertices move
    std::vector<float> v2(vtx);
    for (size_t i = 0; i < v2.size(); i++) v2[i] *= 1.0f + 0.05f * (float)(i % 7) / 7.0f;
    Buffer pos2(v2.data(), (S64)numVerts * 12);
    a.refitBLASesWide(tri, numVerts, pos2);
    CHECK(a.isWideFastFlagsStale());
    a.refitWide();
    CHECK(sameAsWide(a, p, "refitBLASesWide + refitWide") > 0 && a.getWideFastValidations() == ++v);
    // widen() again rewrites the wide boxes
    a.widen();
    CHECK(sameAsWide(a, p, "widen again") > 0 && a.getWideFastValidations() == ++v);
    a.getWideFastFlags(tf, pf);
    CHECK(tf == 15u && pf == poolBuilt && a.getWideFastValidations() == v);
    // a static world: the seeded wide fast entry point against ntr_trace_bvh + ntr_trace_instanced_wide_seeded
    a.setWorld(world);
    CHECK(a.isWideFastFlagsStale());
    CHECK(sameAsWide(a, p, "setWorld") > 0 && a.getWideFastValidations() == ++v);
    {
        Buffer ids;
        a.setTraceWideFast(true);
        a.traceBatch(p, ids);
        a.setTraceWideFast(false);
        const S32* id = (const S32*)ids.getPtr();
        int inWorld = 0, inInstance = 0;
        for (int i = 0; i < n; i++) { inWorld += id[i] == N ? 1 : 0; inInstance += (id[i] >= 0 && id[i] < N) ? 1 : 0; }
        CHECK(inWorld > 0 && inInstance > 0 && a.getWideFastValidations() == v);
    }
    // wide frames with setWideFast equal the wide frames without it, word for word; the caller's switch comes back
    for (int withWorld = 1; withWorld >= 0; withWorld--) {
        if (!withWorld) { a.clearWorld(); CHECK(a.isWideFastFlagsStale()); v++; }
        const Frame pf0 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_Primary, false, W, H, NS);
        const Frame pf1 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_Primary, true, W, H, NS);
        const Frame af0 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_AO, false, W, H, NS);
        const Frame af1 = render(a, tri, numVerts, pos2, mat, shaded, InstancedRenderer::RayType_AO, true, W, H, NS);
        int lit = 0;
        for (int i = 0; i < n; i++) lit += pf1.pixels[(size_t)i] != 0u ? 1 : 0;
        const bool same = pf0.primary == pf1.primary && pf0.pixels == pf1.pixels && af0.primary == af1.primary && af0.pixels == af1.pixels &&
                          af0.aoHit == af1.aoHit && pf0.hits == pf1.hits && af0.hits == af1.hits;
        std::printf("wide frames %dx%d, %d samples, %s: wide fast %s wide; %d lit pixels, %zu AO rays\n", W, H, NS,
                    withWorld ? "with a world" : "no world", same ? "equals" : "DIFFERS FROM", lit, af1.aoHit.size());
        CHECK(same && lit > n / 8 && !af1.aoHit.empty() && af1.hits > 0);
        CHECK(!a.getTraceWideFast() && a.getTraceWide() && !a.isWideFastFlagsStale() && a.getWideFastValidations() == v);
    }
    // a vertex at 2^70: the wide pool loses FASTDIV, and so does the wide top level; no record changes
    std::vector<float> v3(v2);
    v3[3 * (size_t)triIdx[3 * (size_t)meshes[1].firstTri]] = 0x1p70f;
    Buffer pos3(v3.data(), (S64)numVerts * 12);
    a.refitBLASesWide(tri, numVerts, pos3);
    a.refitWide();
    sameAsWide(a, p, "a vertex at 2^70");
    a.getWideFastFlags(tf, pf);
    std::printf("granted wide flags with a vertex at 2^70: top level %u, pool %u\n", tf, pf);
    CHECK((pf & NTR_BVH_FASTDIV) == 0 && (tf & NTR_BVH_FASTDIV) == 0 && a.getWideFastValidations() == ++v);
    a.refitBLASesWide(tri, numVerts, pos2);
    a.refitWide();
    CHECK(sameAsWide(a, p, "the vertex back") > 0);
    a.getWideFastFlags(tf, pf);
    CHECK(tf == 15u && pf == poolBuilt && a.getWideFastValidations() == ++v);
    // what drops the wide pool or the wide TLAS marks the flags stale as well; with nothing wide to trace, nothing is validated
    a.refitBLASes(tri, numVerts, pos2);
    CHECK(!a.isWidePoolCurrent() && a.isWideFastFlagsStale());
    a.refit();
    a.setTraceWideFast(true);
    {
        Buffer ids;
        CHECK(!a.isWide() && a.traceBatch(p, ids) > 0.0f && a.getWideFastValidations() == v && a.getFastValidations() == 0);   // the binary path
    }
    a.setTraceWideFast(false);
    a.widen();
    CHECK(sameAsWide(a, p, "refitBLASes + refit + widen") > 0 && a.getWideFastValidations() == ++v);
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    CHECK(a.isWideFastFlagsStale() && !a.isWide());
    a.widen();
    CHECK(sameAsWide(a, p, "buildBLASes + build + widen") > 0 && a.getWideFastValidations() == ++v);
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
    if (g_failed) { std::printf("instanced_wide_fast_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_wide_fast_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
