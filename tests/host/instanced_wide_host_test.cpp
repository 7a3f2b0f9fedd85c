// instanced_wide_host_test.cpp -- the host mirror's wide path (CudaInstancedBVH::widen / setTraceWide, InstancedRenderer::setWide;
// DESIGN.md 6r).  `cpu`: widen() is refused before build(), and setTraceWide changes nothing without a wide tree; where there is a
// device the invalidation rules are walked through (build, refit, refitBLASes, buildBLASes and addBLAS).  `gpu`: the invalidation
// rules; setTraceWide(false) gives ntr_trace_instanced's bytes; the wide traceBatch equals ntr_trace_instanced_wide byte for byte, for closest hit and any hit, with and without masks; an AO
// frame with setWide(true) reconstructs, and the program prints how many of its pixels and of its primary records differ from the
// binary frame's.  With a directory as second argument the scene's buffers are written there, for the test driver to run the two numpy
// specs on.  Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"
#include "bvh/Platform.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

// a tessellated box: 12 * nTess^2 triangles
static void addBox(std::vector<Vec3i>& tris, std::vector<Vec3f>& verts, Vec3f lo, Vec3f hi, int nTess)
{
    auto quad = [&](Vec3f p0, Vec3f du, Vec3f dv) {
        const int base = (int)verts.size();
        for (int i = 0; i <= nTess; i++)
            for (int j = 0; j <= nTess; j++) verts.push_back(p0 + du * ((F32)i / nTess) + dv * ((F32)j / nTess));
        for (int i = 0; i < nTess; i++)
            for (int j = 0; j < nTess; j++) {
                const int a = base + i * (nTess + 1) + j, b = a + nTess + 1;
                tris.push_back(Vec3i(a, b, b + 1));
                tris.push_back(Vec3i(a, b + 1, a + 1));
            }
    };
    const Vec3f d = hi - lo;
    quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
    quad(Vec3f(lo.x, lo.y, hi.z), Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
    quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
    quad(Vec3f(lo.x, hi.y, lo.z), Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
    quad(lo, Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
    quad(Vec3f(hi.x, lo.y, lo.z), Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
}

template <class Call>
static bool refused(Call call, const char* word)
{
    try { call(); } catch (const FatalError& e) {
        if (std::strstr(e.message.c_str(), word)) return true;
        std::printf("refused with another message: %s\n", e.message.c_str());
    }
    return false;
}

// M instances side by side along x: a rotation about z times a non-uniform scale, instance i of BLAS i % numBlas; every third mirrored
static void transforms(S32 M, S32 numBlas, float angle, std::vector<float>& m, std::vector<S32>& which)
{
    m.assign(12 * (size_t)M, 0.0f);
    which.resize((size_t)M);
    for (S32 i = 0; i < M; i++) {
        const float a = angle * (float)(i + 1), c = std::cos(a), s = std::sin(a), sx = (i % 3 == 2) ? -2.5f : 2.5f, sy = 1.5f;
        float* t = &m[12 * (size_t)i];
        t[0] = c * sx; t[1] = -s * sy; t[3] = 6.0f * (float)(i - M / 2);
        t[4] = s * sx; t[5] = c * sy;  t[7] = 0.5f * (float)(i % 2);
        t[10] = 2.0f;
        which[i] = i % numBlas;
    }
}

// a pinhole camera on the -z side looking along +z: nscreen (nx, ny, 0, 1) -> a world point one unit in front of the eye
static CameraView camera(int w, int h)
{
    CameraView cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position = Vec3f(0.5f, 0.75f, -30.0f);
    F32* m = cam.nscreenToWorld.m;
    m[0] = 0.62f;  m[3] = cam.position.x;
    m[5] = -0.31f; m[7] = cam.position.y;
    m[11] = cam.position.z + 1.0f;
    m[15] = 1.0f;
    cam.cameraFar = 200.0f;
    cam.width = w;
    cam.height = h;
    return cam;
}

struct Mesh3 {
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    std::vector<NtrPlocBatchMesh> meshes;
};

static void makeMeshes(Mesh3& s)
{
    int first[4] = {0, 0, 0, 0};
    addBox(s.tris, s.verts, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), 5);
    first[1] = (int)s.tris.size();
    addBox(s.tris, s.verts, Vec3f(-1.0f, -1.0f, 0.25f), Vec3f(0.5f, 0.5f, 0.75f), 8);
    first[2] = (int)s.tris.size();
    addBox(s.tris, s.verts, Vec3f(-0.5f, -0.5f, -0.25f), Vec3f(0.25f, 0.75f, 0.5f), 1);
    first[3] = (int)s.tris.size();
    for (int k = 0; k < 3; k++) {
        NtrPlocBatchMesh mm;
        mm.firstTri = first[k];
        mm.numTris = first[k + 1] - first[k];
        const float mn[3] = {-4.0f, -4.0f, -4.0f}, mx[3] = {4.0f, 4.0f, 4.0f};
        std::memcpy(mm.sceneMin, mn, sizeof(mn));
        std::memcpy(mm.sceneMax, mx, sizeof(mx));
        s.meshes.push_back(mm);
    }
}

static void dump(const std::string& dir, const char* name, const void* p, size_t bytes)
{
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::printf("cannot write %s\n", path.c_str()); g_failed++; }
    if (f) std::fclose(f);
}

// build(), refit(), refitBLASes, buildBLASes and addBLAS against isWide() / isWidePoolCurrent() (needs a device)
static void invalidation(Mesh3& s)
{
    const S32 numVerts = (S32)s.verts.size();
    Buffer tri(s.tris.data(), (S64)s.tris.size() * 12), pos(s.verts.data(), (S64)numVerts * 12);
    std::vector<float> m;
    std::vector<S32> which;
    transforms(5, 3, 0.3f, m, which);
    CudaInstancedBVH a;
    a.buildBLASes(3, s.meshes.data(), tri, numVerts, pos);
    a.setInstances(5, m.data(), which.data());
    CHECK(refused([&] { a.widen(); }, "no TLAS to widen"));                               // before build()
    a.build();
    CHECK(a.isBuilt() && !a.isWide() && !a.isWidePoolCurrent() && !a.getTraceWide());
    a.widen();
    CHECK(a.isWide() && a.isWidePoolCurrent());
    CHECK(a.getWideResult().recordsBytes == 5 * 64 && a.getWideResult().numLeafLinks == 5 && a.getWideResult().nodesBytes >= 128);
    CHECK(a.getWideResult().stackBound == a.getWideResult().tlasStackBound + 1 + a.getWidePoolResult().stackBound);
    CHECK(a.getWideResult().stackBound <= 104 && a.getWidePoolResult().nodesBytes >= 3 * 128);
    const int64_t poolBytes = a.getWidePoolResult().nodesBytes;
    a.build();                                                                              // build() drops the wide TLAS, keeps the pool
    CHECK(a.isBuilt() && !a.isWide() && a.isWidePoolCurrent());
    a.widen();
    CHECK(a.isWide() && a.getWidePoolResult().nodesBytes == poolBytes);
    transforms(5, 3, 0.35f, m, which);
    a.setInstances(5, m.data(), which.data());
    CHECK(!a.isWide());                                                                     // (no TLAS is current)
    a.refit();                                                                              // refit() drops the wide TLAS, keeps the pool
    CHECK(a.isBuilt() && !a.isWide() && a.isWidePoolCurrent());
    a.widen();
    CHECK(a.isWide());
    a.refitBLASes(tri, numVerts, pos);                                                      // refitBLASes drops the wide pool too
    CHECK(!a.isWide() && !a.isWidePoolCurrent());
    a.refit();
    CHECK(!a.isWide());
    a.widen();
    CHECK(a.isWide() && a.isWidePoolCurrent());
    a.buildBLASes(3, s.meshes.data(), tri, numVerts, pos);                                  // buildBLASes too
    CHECK(!a.isWide() && !a.isWidePoolCurrent());
    a.build();
    a.widen();
    CHECK(a.isWide());
    CudaInstancedBVH b;                                                                     // and addBLAS: a fourth BLAS, a host SAH tree
    b.buildBLASes(3, s.meshes.data(), tri, numVerts, pos);
    b.setInstances(5, m.data(), which.data());
    b.build();
    b.widen();
    CHECK(b.isWide() && b.isWidePoolCurrent());
    const int64_t threeBytes = b.getWidePoolResult().nodesBytes;
    const S32 threeNodes = b.getWidePoolResult().numNodes;
    {
        std::vector<Vec3i> t2;
        std::vector<Vec3f> v2;
        addBox(t2, v2, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), 2);
        Scene scene((S32)t2.size(), t2.data(), (S32)v2.size(), v2.data());
        Platform platform("GPU");
        BVH::BuildParams params;
        BVH bvh(&scene, platform, params);
        CudaBVH sah(bvh, BVHLayout_Compact);
        CHECK(b.addBLAS(sah) == 3);
    }
    CHECK(!b.isBuilt() && !b.isWide() && !b.isWidePoolCurrent());                           // addBLAS drops the wide pool and the wide TLAS
    CHECK(refused([&] { b.widen(); }, "no TLAS to widen"));
    which[4] = 3;                                                                           // an instance of the added BLAS
    b.setInstances(5, m.data(), which.data());
    b.build();
    CHECK(!b.isWide() && !b.isWidePoolCurrent());
    b.widen();
    CHECK(b.isWide() && b.isWidePoolCurrent() && b.getNumBLAS() == 4);
    CHECK(b.getWidePoolResult().nodesBytes > threeBytes && b.getWidePoolResult().numNodes > threeNodes);   // the new pool covers the added BLAS
    {
        const U32* rec = (const U32*)b.getWideRecordBuffer().getPtr();                      // and instance 4's record lies behind the first three
        CHECK((int64_t)rec[16 * 4 + 12] == threeBytes && (int64_t)rec[16 * 4 + 12] + (int64_t)rec[16 * 4 + 14] == b.getWidePoolResult().nodesBytes);
        CHECK(rec[16 * 4 + 14] >= 128u && rec[16 * 4 + 15] == 0u);
    }
    which[4] = 4 % 3;
    // one instance: no top-level node
    S32 zero = 0;
    b.setInstances(1, m.data(), &zero);
    b.build();
    b.widen();
    CHECK(b.isWide() && b.getWideResult().nodesBytes == 0 && b.getWideResult().tlasStackBound == 0 && b.getWideResult().recordsBytes == 64);
}

static void cpuTests()
{
    Mesh3 s;
    makeMeshes(s);
    std::vector<float> m;
    std::vector<S32> which;
    CudaInstancedBVH a;
    CHECK(!a.isWide() && !a.getTraceWide() && a.getWideResult().stackBound == 0);
    CHECK(refused([&] { a.widen(); }, "no TLAS to widen"));                               // before anything
    transforms(5, 3, 0.3f, m, which);
    a.setInstances(5, m.data(), which.data());
    CHECK(refused([&] { a.widen(); }, "no TLAS to widen"));                               // before build()
    a.setTraceWide(true);
    CHECK(a.getTraceWide() && !a.isWide());
    int count = -1;
    const bool device = ntr_device_count(&count) == NTR_OK && count > 0;
    if (device) {
        invalidation(s);
    } else {
        std::printf("no device: widen() stays refused\n");
        RayBuffer rays;
        Buffer ids;
        rays.resize(64);
        CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS"));
    }
    InstancedRenderer r(a);
    CHECK(!r.getWide());
    r.setWide(true);
    CHECK(r.getWide());
}

static void gpuTests(const char* dumpDir)
{
    Mesh3 s;
    makeMeshes(s);
    invalidation(s);
    const S32 numVerts = (S32)s.verts.size(), numTris = (S32)s.tris.size();
    Buffer tri(s.tris.data(), (S64)numTris * 12), pos(s.verts.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[i] = 0xff000000u | (U32)(i * 2654435761u >> 8);
        sc[i] = 0xff000000u | (U32)((i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);

    const S32 M = 5, B = 3;
    std::vector<float> m0;
    std::vector<S32> w0;
    transforms(M, B, 0.3f, m0, w0);
    CudaInstancedBVH a;
    a.buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
    a.setInstances(M, m0.data(), w0.data());
    a.build();

    const int W = 64, H = 32, NS = 4, n = W * H;
    const CameraView cam = camera(W, H);
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(InstancedRenderer::RayType_AO, 1.5f, NS);

    // the binary AO frame
    Buffer pixelsBin, pixelsWide;
    pixelsBin.resizeDiscard((S64)n * 4);
    pixelsWide.resizeDiscard((S64)n * 4);
    pixelsBin.clear(0);
    pixelsWide.clear(0);
    r.beginFrame(cam, W, H);
    CHECK(!a.isWide());                                                                     // setWide(false): nothing is widened
    while (r.nextBatch()) {
        CHECK(r.traceBatch() > 0.0f);
        r.updateResult(pixelsBin, mat, shaded);
    }
    std::vector<U8> primBin((const U8*)r.getPrimaryResolvedBuffer().getPtr(), (const U8*)r.getPrimaryResolvedBuffer().getPtr() + (size_t)n * 16);
    const int hitsBin = r.getTotalNumRays() / NS;

    // setTraceWide(false), wide trees or not, gives ntr_trace_instanced's bytes; the wide traceBatch gives ntr_trace_instanced_wide's
    RayBuffer& p = r.getPrimaryRays();
    const U32 masks[5] = {1u, 2u, 0x80000000u, 3u, 2u};
    a.widen();
    CHECK(a.isWide());
    const int64_t wideTlasBytes = a.getWideResult().nodesBytes, widePoolBytes = a.getWidePoolResult().nodesBytes;
    for (int pass = 0; pass < 2; pass++) {                                                  // without masks, then with
        if (pass) a.setInstanceMasks(masks);
        CHECK(a.isWide());                                                                  // visibility is not geometry
        for (int anyHit = 0; anyHit < 2; anyHit++) {
            for (U32 rayMask : {0xFFFFFFFFu, 2u}) {
                p.setNeedClosestHit(!anyHit);
                NtrInstanceVisibility vis;
                vis.d_instanceMasks = pass ? (const uint32_t*)a.getInstanceMaskBuffer().getCudaPtr() : NULL;
                vis.d_rayMasks = NULL;
                vis.rayMask = rayMask;
                vis.pad = 0;
                float seconds = 0.0f;
                for (int wide = 0; wide < 2; wide++) {
                    a.setTraceWide(wide != 0);
                    Buffer ids, idsDirect;
                    p.getResultBuffer().clear(0x33);
                    CHECK(a.traceBatch(p, ids, rayMask) > 0.0f);
                    std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
                    p.getResultBuffer().clear(0x5a);
                    idsDirect.resizeDiscard((S64)n * 4);
                    int rc;
                    if (wide)
                        rc = ntr_trace_instanced_wide(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(),
                                                      (NtrRayResult*)p.getResultBuffer().getMutableCudaPtr(), (int32_t*)idsDirect.getMutableCudaPtr(),
                                                      a.getWideTLASNodeBuffer().getCudaPtr(), wideTlasBytes, 0, a.getWideRecordBuffer().getCudaPtr(), M,
                                                      a.getWidePoolNodeBuffer().getCudaPtr(), widePoolBytes, a.getPoolTriWoopBuffer().getCudaPtr(),
                                                      a.getPoolTriWoopBuffer().getSize(), (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), &vis,
                                                      &seconds, NULL);
                    else
                        rc = ntr_trace_instanced_masked(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(),
                                                        (NtrRayResult*)p.getResultBuffer().getMutableCudaPtr(), (int32_t*)idsDirect.getMutableCudaPtr(),
                                                        a.getTLASNodeBuffer().getCudaPtr(), 64 * (S64)(M - 1), 0, a.getRecordBuffer().getCudaPtr(), M,
                                                        a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(),
                                                        a.getPoolTriWoopBuffer().getCudaPtr(), a.getPoolTriWoopBuffer().getSize(),
                                                        (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), &vis, &seconds, NULL);
                    CHECK(rc == NTR_OK);
                    CHECK(std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);
                    CHECK(ids.getSize() == (S64)n * 4 && std::memcmp(ids.getPtr(), idsDirect.getPtr(), (size_t)n * 4) == 0);
                    const S32* id = (const S32*)ids.getPtr();
                    int hit = 0;
                    for (int i = 0; i < n; i++) hit += id[i] >= 0 ? 1 : 0;
                    CHECK(hit > 0);
                }
                a.setTraceWide(false);
            }
        }
    }
    p.setNeedClosestHit(true);
    a.setInstanceMasks(NULL);
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);

    if (dumpDir) {   // the scene, for the numpy specs
        const std::string d(dumpDir);
        dump(d, "pool_nodes.bin", a.getPoolNodeBuffer().getPtr(), (size_t)a.getPoolNodeBuffer().getSize());
        dump(d, "pool_woop.bin", a.getPoolTriWoopBuffer().getPtr(), (size_t)a.getPoolTriWoopBuffer().getSize());
        dump(d, "pool_index.bin", a.getPoolTriIndexBuffer().getPtr(), (size_t)a.getPoolTriIndexBuffer().getSize());
        dump(d, "tlas_nodes.bin", a.getTLASNodeBuffer().getPtr(), (size_t)(64 * (M - 1)));
        dump(d, "records.bin", a.getRecordBuffer().getPtr(), (size_t)(64 * M));
        dump(d, "instances.bin", a.getInstanceBuffer().getPtr(), (size_t)M * sizeof(NtrInstance));
        dump(d, "rays.bin", p.getRayBuffer().getPtr(), (size_t)n * 32);
        std::vector<NtrBlasRange> ranges;
        for (S32 k = 0; k < B; k++) ranges.push_back(a.getBLASRange(k));
        dump(d, "ranges.bin", ranges.data(), ranges.size() * sizeof(NtrBlasRange));
    }

    // the wide AO frame: a rebuilt TLAS, so that beginFrame has to widen
    a.build();
    CHECK(!a.isWide());
    r.setWide(true);
    r.beginFrame(cam, W, H);
    CHECK(a.isWide() && !a.getTraceWide());                                                 // widened; the flag is the caller's again
    int batches = 0;
    while (r.nextBatch()) {
        CHECK(r.traceBatch() > 0.0f);
        r.updateResult(pixelsWide, mat, shaded);
        batches++;
    }
    CHECK(batches >= 1 && !a.getTraceWide());
    const U8* primWide = (const U8*)r.getPrimaryResolvedBuffer().getPtr();
    int recDiff = 0, pixDiff = 0;
    for (int i = 0; i < n; i++) recDiff += std::memcmp(primBin.data() + 16 * (size_t)i, primWide + 16 * (size_t)i, 16) != 0 ? 1 : 0;
    const U32 *pb = (const U32*)pixelsBin.getPtr(), *pw = (const U32*)pixelsWide.getPtr();
    int lit = 0;
    for (int i = 0; i < n; i++) { pixDiff += pb[i] != pw[i] ? 1 : 0; lit += pw[i] != 0u ? 1 : 0; }
    CHECK(lit > 0 && r.getTotalNumRays() / NS >= hitsBin - recDiff && r.getTotalNumRays() / NS <= hitsBin + recDiff);
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
    std::printf("AO frame %dx%d, %d samples: wide against binary: %d of %d pixels differ, %d of %d primary records differ\n", W, H, NS, pixDiff, n,
                recDiff, n);
    r.setWide(false);
    r.beginFrame(cam, W, H);
    Buffer pixelsAgain;
    pixelsAgain.resizeDiscard((S64)n * 4);
    pixelsAgain.clear(0);
    while (r.nextBatch()) {
        r.traceBatch();
        r.updateResult(pixelsAgain, mat, shaded);
    }
    CHECK(std::memcmp(pixelsAgain.getPtr(), pixelsBin.getPtr(), (size_t)n * 4) == 0);       // setWide(false): the binary frame's bytes again
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) gpuTests(argc > 2 ? argv[2] : NULL);
        else cpuTests();
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        g_failed++;
    }
    if (g_failed) { std::printf("instanced_wide_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_wide_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
