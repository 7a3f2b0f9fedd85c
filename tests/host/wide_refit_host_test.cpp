// wide_refit_host_test.cpp -- the host mirror's in-place wide refit (CudaInstancedBVH::refitBLASesWide / refitWide).
// `cpu`: both methods are refused on an object without wide trees; where there is a device the preconditions and flags are walked
// through.  `gpu`: the preconditions and flags, and a frame that is updated both ways -- refitBLASesWide + refitWide on one object,
// refitBLASes + refit + widen on another -- and traced on the wide path.  The frame halves every vertex and doubles the linear part of
// every instance: both are exact in binary32, so every box of the pool halves exactly, every area falls to a quarter exactly, the
// widening of the refitted binary pool makes the choices it made before, and every world box stays what it was.  The two objects' wide
// pools, wide TLASes and wide records are then equal byte for byte, and so are their trace records; a wide refit that left a box, a
// padding slot or a record behind would show.  Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"

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

static bool sameBytes(Buffer& a, Buffer& b, int64_t bytes)
{
    return a.getSize() >= bytes && b.getSize() >= bytes && std::memcmp(a.getPtr(), b.getPtr(), (size_t)bytes) == 0;
}

static void cpuTests(void)
{
    CudaInstancedBVH a;
    Buffer tri, pos;
    CHECK(refused([&] { a.refitBLASesWide(tri, 0, pos); }, "no current wide pool"));
    CHECK(refused([&] { a.refitWide(); }, "no wide TLAS to refit"));
    CHECK(a.getWideBLASRefitResult().numEntries == 0 && a.getWideRefitResult().numLeaves == 0);
    int count = 0;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the wide refits stay refused\n");
}

static void gpuTests(void)
{
    Mesh3 s;
    makeMeshes(s);
    const S32 numVerts = (S32)s.verts.size(), numTris = (S32)s.tris.size();
    Buffer tri(s.tris.data(), (S64)numTris * 12), pos(s.verts.data(), (S64)numVerts * 12);
    const S32 M = 5, B = 3;
    std::vector<float> m0;
    std::vector<S32> w0;
    transforms(M, B, 0.3f, m0, w0);

    // ---- preconditions and flags
    CudaInstancedBVH a;
    a.buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
    a.setInstances(M, m0.data(), w0.data());
    a.build();
    CHECK(refused([&] { a.refitBLASesWide(tri, numVerts, pos); }, "no current wide pool"));   // never widened
    CHECK(refused([&] { a.refitWide(); }, "no wide TLAS to refit"));
    a.widen();
    CHECK(a.isBuilt() && a.isWide());
    a.refitWide();                                                                          // nothing moved: allowed, and everything stays current
    CHECK(a.isBuilt() && a.isWide() && a.getWideRefitResult().numLeaves == M && a.getWideRefitResult().errBits == 0);
    CHECK(a.getWideRefitResult().numNodes == a.getWideResult().numNodes);
    a.refitBLASes(tri, numVerts, pos);                                                      // the binary refit alone drops the wide pool
    CHECK(!a.isWidePoolCurrent());
    CHECK(refused([&] { a.refitBLASesWide(tri, numVerts, pos); }, "no current wide pool"));
    CHECK(refused([&] { a.refitWide(); }, "wide pool is not current"));
    a.refit();
    a.widen();
    const S32 two[2] = {2, 0};
    a.refitBLASesWide(tri, numVerts, pos, two, 2);                                          // a selection
    CHECK(a.isWidePoolCurrent() && !a.isBuilt() && !a.isWide());                            // the TLAS flags fall as after refitBLASes
    CHECK(a.getWideBLASRefitResult().numEntries == 2 && a.getWideBLASRefitResult().errBits == 0 && a.getWideBLASRefitResult().firstBadEntry == -1);
    CHECK(a.getBLASRefitResult().numEntries == 2 && a.getWideBLASRefitResult().numRows == a.getBLASRefitResult().numRows);
    CHECK(a.getWideBLASRefitResult().lanesPerLeaf == a.getBLASRefitResult().lanesPerLeaf);
    a.refitWide();
    CHECK(a.isBuilt() && a.isWide());
    a.build();                                                                              // a new TLAS has no wide counterpart yet
    CHECK(refused([&] { a.refitWide(); }, "no wide TLAS to refit"));
    a.widen();
    a.refitWide();
    CHECK(a.isWide());
    a.setInstances(M - 1, m0.data(), w0.data());                                            // another count: neither refit may run
    CHECK(refused([&] { a.refitWide(); }, "no wide TLAS to refit"));
    const S32 bad[1] = {3};
    a.setInstances(M, m0.data(), w0.data());
    a.build();
    a.widen();
    CHECK(refused([&] { a.refitBLASesWide(tri, numVerts, pos, bad, 1); }, "BLAS index"));

    // ---- one frame, updated both ways
    CudaInstancedBVH x, y;
    for (CudaInstancedBVH* o : {&x, &y}) {
        o->buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
        o->setInstances(M, m0.data(), w0.data());
        o->build();
        o->widen();
        o->setTraceWide(true);
    }
    std::vector<Vec3f> half(s.verts);
    for (Vec3f& v : half) v = v * 0.5f;
    Buffer pos2(half.data(), (S64)numVerts * 12);
    std::vector<float> m1(m0);
    for (S32 i = 0; i < M; i++)
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) m1[12 * (size_t)i + 4 * r + c] *= 2.0f;
    x.refitBLASesWide(tri, numVerts, pos2);
    x.setInstances(M, m1.data(), w0.data());
    x.refitWide();
    y.refitBLASes(tri, numVerts, pos2);
    y.setInstances(M, m1.data(), w0.data());
    y.refit();
    y.widen();
    CHECK(x.isBuilt() && x.isWide() && y.isBuilt() && y.isWide());
    CHECK(x.getWideBLASRefitResult().numEntries == B && x.getWideBLASRefitResult().numNodes == x.getWidePoolResult().numNodes);
    CHECK(x.getWideBLASRefitResult().numLeafLinks == x.getWidePoolResult().numLeafLinks);
    const int64_t poolBytes = x.getWidePoolResult().nodesBytes, tlasBytes = x.getWideResult().nodesBytes;
    CHECK(poolBytes == y.getWidePoolResult().nodesBytes && tlasBytes == y.getWideResult().nodesBytes && tlasBytes >= 128);
    CHECK(sameBytes(x.getPoolNodeBuffer(), y.getPoolNodeBuffer(), x.getPoolNodeBuffer().getSize()));
    CHECK(sameBytes(x.getWidePoolNodeBuffer(), y.getWidePoolNodeBuffer(), poolBytes));
    CHECK(sameBytes(x.getWideTLASNodeBuffer(), y.getWideTLASNodeBuffer(), tlasBytes));
    CHECK(sameBytes(x.getWideRecordBuffer(), y.getWideRecordBuffer(), 64 * (int64_t)M));
    {   // the refit did move something: the wide pool's root box of BLAS 0 is half of what the first widening wrote
        CudaInstancedBVH z;
        z.buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
        z.setInstances(M, m0.data(), w0.data());
        z.build();
        z.widen();
        const F32 *before = (const F32*)z.getWidePoolNodeBuffer().getPtr(), *after = (const F32*)x.getWidePoolNodeBuffer().getPtr();
        for (int wd = 0; wd < 12; wd++) CHECK(after[wd] == 0.5f * before[wd]);
        CHECK(!sameBytes(x.getWideRecordBuffer(), z.getWideRecordBuffer(), 64 * (int64_t)M));
    }

    const int W = 64, H = 32, n = W * H;
    const CameraView cam = camera(W, H);
    InstancedRenderer r(x);
    r.setGeometry(tri, numVerts, pos2);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch());
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        p.setNeedClosestHit(!anyHit);
        Buffer idsX, idsY;
        p.getResultBuffer().clear(0x33);
        CHECK(x.traceBatch(p, idsX) > 0.0f);
        std::vector<U8> resX((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
        p.getResultBuffer().clear(0x5a);
        CHECK(y.traceBatch(p, idsY) > 0.0f);
        const NtrRayResult *rx = (const NtrRayResult*)resX.data(), *ry = (const NtrRayResult*)p.getResultBuffer().getPtr();
        const S32 *ix = (const S32*)idsX.getPtr(), *iy = (const S32*)idsY.getPtr();
        int hits = 0, differ = 0;
        for (int i = 0; i < n; i++) {
            hits += ix[i] >= 0 ? 1 : 0;
            differ += (rx[i].id != ry[i].id || ix[i] != iy[i]) ? 1 : 0;
        }
        CHECK(hits > n / 16 && differ == 0);
        CHECK(std::memcmp(resX.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);   // the trees are the same bytes: so are the records
        std::printf("anyHit %d: %d of %d rays hit, %d records differ between the refitted and the re-widened trees\n", anyHit, hits, n, differ);
    }
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) gpuTests();
        else cpuTests();
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        g_failed++;
    }
    if (g_failed) { std::printf("wide_refit_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("wide_refit_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
