// instanced_masked_host_test.cpp -- the host mirror's instance visibility (CudaInstancedBVH::setInstanceMasks / traceBatch's ray mask,
// InstancedRenderer::setRayMasks).  `cpu`: setInstanceMasks is refused before setInstances; a setInstances with the same
// count keeps the masks and one with another count drops them; a mask change leaves isBuilt() as it was.  `gpu`: traceBatch with masks
// equals ntr_trace_instanced_masked byte for byte, for closest hit and any hit; in an AO frame whose primary mask hides the one instance
// of a BLAS while the secondary mask shows everything, no resolved primary record names a triangle of that BLAS and at least one AO ray
// hits it -- an object invisible to the camera that still occludes.  Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "InstancedRenderer.hpp"
#include "Random.hpp"
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
        const float mn[3] = {-4.0f, -4.0f, -4.0f}, mx[3] = {4.0f, 4.0f, 4.0f};   // (a box that holds the moved vertices too)
        std::memcpy(mm.sceneMin, mn, sizeof(mn));
        std::memcpy(mm.sceneMax, mx, sizeof(mx));
        s.meshes.push_back(mm);
    }
}

static void cpuTests()
{
    Mesh3 s;
    makeMeshes(s);
    std::vector<float> m;
    std::vector<S32> which;
    CudaInstancedBVH a;
    const U32 five[5] = {1u, 2u, 0x80000000u, 0u, 0xFFFFFFFFu};
    CHECK(refused([&] { a.setInstanceMasks(five); }, "setInstances first"));            // before any instance
    CHECK(refused([&] { a.setInstanceMasks(NULL); }, "setInstances first"));
    CHECK(a.getInstanceMaskBuffer().getSize() == 0);
    transforms(5, 3, 0.3f, m, which);
    a.setInstances(5, m.data(), which.data());
    CHECK(a.getInstanceMaskBuffer().getSize() == 0 && !a.isBuilt());
    a.setInstanceMasks(five);
    CHECK(a.getInstanceMaskBuffer().getSize() == 20 && std::memcmp(a.getInstanceMaskBuffer().getPtr(), five, 20) == 0 && !a.isBuilt());
    a.setInstances(5, m.data(), which.data());                                          // the same count keeps them
    CHECK(a.getInstanceMaskBuffer().getSize() == 20 && std::memcmp(a.getInstanceMaskBuffer().getPtr(), five, 20) == 0);
    a.setInstanceMasks(NULL);                                                           // all visible again
    CHECK(a.getInstanceMaskBuffer().getSize() == 0);
    a.setInstanceMasks(five);
    transforms(4, 3, 0.3f, m, which);
    a.setInstances(4, m.data(), which.data());                                          // another count drops them
    CHECK(a.getInstanceMaskBuffer().getSize() == 0 && a.getNumInstances() == 4);
    a.setInstanceMasks(five);
    CHECK(a.getInstanceMaskBuffer().getSize() == 16);

    // a mask change leaves isBuilt() as it was: false without a TLAS, and true with one where there is a device to build it
    int count = -1;
    const bool device = ntr_device_count(&count) == NTR_OK && count > 0;
    if (device) {
        const S32 numVerts = (S32)s.verts.size();
        Buffer tri(s.tris.data(), (S64)s.tris.size() * 12), pos(s.verts.data(), (S64)numVerts * 12);
        a.buildBLASes(3, s.meshes.data(), tri, numVerts, pos);
        a.build();
        CHECK(a.isBuilt() && a.getInstanceMaskBuffer().getSize() == 16);                // buildBLASes and build keep the masks
        a.setInstanceMasks(five + 1);
        CHECK(a.isBuilt());
        a.setInstanceMasks(NULL);
        CHECK(a.isBuilt());
    } else {
        std::printf("no device: isBuilt() stays false\n");
        RayBuffer rays;
        Buffer ids;
        rays.resize(64);
        CHECK(refused([&] { a.traceBatch(rays, ids, 1u); }, "No TLAS"));
    }
}

static void gpuTests()
{
    Mesh3 s;
    makeMeshes(s);
    const S32 numVerts = (S32)s.verts.size(), numTris = (S32)s.tris.size();
    Buffer tri(s.tris.data(), (S64)numTris * 12), pos(s.verts.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[i] = 0xff000000u | (U32)(i * 2654435761u >> 8);
        sc[i] = 0xff000000u | (U32)((i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);

    // five instances side by side; instance 2, the only user of BLAS 2 (the small box), floats half a unit in front of instance 3
    const S32 M = 5, B = 3, HID = 2;
    std::vector<float> m0;
    std::vector<S32> w0;
    transforms(M, B, 0.3f, m0, w0);
    m0[12 * HID + 3] = m0[12 * 3 + 3];
    m0[12 * HID + 7] = m0[12 * 3 + 7];
    m0[12 * HID + 11] = -5.0f;
    CudaInstancedBVH a;
    a.buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
    a.setInstances(M, m0.data(), w0.data());
    a.build();
    for (S32 i = 0; i < M; i++) CHECK((w0[i] == HID) == (i == HID));
    const S32 hidFirst = s.meshes[HID].firstTri, hidEnd = hidFirst + s.meshes[HID].numTris;

    const int W = 64, H = 32, NS = 4, n = W * H, ns = n * NS;
    const F32 radius = 1.5f;
    const CameraView cam = camera(W, H);
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(InstancedRenderer::RayType_AO, radius, NS);
    auto countIn = [&](Buffer& resolved, int num) {
        const NtrRayResult* rr = (const NtrRayResult*)resolved.getPtr();
        int c = 0;
        for (int i = 0; i < num; i++) c += (rr[i].id >= hidFirst && rr[i].id < hidEnd) ? 1 : 0;
        return c;
    };
    // everything visible: the camera sees the small box
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch() && r.traceBatch() > 0.0f);
    const int seen = countIn(r.getPrimaryResolvedBuffer(), n);
    CHECK(seen > 0);
    const int hits0 = r.getTotalNumRays() / NS;

    // traceBatch with masks is the C-ABI call, byte for byte
    const U32 masks[5] = {1u, 2u, 0x80000000u, 3u, 2u};
    a.setInstanceMasks(masks);
    CHECK(a.isBuilt());
    RayBuffer& p = r.getPrimaryRays();
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        for (U32 rayMask : {2u, 0x80000001u, 0xFFFFFFFFu}) {
            p.setNeedClosestHit(!anyHit);
            Buffer ids, idsDirect;
            CHECK(a.traceBatch(p, ids, rayMask) > 0.0f);
            std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
            p.getResultBuffer().clear(0x5a);
            idsDirect.resizeDiscard((S64)n * 4);
            NtrInstanceVisibility vis;
            vis.d_instanceMasks = (const uint32_t*)a.getInstanceMaskBuffer().getCudaPtr();
            vis.d_rayMasks = NULL;
            vis.rayMask = rayMask;
            vis.pad = 0;
            float seconds = 0.0f;
            CHECK(ntr_trace_instanced_masked(n, anyHit, (const NtrRay*)p.getRayBuffer().getCudaPtr(), (NtrRayResult*)p.getResultBuffer().getMutableCudaPtr(),
                                             (int32_t*)idsDirect.getMutableCudaPtr(), a.getTLASNodeBuffer().getCudaPtr(), 64 * (S64)(M - 1), 0,
                                             a.getRecordBuffer().getCudaPtr(), M, a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(),
                                             a.getPoolTriWoopBuffer().getCudaPtr(), a.getPoolTriWoopBuffer().getSize(),
                                             (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), &vis, &seconds, NULL) == NTR_OK);
            CHECK(std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);
            CHECK(ids.getSize() == (S64)n * 4 && std::memcmp(ids.getPtr(), idsDirect.getPtr(), (size_t)n * 4) == 0);
            const S32* id = (const S32*)ids.getPtr();
            int hit = 0;
            for (int i = 0; i < n; i++) {
                if (id[i] >= 0) { hit++; CHECK((masks[id[i]] & rayMask) != 0); }
            }
            CHECK(hit > 0);
        }
    }
    p.setNeedClosestHit(true);
    a.setInstanceMasks(NULL);

    // the AO frame: bit 0 is "seen by the camera"; instance HID lacks it, the secondary mask shows everything
    U32 vm[5];
    for (S32 i = 0; i < M; i++) vm[i] = (i == HID) ? 2u : 3u;
    a.setInstanceMasks(vm);
    r.setRayMasks(1u, 0xFFFFFFFFu);
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch());
    RayBuffer* ao = r.getBatchRays();
    CHECK(ao && ao->getSize() == ns && !ao->getNeedClosestHit());
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pixels, mat, shaded);
    const int primaryOnHidden = countIn(r.getPrimaryResolvedBuffer(), n), aoOnHidden = countIn(r.getBatchResolvedBuffer(), ns);
    CHECK(primaryOnHidden == 0);              // the camera does not see it
    CHECK(aoOnHidden > 0);                    // and it still occludes
    CHECK(r.getTotalNumRays() / NS >= hits0); // what it covered is seen instead (it floats in front of instance 3)
    CHECK(!r.nextBatch());
    std::printf("AO frame, instance %d hidden from the camera: %d primary records named it before, %d now; %d of %d AO rays hit it\n", HID, seen,
                primaryOnHidden, aoOnHidden, ns);

    // the masks the other way round: seen by the camera, no occluder
    r.setRayMasks(0xFFFFFFFFu, 1u);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch() && r.traceBatch() > 0.0f);
    CHECK(countIn(r.getPrimaryResolvedBuffer(), n) == seen && countIn(r.getBatchResolvedBuffer(), r.getBatchRays()->getSize()) == 0);
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
    if (g_failed) { std::printf("instanced_masked_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_masked_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
