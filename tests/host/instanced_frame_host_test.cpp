// instanced_frame_host_test.cpp -- the host mirror's instanced frames (InstancedRenderer over CudaInstancedBVH, RayGen::aoNormals,
// CudaInstancedBVH::getBLASTrisBuffer).  `cpu`: beginFrame refuses a renderer without geometry, a pool with an addBLAS tree and a TLAS
// that is not built, and each message names the remedy.  `gpu`: an AO frame of a 3-mesh buildBLASes pool with 5 instances at 64 x 32
// equals, byte for byte, the buffers the same calls give when made directly through the C-ABI here -- rays, results, resolved results,
// normals and pixels; getTotalNumRays equals ntr_count_hits; after refitBLASes with moved vertices and refit() the next frame's normals
// differ from the first frame's and equal the direct calls'.  Compiled with plain g++ against libntrace_amd.so.
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

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    addBox(tris, verts, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), 2);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    const CameraView cam = camera(64, 32);

    // no geometry
    CudaInstancedBVH empty;
    InstancedRenderer r0(empty);
    CHECK(refused([&] { r0.beginFrame(cam, 64, 32); }, "setGeometry()"));
    // geometry, but nothing built: the TLAS is not current
    r0.setGeometry(scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer());
    CHECK(refused([&] { r0.beginFrame(cam, 64, 32); }, "build() or refit()"));
    CHECK(empty.getBLASTrisBuffer().getSize() == 0 && empty.getFirstMeshlessBLAS() == -1 && !empty.isBuilt());
    // a pool that holds an addBLAS tree: its mesh is not known, built or not
    CudaInstancedBVH inst;
    CHECK(inst.addBLAS(sah) == 0);
    InstancedRenderer r1(inst);
    r1.setGeometry(scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer());
    CHECK(refused([&] { r1.beginFrame(cam, 64, 32); }, "buildBLASes"));
    CHECK(inst.getFirstMeshlessBLAS() == 0 && inst.getBLASTrisBuffer().getSize() == (S64)sizeof(NtrBlasTris));
    const NtrBlasTris* bt = (const NtrBlasTris*)inst.getBLASTrisBuffer().getPtr();
    CHECK(bt[0].firstTri == 0 && bt[0].numTris == 0);
    CHECK(refused([&] { r1.traceBatch(); }, "no batch") && refused([&] { r1.setParams(InstancedRenderer::RayType_AO, 1.0f, 0); }, "sample count"));

    std::vector<float> m;
    std::vector<S32> which;
    transforms(5, 1, 0.3f, m, which);
    inst.setInstances(5, m.data(), which.data());
    int count = -1;
    const bool device = ntr_device_count(&count) == NTR_OK && count > 0;
    bool built = false;
    try { inst.build(); built = true; }
    catch (const FatalError& e) { std::printf("no device: build refused (%s)\n", e.message.c_str()); }
    CHECK(built == device && inst.isBuilt() == device);
    CHECK(refused([&] { r1.beginFrame(cam, 64, 32); }, "buildBLASes"));   // built or not, the addBLAS tree is refused first
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

static bool same(Buffer& a, Buffer& b, S64 bytes)
{
    return a.getSize() >= bytes && b.getSize() >= bytes && std::memcmp(a.getPtr(), b.getPtr(), (size_t)bytes) == 0;
}

// The AO frame through the C-ABI alone, over the mirror's pool, tree and instances
struct Direct {
    Buffer table, ids, resolved, normals, sids, sresolved, pixels;
    RayBuffer primary, secondary;
    int hits;
};

static void directFrame(Direct& d, CudaInstancedBVH& a, Buffer& tri, S32 numVerts, Buffer& pos, const CameraView& cam, int W, int H, int NS, F32 radius,
                        Buffer& mat, Buffer& shaded)
{
    const int n = W * H, m = n * NS;
    const S32 M = a.getNumInstances();
    const S64 tlasBytes = 64 * (S64)(M - 1);
    d.table.resizeDiscard((S64)n * 4);
    CHECK(ntr_pixel_table(W, H, (int32_t*)d.table.getMutableCudaPtr(), NULL, NULL) == NTR_OK);
    d.primary.resize(n);
    const float o[3] = {cam.position.x, cam.position.y, cam.position.z};
    CHECK(ntr_raygen_primary((NtrRay*)d.primary.getRayBuffer().getMutableCudaPtr(), (int32_t*)d.primary.getIDToSlotBuffer().getMutableCudaPtr(),
                             (int32_t*)d.primary.getSlotToIDBuffer().getMutableCudaPtr(), (const int32_t*)d.table.getCudaPtr(), o,
                             cam.nscreenToWorld.m, W, H, cam.cameraFar, 0, NULL) == NTR_OK);
    auto trace = [&](RayBuffer& rays, int count, int anyHit, Buffer& ids) {
        ids.resizeDiscard((S64)count * 4);
        float seconds = 0.0f;
        CHECK(ntr_trace_instanced(count, anyHit, (const NtrRay*)rays.getRayBuffer().getCudaPtr(), (NtrRayResult*)rays.getResultBuffer().getMutableCudaPtr(),
                                  (int32_t*)ids.getMutableCudaPtr(), a.getTLASNodeBuffer().getCudaPtr(), tlasBytes, 0, a.getRecordBuffer().getCudaPtr(),
                                  M, a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(), a.getPoolTriWoopBuffer().getCudaPtr(),
                                  a.getPoolTriWoopBuffer().getSize(), (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), &seconds,
                                  NULL) == NTR_OK);
    };
    NtrInstancedGeometry g;
    g.numInstances = M;
    g.numBlas = a.getNumBLAS();
    g.numTrisTotal = (int32_t)(tri.getSize() / 12);
    g.numVerts = numVerts;
    g.d_instances = (const NtrInstance*)a.getInstanceBuffer().getCudaPtr();
    g.d_blasTris = (const NtrBlasTris*)a.getBLASTrisBuffer().getCudaPtr();
    g.d_triVtxIndex = (const int32_t*)tri.getCudaPtr();
    g.d_vtxPos = (const float*)pos.getCudaPtr();

    trace(d.primary, n, 0, d.ids);
    d.resolved.resizeDiscard((S64)n * 16);
    d.normals.resizeDiscard((S64)n * 16);
    CHECK(ntr_instanced_hit_attributes(n, (const NtrRayResult*)d.primary.getResultBuffer().getCudaPtr(), (const int32_t*)d.ids.getCudaPtr(), &g,
                                       (NtrRayResult*)d.resolved.getMutableCudaPtr(), (float*)d.normals.getMutableCudaPtr(), NULL) == NTR_OK);
    d.secondary.resize(m);
    CHECK(ntr_raygen_ao_normals((NtrRay*)d.secondary.getRayBuffer().getMutableCudaPtr(), (int32_t*)d.secondary.getIDToSlotBuffer().getMutableCudaPtr(),
                                (int32_t*)d.secondary.getSlotToIDBuffer().getMutableCudaPtr(), (const NtrRay*)d.primary.getRayBuffer().getCudaPtr(),
                                (const NtrRayResult*)d.primary.getResultBuffer().getCudaPtr(), (const float*)d.normals.getCudaPtr(), 0, n, NS, radius,
                                Random(0).getU32(), NULL) == NTR_OK);
    trace(d.secondary, m, 1, d.sids);
    d.sresolved.resizeDiscard((S64)m * 16);
    CHECK(ntr_instanced_hit_attributes(m, (const NtrRayResult*)d.secondary.getResultBuffer().getCudaPtr(), (const int32_t*)d.sids.getCudaPtr(), &g,
                                       (NtrRayResult*)d.sresolved.getMutableCudaPtr(), NULL, NULL) == NTR_OK);
    d.pixels.resizeDiscard((S64)n * 4);
    d.pixels.clear(0x5a);
    CHECK(ntr_reconstruct(1, NS, 0, n, (const int32_t*)d.primary.getSlotToIDBuffer().getCudaPtr(), (const NtrRayResult*)d.resolved.getCudaPtr(),
                          (const int32_t*)d.secondary.getIDToSlotBuffer().getCudaPtr(), (const NtrRayResult*)d.sresolved.getCudaPtr(),
                          (const uint32_t*)mat.getCudaPtr(), (const uint32_t*)shaded.getCudaPtr(), (uint32_t*)d.pixels.getMutableCudaPtr(),
                          NULL) == NTR_OK);
    int32_t hits = -1;
    CHECK(ntr_count_hits((const NtrRayResult*)d.resolved.getCudaPtr(), n, &hits, NULL) == NTR_OK);
    d.hits = hits;
}

// One AO frame through the mirror, compared with the direct calls buffer by buffer -> the frame's normals
static void mirrorFrame(InstancedRenderer& r, Direct& d, int W, int H, int NS, const CameraView& cam, Buffer& mat, Buffer& shaded,
                        std::vector<U8>& normalsOut, const char* what)
{
    const int n = W * H, m = n * NS;
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0x5a);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch());                        // 2048 x 4 rays: one batch
    RayBuffer* last = r.getBatchRays();
    CHECK(last && last != &r.getPrimaryRays() && last->getSize() == m && !last->getNeedClosestHit());
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pixels, mat, shaded);
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);
    CHECK(same(p.getRayBuffer(), d.primary.getRayBuffer(), (S64)n * 32) && same(p.getResultBuffer(), d.primary.getResultBuffer(), (S64)n * 16));
    CHECK(same(p.getSlotToIDBuffer(), d.primary.getSlotToIDBuffer(), (S64)n * 4));
    CHECK(same(r.getPrimaryResolvedBuffer(), d.resolved, (S64)n * 16) && same(r.getPrimaryNormalBuffer(), d.normals, (S64)n * 16));
    CHECK(same(last->getRayBuffer(), d.secondary.getRayBuffer(), (S64)m * 32) && same(last->getResultBuffer(), d.secondary.getResultBuffer(), (S64)m * 16));
    CHECK(same(last->getIDToSlotBuffer(), d.secondary.getIDToSlotBuffer(), (S64)m * 4));
    CHECK(same(r.getBatchResolvedBuffer(), d.sresolved, (S64)m * 16));
    CHECK(same(pixels, d.pixels, (S64)n * 4));
    CHECK(r.getTotalNumRays() == d.hits * NS && d.hits > n / 16);
    CHECK(!r.nextBatch());
    const U8* nr = d.normals.getPtr();
    normalsOut.assign(nr, nr + (size_t)n * 16);
    // the frame is a picture: some secondary rays hit, some do not, and the resolved ids name pool triangles beyond the first mesh
    const NtrRayResult* sr = (const NtrRayResult*)d.sresolved.getPtr();
    const NtrRayResult* pr = (const NtrRayResult*)d.resolved.getPtr();
    const NtrRayResult* raw = (const NtrRayResult*)d.primary.getResultBuffer().getPtr();
    int occluded = 0, shifted = 0;
    for (int i = 0; i < m; i++) occluded += sr[i].id >= 0 ? 1 : 0;
    for (int i = 0; i < n; i++) shifted += pr[i].id > raw[i].id ? 1 : 0;
    CHECK(occluded > 0 && occluded < m && shifted > 0);
    std::printf("%s: %d primary hits, %d of %d AO rays occluded, %d ids moved to their pool triangle\n", what, d.hits, occluded, m, shifted);
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

    const S32 M = 5, B = 3;
    std::vector<float> m0;
    std::vector<S32> w0;
    transforms(M, B, 0.3f, m0, w0);
    CudaInstancedBVH a;
    a.buildBLASes(B, s.meshes.data(), tri, numVerts, pos);
    a.setInstances(M, m0.data(), w0.data());
    a.build();
    CHECK(a.isBuilt() && a.getFirstMeshlessBLAS() == -1 && a.getBLASTrisBuffer().getSize() == (S64)B * 8);
    const NtrBlasTris* bt = (const NtrBlasTris*)a.getBLASTrisBuffer().getPtr();
    for (S32 k = 0; k < B; k++) CHECK(bt[k].firstTri == s.meshes[k].firstTri && bt[k].numTris == s.meshes[k].numTris);

    const int W = 64, H = 32, NS = 4;
    const F32 radius = 1.5f;
    const CameraView cam = camera(W, H);
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(InstancedRenderer::RayType_AO, radius, NS);
    Direct d;
    std::vector<U8> n0, n1;
    directFrame(d, a, tri, numVerts, pos, cam, W, H, NS, radius, mat, shaded);
    mirrorFrame(r, d, W, H, NS, cam, mat, shaded, n0, "frame 0");

    // the meshes deform (a shear and a stretch: every normal turns), the triangles stay
    std::vector<Vec3f> moved(s.verts);
    for (size_t i = 0; i < moved.size(); i++) {
        const Vec3f v = moved[i];
        moved[i] = Vec3f(v.x + 0.4f * v.y, 1.2f * v.y - 0.3f * v.z, v.z + 0.25f * v.x);
    }
    pos.set(moved.data(), (S64)numVerts * 12);
    a.refitBLASes(tri, numVerts, pos);
    CHECK(refused([&] { r.beginFrame(cam, W, H); }, "build() or refit()"));   // the pool moved under the TLAS
    a.refit();
    directFrame(d, a, tri, numVerts, pos, cam, W, H, NS, radius, mat, shaded);
    mirrorFrame(r, d, W, H, NS, cam, mat, shaded, n1, "frame 1, after refitBLASes and refit");
    CHECK(n0.size() == n1.size() && std::memcmp(n0.data(), n1.data(), n0.size()) != 0);

    // a primary frame: one batch, the primary rays; its pixels are the direct ntr_reconstruct's over the resolved records
    r.setParams(InstancedRenderer::RayType_Primary, radius, NS);
    Buffer pix, pixDirect;
    pix.resizeDiscard((S64)W * H * 4);
    pixDirect.resizeDiscard((S64)W * H * 4);
    r.beginFrame(cam, W, H);
    CHECK(r.nextBatch() && r.getBatchRays() == &r.getPrimaryRays());
    CHECK(r.traceBatch() > 0.0f);
    r.updateResult(pix, mat, shaded);
    CHECK(r.getTotalNumRays() == W * H && !r.nextBatch());
    CHECK(same(r.getPrimaryResolvedBuffer(), d.resolved, (S64)W * H * 16));
    CHECK(ntr_reconstruct(0, 1, 0, W * H, (const int32_t*)d.primary.getSlotToIDBuffer().getCudaPtr(), (const NtrRayResult*)d.resolved.getCudaPtr(),
                          (const int32_t*)d.primary.getIDToSlotBuffer().getCudaPtr(), (const NtrRayResult*)d.resolved.getCudaPtr(),
                          (const uint32_t*)mat.getCudaPtr(), (const uint32_t*)shaded.getCudaPtr(), (uint32_t*)pixDirect.getMutableCudaPtr(),
                          NULL) == NTR_OK);
    CHECK(ntr_stream_synchronize(NULL) == NTR_OK);
    CHECK(same(pix, pixDirect, (S64)W * H * 4));
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
    if (g_failed) { std::printf("instanced_frame_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_frame_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
