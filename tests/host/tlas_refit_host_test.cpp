// tlas_refit_host_test.cpp -- the host mirror's top-level refit (CudaInstancedBVH::refit over ntr_tlas_refit): a call before build(), after
// a changed instance count and after addBLAS is refused and says to call build() (`cpu`); on a GPU (`gpu`) buildBLASes, setInstances,
// build(), setInstances with moved transforms of the same count and refit(): the TLAS and record buffers equal, byte for byte, those of
// a second object refitted through the C-ABI directly, and traceBatch gives the records of ntr_trace_instanced over that tree.
// Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "CudaInstancedBVH.hpp"
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

// M instances side by side along x: a rotation about z by `angle` radians times a non-uniform scale, instance i of BLAS i % numBlas;
// every third mirrored
static void transforms(S32 M, S32 numBlas, float angle, float shift, std::vector<float>& m, std::vector<S32>& which)
{
    m.assign(12 * (size_t)M, 0.0f);
    which.resize((size_t)M);
    for (S32 i = 0; i < M; i++) {
        const float a = angle * (float)(i + 1), c = std::cos(a), s = std::sin(a), sx = (i % 3 == 2) ? -1.25f : 1.25f, sy = 0.75f;
        float* t = &m[12 * (size_t)i];
        t[0] = c * sx; t[1] = -s * sy; t[3] = 8.0f * (float)(i - M / 2) + shift;
        t[4] = s * sx; t[5] = c * sy;  t[7] = shift * (float)(i % 2);
        t[10] = 1.0f;
        which[i] = i % numBlas;
    }
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

    CudaInstancedBVH inst;
    CHECK(refused([&] { inst.refit(); }, "build()"));
    CHECK(inst.addBLAS(sah) == 0);
    std::vector<float> m;
    std::vector<S32> which;
    transforms(5, 1, 0.3f, 0.0f, m, which);
    inst.setInstances(5, m.data(), which.data());
    CHECK(refused([&] { inst.refit(); }, "build()"));           // instances alone are no tree
    CHECK(inst.getRefitResult().numNodes == 0 && inst.getRefitResult().seconds == 0.0f);

    int count = -1;
    const bool device = ntr_device_count(&count) == NTR_OK && count > 0;
    bool builtOnce = false;
    try { inst.build(); builtOnce = true; }
    catch (const FatalError& e) { std::printf("no device: build refused (%s)\n", e.message.c_str()); }
    CHECK(builtOnce == device);
    if (!device) CHECK(refused([&] { inst.refit(); }, "build()"));   // a failed build leaves no tree behind
    // a changed instance count invalidates the tree, built or not
    transforms(4, 1, 0.3f, 0.0f, m, which);
    inst.setInstances(4, m.data(), which.data());
    CHECK(refused([&] { inst.refit(); }, "build()"));
    if (device) {
        // the same count keeps it; addBLAS invalidates it
        inst.build();
        transforms(4, 1, 0.5f, 1.0f, m, which);
        inst.setInstances(4, m.data(), which.data());
        inst.refit();
        CHECK(inst.getRefitResult().numNodes == 3 && inst.getRefitResult().numLeaves == 4 && inst.getRefitResult().errBits == 0);
        CHECK(inst.addBLAS(sah) == 1);
        CHECK(refused([&] { inst.refit(); }, "build()"));
    } else {
        int64_t held = -1;
        CHECK(ntr_tlas_refit_scratch_bytes(&held) == NTR_OK && held == 0);
    }
}

static void fillRays(RayBuffer& rays, int W, int H)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            Ray r;
            r.origin = Vec3f(-36.0f + 72.0f * (x + 0.5f) / W, -3.0f + 8.0f * (y + 0.5f) / H, -30.0f);
            r.direction = Vec3f(0.0f, 0.0f, 1.0f);
            r.tmin = 0.0f;
            r.tmax = 100.0f;
            rays.setRay(y * W + x, r);
        }
}

static void makePool(CudaInstancedBVH& inst, Scene& scene, const std::vector<NtrPlocBatchMesh>& meshes)
{
    inst.buildBLASes((S32)meshes.size(), meshes.data(), scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer());
}

static void gpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    int first[4] = {0, 0, 0, 0};
    addBox(tris, verts, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), 5);
    first[1] = (int)tris.size();
    addBox(tris, verts, Vec3f(-1.0f, -1.0f, 0.25f), Vec3f(0.5f, 0.5f, 0.75f), 8);
    first[2] = (int)tris.size();
    addBox(tris, verts, Vec3f(-0.5f, -0.5f, -0.25f), Vec3f(0.25f, 0.75f, 0.5f), 1);
    first[3] = (int)tris.size();
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Vec3f lo, hi;
    scene.getBBox(lo, hi);
    std::vector<NtrPlocBatchMesh> meshes;
    for (int k = 0; k < 3; k++) {
        NtrPlocBatchMesh mm;
        mm.firstTri = first[k];
        mm.numTris = first[k + 1] - first[k];
        const float mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
        std::memcpy(mm.sceneMin, mn, sizeof(mn));
        std::memcpy(mm.sceneMax, mx, sizeof(mx));
        meshes.push_back(mm);
    }
    const S32 M = 9, B = (S32)meshes.size();
    std::vector<float> m0, m1;
    std::vector<S32> w0, w1;
    transforms(M, B, 0.3f, 0.0f, m0, w0);
    transforms(M, B, 0.45f, 1.5f, m1, w1);
    for (S32 i = 0; i < M; i += 4) w1[i] = (w1[i] + 1) % B;     // a level-of-detail switch for some

    CudaInstancedBVH a, b;
    makePool(a, scene, meshes);
    makePool(b, scene, meshes);
    a.setInstances(M, m0.data(), w0.data());
    b.setInstances(M, m0.data(), w0.data());
    a.build();
    b.build();
    CHECK(a.getTLASNodeBuffer().getSize() == 64 * (M - 1) && b.getTLASNodeBuffer().getSize() == 64 * (M - 1));
    CHECK(std::memcmp(a.getTLASNodeBuffer().getPtr(), b.getTLASNodeBuffer().getPtr(), 64 * (M - 1)) == 0);

    // the mirror's path
    a.setInstances(M, m1.data(), w1.data());
    a.refit();
    const NtrTlasRefitResult& rr = a.getRefitResult();
    CHECK(rr.numNodes == M - 1 && rr.numLeaves == M && rr.errBits == 0 && rr.seconds > 0.0f);
    CHECK(std::memcmp(rr.sceneMin, a.getBuildResult().sceneMin, 6 * sizeof(float)) == 0);
    std::printf("refit: %d instances, %.1f us\n", M, rr.seconds * 1e6f);

    // the C-ABI directly, on the second object's buffers
    b.setInstances(M, m1.data(), w1.data());
    std::vector<NtrBlasRange> ranges;
    for (S32 k = 0; k < B; k++) ranges.push_back(b.getBLASRange(k));
    NtrTlasRefitResult direct;
    const int rc = ntr_tlas_refit(M, (const NtrInstance*)b.getInstanceBuffer().getCudaPtr(), B, ranges.data(), b.getPoolNodeBuffer().getCudaPtr(),
                                  b.getPoolNodeBuffer().getSize(), b.getTLASNodeBuffer().getMutableCudaPtr(), 64 * (M - 1), 0,
                                  b.getRecordBuffer().getMutableCudaPtr(), b.getRecordBuffer().getSize(), NULL, &direct, NULL);
    CHECK(rc == NTR_OK);
    CHECK(direct.numNodes == rr.numNodes && direct.numLeaves == rr.numLeaves && std::memcmp(direct.sceneMin, rr.sceneMin, 6 * sizeof(float)) == 0);
    CHECK(std::memcmp(a.getTLASNodeBuffer().getPtr(), b.getTLASNodeBuffer().getPtr(), 64 * (M - 1)) == 0);
    CHECK(a.getRecordBuffer().getSize() == b.getRecordBuffer().getSize() &&
          std::memcmp(a.getRecordBuffer().getPtr(), b.getRecordBuffer().getPtr(), (size_t)a.getRecordBuffer().getSize()) == 0);
    // the boxes did change
    CudaInstancedBVH c;
    makePool(c, scene, meshes);
    c.setInstances(M, m0.data(), w0.data());
    c.build();
    CHECK(std::memcmp(a.getTLASNodeBuffer().getPtr(), c.getTLASNodeBuffer().getPtr(), 64 * (M - 1)) != 0);

    // traceBatch gives that tree's records
    const int W = 96, H = 16;
    RayBuffer ra(W * H, true), rb(W * H, true);
    fillRays(ra, W, H);
    fillRays(rb, W, H);
    Buffer ia, ib;
    CHECK(a.traceBatch(ra, ia) > 0.0f);
    ib.resizeDiscard((S64)W * H * sizeof(S32));
    float seconds = 0.0f;
    const int rt = ntr_trace_instanced(W * H, 0, (const NtrRay*)rb.getRayBuffer().getCudaPtr(), (NtrRayResult*)rb.getResultBuffer().getMutableCudaPtr(),
                                       (int32_t*)ib.getMutableCudaPtr(), b.getTLASNodeBuffer().getCudaPtr(), 64 * (M - 1), 0,
                                       b.getRecordBuffer().getCudaPtr(), M, b.getPoolNodeBuffer().getCudaPtr(), b.getPoolNodeBuffer().getSize(),
                                       b.getPoolTriWoopBuffer().getCudaPtr(), b.getPoolTriWoopBuffer().getSize(),
                                       (const int32_t*)b.getPoolTriIndexBuffer().getCudaPtr(), &seconds, NULL);
    CHECK(rt == NTR_OK);
    CHECK(std::memcmp(ra.getResultBuffer().getPtr(), rb.getResultBuffer().getPtr(), (size_t)ra.getResultBuffer().getSize()) == 0);
    CHECK(ia.getSize() == ib.getSize() && std::memcmp(ia.getPtr(), ib.getPtr(), (size_t)ia.getSize()) == 0);
    const S32* id = (const S32*)ia.getPtr();
    int hits = 0;
    for (int i = 0; i < W * H; i++) hits += id[i] >= 0 ? 1 : 0;
    CHECK(hits > 0);

    // b's tree is stale for the mirror (setInstances) until refit(); a changed count refuses
    CHECK(refused([&] { b.traceBatch(rb, ib); }, "No TLAS"));
    b.refit();
    CHECK(b.traceBatch(rb, ib) > 0.0f);
    b.setInstances(M - 1, m1.data(), w1.data());
    CHECK(refused([&] { b.refit(); }, "build()"));
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
    if (g_failed) { std::printf("tlas_refit_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("tlas_refit_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
