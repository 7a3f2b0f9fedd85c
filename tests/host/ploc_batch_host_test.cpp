// ploc_batch_host_test.cpp -- the host mirror's batched BLAS build (CudaInstancedBVH::buildBLASes over ntr_ploc_build_batch): bad batches
// and a build without a device are refused and leave no BLAS behind (`cpu`); on a GPU (`gpu`) the pool that buildBLASes fills equals, byte
// for byte, the pool that addBLAS makes of one CudaPLOCBuilder tree per mesh, its ranges are addBLAS's, and a top-level tree over it
// traces.  Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <vector>

#include "CudaInstancedBVH.hpp"
#include "CudaPLOCBuilder.hpp"

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

// three boxes in one index array, and the meshes of the batch: the boxes, the second box once more, and one triangle.  Every mesh
// takes its codes over the box of ALL vertices, as a Scene of those triangles over the whole vertex array does
static void makeBatch(std::vector<Vec3i>& tris, std::vector<Vec3f>& verts, std::vector<NtrPlocBatchMesh>& meshes, int nTess)
{
    int first[4] = {0, 0, 0, 0};
    addBox(tris, verts, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), nTess);
    first[1] = (int)tris.size();
    addBox(tris, verts, Vec3f(2.0f, -1.0f, 0.25f), Vec3f(3.5f, 0.5f, 0.75f), nTess + 3);
    first[2] = (int)tris.size();
    addBox(tris, verts, Vec3f(-0.5f, 2.0f, -0.25f), Vec3f(0.25f, 2.75f, 0.5f), 1);
    first[3] = (int)tris.size();
    Scene all((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Vec3f lo, hi;
    all.getBBox(lo, hi);
    const int ranges[5][2] = {{first[0], first[1] - first[0]}, {first[1], first[2] - first[1]}, {first[2], first[3] - first[2]},
                              {first[1], first[2] - first[1]}, {first[3] - 1, 1}};
    for (const auto& r : ranges) {
        NtrPlocBatchMesh m;
        m.firstTri = r[0];
        m.numTris = r[1];
        const float mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
        std::memcpy(m.sceneMin, mn, sizeof(mn));
        std::memcpy(m.sceneMax, mx, sizeof(mx));
        meshes.push_back(m);
    }
}

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    std::vector<NtrPlocBatchMesh> meshes;
    makeBatch(tris, verts, meshes, 2);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    CudaInstancedBVH inst;
    bool threw = false;
    try { inst.buildBLASes(0, meshes.data(), scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer()); } catch (const FatalError&) { threw = true; }
    CHECK(threw);
    std::vector<NtrPlocBatchMesh> bad = meshes;
    bad[1].numTris = 0;
    threw = false;
    try { inst.buildBLASes((S32)bad.size(), bad.data(), scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer()); } catch (const FatalError&) { threw = true; }
    CHECK(threw && inst.getNumBLAS() == 0 && inst.getBLASBuildResult().numMeshes == 0);
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        threw = false;
        try { inst.buildBLASes((S32)meshes.size(), meshes.data(), scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer()); }
        catch (const FatalError& e) { threw = true; std::printf("no device: buildBLASes refused (%s)\n", e.message.c_str()); }
        CHECK(threw && inst.getNumBLAS() == 0);
        int64_t held = -1;
        CHECK(ntr_ploc_batch_scratch_bytes(&held) == NTR_OK && held == 0);
    }
}

static void gpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    std::vector<NtrPlocBatchMesh> meshes;
    makeBatch(tris, verts, meshes, 9);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    const S32 M = (S32)meshes.size();

    CudaInstancedBVH batch;
    batch.buildBLASes(M, meshes.data(), scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer());
    const NtrPlocBatchResult& br = batch.getBLASBuildResult();
    CHECK(batch.getNumBLAS() == M && br.numMeshes == M && br.numTris > (int64_t)tris.size() && br.nodesBytes == batch.getPoolNodeBuffer().getSize());
    CHECK(br.triWoopBytes == batch.getPoolTriWoopBuffer().getSize() && br.triIndexBytes == batch.getPoolTriIndexBuffer().getSize());
    std::printf("buildBLASes: %d meshes, %lld triangles, %d rounds, height %d, %.3f ms\n", M, (long long)br.numTris, br.numRounds, br.maxHeight,
                br.seconds * 1e3f);

    // one builder call and one copy per BLAS: the same pool
    CudaInstancedBVH loop;
    for (S32 k = 0; k < M; k++) {
        Scene part(meshes[k].numTris, tris.data() + meshes[k].firstTri, (S32)verts.size(), verts.data());
        CudaPLOCBuilder one(&part);
        CHECK(loop.addBLAS(one) == k);
        CHECK(std::memcmp(&loop.getBLASRange(k), &batch.getBLASRange(k), sizeof(NtrBlasRange)) == 0);
    }
    Buffer *a[3] = {&batch.getPoolNodeBuffer(), &batch.getPoolTriWoopBuffer(), &batch.getPoolTriIndexBuffer()};
    Buffer *b[3] = {&loop.getPoolNodeBuffer(), &loop.getPoolTriWoopBuffer(), &loop.getPoolTriIndexBuffer()};
    for (int k = 0; k < 3; k++) CHECK(a[k]->getSize() == b[k]->getSize() && std::memcmp(a[k]->getPtr(), b[k]->getPtr(), (size_t)a[k]->getSize()) == 0);

    // the pool feeds the top-level build and the trace: one instance per BLAS, side by side
    std::vector<float> m(12 * (size_t)M, 0.0f);
    std::vector<S32> which((size_t)M);
    for (S32 i = 0; i < M; i++) {
        m[12 * i] = m[12 * i + 5] = m[12 * i + 10] = 1.0f;
        m[12 * i + 3] = 8.0f * (i - 2);
        which[i] = i;
    }
    batch.setInstances(M, m.data(), which.data());
    batch.build();
    CHECK(batch.getBuildResult().numNodes == M - 1);
    const int W = 64, H = 16;
    RayBuffer rays(W * H, true);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            Ray r;
            r.origin = Vec3f(-20.0f + 40.0f * (x + 0.5f) / W, -1.0f + 3.5f * (y + 0.5f) / H, -30.0f);
            r.direction = Vec3f(0.0f, 0.0f, 1.0f);
            r.tmin = 0.0f;
            r.tmax = 100.0f;
            rays.setRay(y * W + x, r);
        }
    Buffer ids;
    CHECK(batch.traceBatch(rays, ids) > 0.0f);
    const S32* id = (const S32*)ids.getPtr();
    bool seen[8] = {false, false, false, false, false, false, false, false};
    for (int i = 0; i < W * H; i++) {
        CHECK((rays.getResultForSlot(i).id >= 0) == (id[i] >= 0) && id[i] < M);
        if (id[i] >= 0) seen[id[i]] = true;
    }
    CHECK(seen[0] && seen[1] && seen[2] && seen[3]);
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
    if (g_failed) { std::printf("ploc_batch_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("ploc_batch_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
