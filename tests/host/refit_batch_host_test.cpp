// refit_batch_host_test.cpp -- the host mirror's batched BLAS refit (CudaInstancedBVH::refitBLASes over ntr_bvh_refit_batch): a call
// before there is a BLAS, a selection of an addBLAS tree (it has no mesh here) and a bad index are refused, and without a device
// buildBLASes leaves nothing that could be refitted (`cpu`); on a GPU (`gpu`) buildBLASes, moved vertices, refitBLASes, build() and
// traceBatch: the pool equals, byte for byte, the pool addBLAS makes of one CudaPLOCBuilder tree per mesh after one CudaBVH::refit each,
// and the trace's records and instance ids equal those over that pool.  Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "CudaInstancedBVH.hpp"
#include "CudaPLOCBuilder.hpp"
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

// three boxes in one index array; the meshes: the boxes, the second box once more, and one triangle, each over the box of all vertices
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

template <class Call>
static bool refused(Call call, const char* word)
{
    try { call(); } catch (const FatalError& e) {
        if (std::strstr(e.message.c_str(), word)) return true;
        std::printf("refused with another message: %s\n", e.message.c_str());
    }
    return false;
}

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    std::vector<NtrPlocBatchMesh> meshes;
    makeBatch(tris, verts, meshes, 2);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Buffer &tri = scene.getTriVtxIndexBuffer(), &pos = scene.getVtxPosBuffer();
    const S32 nv = scene.getNumVertices();

    CudaInstancedBVH inst;
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos); }, "buildBLASes first"));
    CHECK(inst.getBLASRefitResult().numEntries == 0);

    // a tree that came through addBLAS has no mesh here
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CHECK(inst.addBLAS(sah) == 0);
    const S32 zero = 0, five = 5, minus = -1;
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos); }, "addBLAS"));
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos, &zero, 1); }, "addBLAS"));
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos, &five, 1); }, "outside"));
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos, &minus, 1); }, "outside"));
    CHECK(refused([&] { inst.refitBLASes(tri, nv, pos, &zero, 0); }, "selected"));
    Buffer empty;
    CHECK(refused([&] { inst.refitBLASes(empty, nv, pos, &zero, 1); }, "mesh buffers"));

    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        // without a device no mesh ever gets here: buildBLASes fails with the library's message and leaves no BLAS behind
        CudaInstancedBVH none;
        bool threw = false;
        try { none.buildBLASes((S32)meshes.size(), meshes.data(), tri, nv, pos); }
        catch (const FatalError& e) { threw = true; std::printf("no device: buildBLASes refused (%s)\n", e.message.c_str()); }
        CHECK(threw && none.getNumBLAS() == 0);
        CHECK(refused([&] { none.refitBLASes(tri, nv, pos); }, "buildBLASes first"));
        int64_t held = -1;
        CHECK(ntr_bvh_refit_batch_scratch_bytes(&held) == NTR_OK && held == 0);
    }
}

static void instancesSideBySide(CudaInstancedBVH& inst, S32 M)
{
    std::vector<float> m(12 * (size_t)M, 0.0f);
    std::vector<S32> which((size_t)M);
    for (S32 i = 0; i < M; i++) {
        m[12 * i] = m[12 * i + 5] = m[12 * i + 10] = 1.0f;
        m[12 * i + 3] = 8.0f * (i - 2);
        which[i] = i;
    }
    inst.setInstances(M, m.data(), which.data());
    inst.build();
}

static void fillRays(RayBuffer& rays, int W, int H)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            Ray r;
            r.origin = Vec3f(-20.0f + 40.0f * (x + 0.5f) / W, -1.5f + 4.5f * (y + 0.5f) / H, -30.0f);
            r.direction = Vec3f(0.0f, 0.0f, 1.0f);
            r.tmin = 0.0f;
            r.tmax = 100.0f;
            rays.setRay(y * W + x, r);
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
    // one builder call per BLAS over the same vertices: the trees that are refitted one by one below
    std::vector<std::unique_ptr<Scene>> parts;
    std::vector<std::unique_ptr<CudaPLOCBuilder>> trees;
    for (S32 k = 0; k < M; k++) {
        parts.emplace_back(new Scene(meshes[k].numTris, tris.data() + meshes[k].firstTri, (S32)verts.size(), verts.data()));
        trees.emplace_back(new CudaPLOCBuilder(parts.back().get()));
    }

    // the meshes deform: every vertex moves along a wave, the triangles stay
    std::vector<Vec3f> moved(verts);
    for (Vec3f& v : moved) v = v + Vec3f(0.21f * std::sin(2.0f * v.y + 0.3f), 0.17f * std::sin(3.0f * v.z + 1.1f), 0.13f * std::sin(2.5f * v.x + 2.3f));
    scene.setVertexPositions(moved.data());
    batch.refitBLASes(scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer());
    const NtrBvhRefitBatchResult& rr = batch.getBLASRefitResult();
    int64_t nodes = 0, leaves = 0;
    for (S32 k = 0; k < M; k++) {
        nodes += meshes[k].numTris == 1 ? 1 : meshes[k].numTris - 1;
        leaves += meshes[k].numTris == 1 ? 2 : meshes[k].numTris;
    }
    CHECK(rr.numEntries == M && rr.lanesPerLeaf == 1 && rr.firstBadEntry == -1 && rr.errBits == 0 && rr.seconds > 0.0f);
    CHECK(rr.numNodes == nodes && rr.numLeaves == leaves && rr.numRows == batch.getPoolTriWoopBuffer().getSize() / 16);
    std::printf("refitBLASes: %d BLASes, %lld nodes, %.1f us\n", M, (long long)rr.numNodes, rr.seconds * 1e6f);

    CudaInstancedBVH loop;
    for (S32 k = 0; k < M; k++) {
        parts[k]->setVertexPositions(moved.data());
        trees[k]->refit(*parts[k]);
        CHECK(loop.addBLAS(*trees[k]) == k);
        CHECK(std::memcmp(&loop.getBLASRange(k), &batch.getBLASRange(k), sizeof(NtrBlasRange)) == 0);
    }
    Buffer *a[3] = {&batch.getPoolNodeBuffer(), &batch.getPoolTriWoopBuffer(), &batch.getPoolTriIndexBuffer()};
    Buffer *b[3] = {&loop.getPoolNodeBuffer(), &loop.getPoolTriWoopBuffer(), &loop.getPoolTriIndexBuffer()};
    for (int k = 0; k < 3; k++) CHECK(a[k]->getSize() == b[k]->getSize() && std::memcmp(a[k]->getPtr(), b[k]->getPtr(), (size_t)a[k]->getSize()) == 0);

    // build() rebuilds the TLAS from the new node-0 boxes; nothing else is needed.  The records equal those over the loop's pool
    instancesSideBySide(batch, M);
    instancesSideBySide(loop, M);
    CHECK(batch.getBuildResult().numNodes == M - 1);
    CHECK(std::memcmp(&batch.getBuildResult().sceneMin, &loop.getBuildResult().sceneMin, 6 * sizeof(float)) == 0);
    const int W = 64, H = 24;
    RayBuffer ra(W * H, true), rb(W * H, true);
    fillRays(ra, W, H);
    fillRays(rb, W, H);
    Buffer ia, ib;
    CHECK(batch.traceBatch(ra, ia) > 0.0f && loop.traceBatch(rb, ib) > 0.0f);
    CHECK(std::memcmp(ra.getResultBuffer().getPtr(), rb.getResultBuffer().getPtr(), (size_t)ra.getResultBuffer().getSize()) == 0);
    CHECK(ia.getSize() == ib.getSize() && std::memcmp(ia.getPtr(), ib.getPtr(), (size_t)ia.getSize()) == 0);
    const S32* id = (const S32*)ia.getPtr();
    bool seen[8] = {false, false, false, false, false, false, false, false};
    for (int i = 0; i < W * H; i++) {
        CHECK((ra.getResultForSlot(i).id >= 0) == (id[i] >= 0) && id[i] < M);
        if (id[i] >= 0) seen[id[i]] = true;
    }
    CHECK(seen[0] && seen[1] && seen[2] && seen[3]);

    // a selection: back to the first positions for BLASes 3 and 0 only, in that order; the others keep the moved ones
    scene.setVertexPositions(verts.data());
    const S32 sel[2] = {3, 0};
    batch.refitBLASes(scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer(), sel, 2);
    CHECK(batch.getBLASRefitResult().numEntries == 2);
    CudaInstancedBVH loop2;
    for (S32 k = 0; k < M; k++) {
        if (k == 3 || k == 0) {
            parts[k]->setVertexPositions(verts.data());
            trees[k]->refit(*parts[k]);
        }
        loop2.addBLAS(*trees[k]);
    }
    Buffer *c[3] = {&loop2.getPoolNodeBuffer(), &loop2.getPoolTriWoopBuffer(), &loop2.getPoolTriIndexBuffer()};
    for (int k = 0; k < 3; k++) CHECK(a[k]->getSize() == c[k]->getSize() && std::memcmp(a[k]->getPtr(), c[k]->getPtr(), (size_t)a[k]->getSize()) == 0);
    // a BLAS named twice is refused by the library (two threads would refit one tree)
    const S32 twice[2] = {1, 1};
    CHECK(refused([&] { batch.refitBLASes(scene.getTriVtxIndexBuffer(), scene.getNumVertices(), scene.getVtxPosBuffer(), twice, 2); }, "overlap"));
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
    if (g_failed) { std::printf("refit_batch_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("refit_batch_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
