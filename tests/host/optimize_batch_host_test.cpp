// optimize_batch_host_test.cpp -- CudaInstancedBVH::optimizeBLASes and measureBLASes (ntr_bvh_optimize_batch, ntr_bvh_sah_cost_batch;
// DESIGN.md 6v) in the frame loop they are made for: buildBLASes, the vertices move, refitBLASes, refit, optimizeBLASes.  `gpu <dir>`:
// isBuilt() and a world survive the restructuring, the wide pool is dropped and widen() restores it, and the pool before and after, the
// costs measured before and after, and the binary and the wide traceBatch's records, closest hit and any hit, are written to <dir> with
// the scene's buffers, for the test driver to run the numpy specs on.  Compiled with plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaInstancedBVH.hpp"

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

static void dump(const std::string& dir, const char* name, const void* p, size_t bytes)
{
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::printf("cannot write %s\n", path.c_str()); g_failed++; }
    if (f) std::fclose(f);
}

static void traces(CudaInstancedBVH& a, RayBuffer& rays, int n, const std::string& dir, const char* tag)
{
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        rays.setNeedClosestHit(!anyHit);
        Buffer ids;
        rays.getResultBuffer().clear(0x33);
        CHECK(a.traceBatch(rays, ids) > 0.0f);
        const S32* id = (const S32*)ids.getPtr();
        int hit = 0;
        for (int i = 0; i < n; i++) hit += id[i] >= 0 ? 1 : 0;
        CHECK(hit > n / 16);
        const std::string kind = std::string(tag) + (anyHit ? "_any.bin" : "_closest.bin");
        dump(dir, ("results_" + kind).c_str(), rays.getResultBuffer().getPtr(), (size_t)n * 16);
        dump(dir, ("ids_" + kind).c_str(), ids.getPtr(), (size_t)n * 4);
    }
}

static void gpuTests(const std::string& dir)
{
    // three meshes of very different sizes: 12, 300 and 768 triangles
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    int first[4] = {0, 0, 0, 0};
    addBox(tris, verts, Vec3f(-0.5f, -0.5f, -0.25f), Vec3f(0.25f, 0.75f, 0.5f), 1);
    first[1] = (int)tris.size();
    addBox(tris, verts, Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f), 5);
    first[2] = (int)tris.size();
    addBox(tris, verts, Vec3f(-1.0f, -1.0f, 0.25f), Vec3f(0.5f, 0.5f, 0.75f), 8);
    first[3] = (int)tris.size();
    std::vector<NtrPlocBatchMesh> meshes;
    for (int k = 0; k < 3; k++) {
        NtrPlocBatchMesh mm;
        mm.firstTri = first[k];
        mm.numTris = first[k + 1] - first[k];
        const float mn[3] = {-4.0f, -4.0f, -4.0f}, mx[3] = {4.0f, 4.0f, 4.0f};
        std::memcpy(mm.sceneMin, mn, sizeof(mn));
        std::memcpy(mm.sceneMax, mx, sizeof(mx));
        meshes.push_back(mm);
    }
    const S32 numVerts = (S32)verts.size();
    Buffer tri(tris.data(), (S64)tris.size() * 12), pos(verts.data(), (S64)numVerts * 12);

    const S32 M = 5, B = 3;
    std::vector<float> m(12 * (size_t)M, 0.0f);
    std::vector<S32> which((size_t)M);
    for (S32 i = 0; i < M; i++) {               // side by side along x: a rotation about z times a non-uniform scale; every third mirrored
        const float a = 0.3f * (float)(i + 1), c = std::cos(a), s = std::sin(a), sx = (i % 3 == 2) ? -2.5f : 2.5f, sy = 1.5f;
        float* t = &m[12 * (size_t)i];
        t[0] = c * sx; t[1] = -s * sy; t[3] = 6.0f * (float)(i - M / 2);
        t[4] = s * sx; t[5] = c * sy;  t[7] = 0.5f * (float)(i % 2);
        t[10] = 2.0f;
        which[i] = i % B;
    }
    CudaInstancedBVH a;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(M, m.data(), which.data());
    a.build();
    a.widen();
    CHECK(a.isBuilt() && a.isWide() && a.isWidePoolCurrent() && a.getBLASOptimizeResult().numEntries == 0);

    // the vertices move (a wave along every axis), the BLASes are refitted and the TLAS follows
    for (Vec3f& v : verts) {
        const Vec3f p = v;
        v = Vec3f(p.x + 0.2f * std::sin(4.0f * p.y), p.y + 0.2f * std::sin(4.0f * p.z + 1.0f), p.z + 0.2f * std::sin(4.0f * p.x + 2.0f));
    }
    Buffer moved(verts.data(), (S64)numVerts * 12);
    a.refitBLASes(tri, numVerts, moved);
    a.refit();
    CHECK(a.isBuilt() && !a.isWidePoolCurrent());
    a.widen();
    CHECK(a.isWide());

    std::vector<NtrBlasRange> ranges;
    for (S32 k = 0; k < B; k++) ranges.push_back(a.getBLASRange(k));
    std::vector<NtrBvhSahResult> before, after, some;
    a.measureBLASes(before);
    CHECK(before.size() == 3 && before[0].numTris == 12 && before[1].numTris == 300 && before[2].numTris == 768);
    dump(dir, "pool_refitted.bin", a.getPoolNodeBuffer().getPtr(), (size_t)a.getPoolNodeBuffer().getSize());
    std::vector<unsigned char> tlasBefore((size_t)(64 * (M - 1))), recBefore((size_t)M * 64);
    std::memcpy(tlasBefore.data(), a.getTLASNodeBuffer().getPtr(), tlasBefore.size());
    std::memcpy(recBefore.data(), a.getRecordBuffer().getPtr(), recBefore.size());

    // the repair: two treelet passes over every BLAS.  The TLAS stays current, the wide pool does not
    a.optimizeBLASes();
    const NtrBvhOptimizeBatchResult res = a.getBLASOptimizeResult();
    CHECK(a.isBuilt() && !a.isWidePoolCurrent() && !a.isWide());
    CHECK(res.numEntries == 3 && res.passes == 2 && res.firstBadEntry == -1 && res.errBits == 0 && res.seconds > 0.0f);
    CHECK(res.formed[0] >= 3 && res.rewritten[0] > 0 && res.formed[2] == 0 && res.readBacks == 3);
    CHECK(res.launches <= 2 * (5 + std::max(res.maxHeightBefore, res.maxHeightAfter)) + 2);
    a.measureBLASes(after);
    const S32 pick[3] = {2, 0, 2};               // a selection in another order, one BLAS twice: the cost only reads
    a.measureBLASes(some, pick, 3);
    CHECK(some.size() == 3 && std::memcmp(&some[0], &after[2], sizeof(NtrBvhSahResult)) == 0 &&
          std::memcmp(&some[1], &after[0], sizeof(NtrBvhSahResult)) == 0 && std::memcmp(&some[2], &after[2], sizeof(NtrBvhSahResult)) == 0);
    for (S32 k = 0; k < B; k++) {
        CHECK(after[k].numTris == before[k].numTris && after[k].numLeaves == before[k].numLeaves && after[k].numNodes == before[k].numNodes);
        CHECK(after[k].seconds == 0.0f);
    }
    CHECK(after[1].sahCost < before[1].sahCost && after[2].sahCost < before[2].sahCost);
    dump(dir, "sah_before.bin", before.data(), before.size() * sizeof(NtrBvhSahResult));
    dump(dir, "sah_after.bin", after.data(), after.size() * sizeof(NtrBvhSahResult));
    dump(dir, "optimize_result.bin", &res, sizeof(res));
    // a second call on a selection: only BLAS 1, one pass
    const S32 only[1] = {1};
    a.optimizeBLASes(only, 1, 1);
    CHECK(a.getBLASOptimizeResult().numEntries == 1 && a.getBLASOptimizeResult().passes == 1 && a.isBuilt());
    dump(dir, "pool_optimized.bin", a.getPoolNodeBuffer().getPtr(), (size_t)a.getPoolNodeBuffer().getSize());
    // the TLAS was not touched, and a refit over the optimised pool writes the bytes it holds: every node-0 union kept its bits
    CHECK(std::memcmp(tlasBefore.data(), a.getTLASNodeBuffer().getPtr(), tlasBefore.size()) == 0);
    a.refit();
    CHECK(std::memcmp(tlasBefore.data(), a.getTLASNodeBuffer().getPtr(), tlasBefore.size()) == 0);
    CHECK(std::memcmp(recBefore.data(), a.getRecordBuffer().getPtr(), recBefore.size()) == 0);

    // rays: a grid from the -z side along +z with a slight fan, over all five instances
    const int W = 64, H = 24, n = W * H;
    RayBuffer rays(n);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            Ray r;
            r.origin = Vec3f(-16.0f + 32.0f * ((F32)x + 0.5f) / W, -3.0f + 6.0f * ((F32)y + 0.5f) / H, -30.0f);
            r.direction = Vec3f(0.01f * (F32)(x % 5 - 2), 0.01f * (F32)(y % 3 - 1), 1.0f);
            r.tmin = 0.0f;
            r.tmax = 200.0f;
            rays.setRay(y * W + x, r);
        }
    traces(a, rays, n, dir, "binary");
    // refitBLASesWide needs the wide pool of the new topology: it refuses until widen() has run
    bool refused = false;
    try {
        a.refitBLASesWide(tri, numVerts, moved);
    } catch (const FatalError&) {
        refused = true;
    }
    CHECK(refused);
    a.widen();
    CHECK(a.isWide() && a.isWidePoolCurrent());
    a.setTraceWide(true);
    traces(a, rays, n, dir, "wide");
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
    dump(dir, "pool_woop.bin", a.getPoolTriWoopBuffer().getPtr(), (size_t)a.getPoolTriWoopBuffer().getSize());
    dump(dir, "pool_index.bin", a.getPoolTriIndexBuffer().getPtr(), (size_t)a.getPoolTriIndexBuffer().getSize());
    dump(dir, "wide_pool.bin", a.getWidePoolNodeBuffer().getPtr(), (size_t)a.getWidePoolResult().nodesBytes);
    dump(dir, "tlas_nodes.bin", a.getTLASNodeBuffer().getPtr(), (size_t)(64 * (M - 1)));
    dump(dir, "records.bin", a.getRecordBuffer().getPtr(), (size_t)M * 64);
    dump(dir, "instances.bin", a.getInstanceBuffer().getPtr(), (size_t)M * sizeof(NtrInstance));
    dump(dir, "rays.bin", rays.getRayBuffer().getPtr(), (size_t)n * 32);
    dump(dir, "ranges.bin", ranges.data(), ranges.size() * sizeof(NtrBlasRange));

    // a world set by setWorld survives, and so does isBuilt(); an addBLAS tree has no mesh and is optimised all the same
    CudaInstancedBVH w;
    w.buildBLASes(B, meshes.data(), tri, numVerts, moved);
    w.setWorld(1);
    w.setInstances(M, m.data(), which.data());
    w.build();
    const S32 world[1] = {1};
    w.optimizeBLASes(world, 1, 8);
    CHECK(w.hasWorld() && w.getWorldBLAS() == 1 && w.isBuilt() && w.getBLASOptimizeResult().passes == 8);
    Buffer ids;
    rays.setNeedClosestHit(true);
    CHECK(w.traceBatch(rays, ids) > 0.0f);
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
    bool bad = false;
    try {
        const S32 out[1] = {3};
        w.optimizeBLASes(out, 1);
    } catch (const FatalError&) {
        bad = true;
    }
    CHECK(bad);
}

int main(int argc, char** argv)
{
    if (argc < 3 || std::strcmp(argv[1], "gpu") != 0) { std::printf("usage: optimize_batch_host_test gpu <dir>\n"); return 2; }
    try {
        gpuTests(argv[2]);
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        g_failed++;
    }
    if (g_failed) { std::printf("optimize_batch_host_test gpu: %d check(s) FAILED\n", g_failed); return 1; }
    std::printf("optimize_batch_host_test gpu: ok\n");
    return 0;
}
