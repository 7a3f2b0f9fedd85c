// pool_widen_batch_host_test.cpp -- CudaInstancedBVH::widen over a pool of three BLASes, which takes the batched pass
// (ntr_pool_widen_batch).  `gpu <dir>`: the wide pool the object holds equals ntr_pool_widen's byte for byte, a pool of one
// BLAS widens too (the single call), and the wide traceBatch's records, closest hit and any hit, are written to <dir> with the scene's
// buffers, for the test driver to run the numpy spec on.  Compiled with plain g++ against libntrace_amd.so.
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
    CHECK(a.isWide() && a.isWidePoolCurrent() && a.getNumBLAS() == 3);
    const NtrBvhWideResult got = a.getWidePoolResult();
    CHECK(got.nodesBytes >= 3 * 128 && got.seconds > 0.0f);

    // the loop, into a buffer of its own: the same bytes, ranges and totals
    std::vector<NtrBlasRange> ranges;
    for (S32 k = 0; k < B; k++) ranges.push_back(a.getBLASRange(k));
    int64_t cap = 0;
    CHECK(ntr_pool_widen_capacity(B, ranges.data(), &cap) == NTR_OK);
    Buffer loopPool;
    loopPool.resizeDiscard(cap);
    NtrWideBlasRange loopRanges[3];
    NtrBvhWideResult loop;
    CHECK(ntr_pool_widen(B, ranges.data(), a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(), loopPool.getMutableCudaPtr(), cap,
                         loopRanges, &loop, NULL) == NTR_OK);
    CHECK(loop.nodesBytes == got.nodesBytes && loop.numNodes == got.numNodes && loop.numLeafLinks == got.numLeafLinks);
    CHECK(loop.height == got.height && loop.stackBound == got.stackBound && std::memcmp(loop.counts, got.counts, sizeof(loop.counts)) == 0);
    CHECK(std::memcmp(loopPool.getPtr(), a.getWidePoolNodeBuffer().getPtr(), (size_t)got.nodesBytes) == 0);
    // (the wide records hold each BLAS's offset and extent: the ranges the object keeps)
    const U32* rec = (const U32*)a.getWideRecordBuffer().getPtr();
    for (S32 i = 0; i < M; i++)
        CHECK((int64_t)rec[16 * i + 12] == loopRanges[which[i]].nodesOffset && (int64_t)rec[16 * i + 14] == loopRanges[which[i]].nodesBytes);

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
    a.setTraceWide(true);
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        rays.setNeedClosestHit(!anyHit);
        Buffer ids;
        rays.getResultBuffer().clear(0x33);
        CHECK(a.traceBatch(rays, ids) > 0.0f);
        const S32* id = (const S32*)ids.getPtr();
        int hit = 0;
        for (int i = 0; i < n; i++) hit += id[i] >= 0 ? 1 : 0;
        CHECK(hit > n / 16);
        dump(dir, anyHit ? "results_any.bin" : "results_closest.bin", rays.getResultBuffer().getPtr(), (size_t)n * 16);
        dump(dir, anyHit ? "ids_any.bin" : "ids_closest.bin", ids.getPtr(), (size_t)n * 4);
    }
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
    dump(dir, "pool_nodes.bin", a.getPoolNodeBuffer().getPtr(), (size_t)a.getPoolNodeBuffer().getSize());
    dump(dir, "pool_woop.bin", a.getPoolTriWoopBuffer().getPtr(), (size_t)a.getPoolTriWoopBuffer().getSize());
    dump(dir, "pool_index.bin", a.getPoolTriIndexBuffer().getPtr(), (size_t)a.getPoolTriIndexBuffer().getSize());
    dump(dir, "wide_pool.bin", a.getWidePoolNodeBuffer().getPtr(), (size_t)got.nodesBytes);
    dump(dir, "tlas_nodes.bin", a.getTLASNodeBuffer().getPtr(), (size_t)(64 * (M - 1)));
    dump(dir, "instances.bin", a.getInstanceBuffer().getPtr(), (size_t)M * sizeof(NtrInstance));
    dump(dir, "rays.bin", rays.getRayBuffer().getPtr(), (size_t)n * 32);
    dump(dir, "ranges.bin", ranges.data(), ranges.size() * sizeof(NtrBlasRange));

    // a pool of one BLAS keeps the single call: it widens and traces all the same
    CudaInstancedBVH one;
    one.buildBLASes(1, meshes.data() + 1, tri, numVerts, pos);
    S32 zero[2] = {0, 0};
    one.setInstances(2, m.data(), zero);
    one.build();
    one.widen();
    CHECK(one.isWide() && one.getNumBLAS() == 1 && one.getWidePoolResult().nodesBytes >= 128);
}

int main(int argc, char** argv)
{
    if (argc < 3 || std::strcmp(argv[1], "gpu") != 0) { std::printf("usage: pool_widen_batch_host_test gpu <dir>\n"); return 2; }
    try {
        gpuTests(argv[2]);
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        g_failed++;
    }
    if (g_failed) { std::printf("pool_widen_batch_host_test gpu: %d check(s) FAILED\n", g_failed); return 1; }
    std::printf("pool_widen_batch_host_test gpu: ok\n");
    return 0;
}
