// motion_refit_batch_host_test.cpp -- CudaInstancedBVH::refitBLASesMotion over ntr_bvh_motion_refit_batch.  `cpu`: what
// needs no device.  `gpu <dir>`: a pool of five BLASes that the test driver writes into <dir>.  After refitBLASesMotion the five pool
// buffers equal, byte for byte, what the loop it replaced leaves -- one ntr_bvh_motion_refit per selected BLAS at pool + offset, made here
// on copies of the pool as built -- for all BLASes, for a subset in scrambled order, and for a second call that keeps the earlier
// deforming BLASes; getBLASMotionRefitResult() holds the sums of the loop's results.  Then one batch of the driver's rays is traced: the
// records equal the ones the driver's numpy rule wrote into <dir>, and are written back for the driver.  Compiled with plain g++ against
// libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaInstancedBVH.hpp"
#include "RayBuffer.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

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

static void dump(const std::string& dir, const char* name, const void* p, size_t bytes)
{
    const std::string path = dir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::printf("cannot write %s\n", path.c_str()); g_failed++; }
    if (f) std::fclose(f);
}

static void cpuTests()
{
    CudaInstancedBVH a;
    const NtrBvhRefitBatchResult& r = a.getBLASMotionRefitResult();
    CHECK(r.numEntries == 0 && r.numNodes == 0 && r.numLeaves == 0 && r.numRows == 0 && r.seconds == 0.0f);
    Buffer tri, pos;
    tri.resizeDiscard(12);
    pos.resizeDiscard(36);
    bool refused = false;
    try { a.refitBLASesMotion(tri, 3, pos, pos); } catch (const FatalError& e) { refused = std::strstr(e.message.c_str(), "no BLASes to refit") != NULL; }
    CHECK(refused && a.getBLASMotionRefitResult().numEntries == 0);
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the result is bookkeeping only\n");
}

// The loop refitBLASesMotion made before the batch call: five buffers of the test's own, and the sums of the per-BLAS results.
struct Loop {
    Buffer nodes0, nodes1, woop, rows0, rows1;
    S64 numNodes = 0, numLeaves = 0, numRows = 0;

    void start(CudaInstancedBVH& built)           // the pool as built; the key-1 buffers hold 0xCD
    {
        nodes0.set(built.getPoolNodeBuffer());
        woop.set(built.getPoolTriWoopBuffer());
        nodes1.resizeDiscard(nodes0.getSize());
        rows0.resizeDiscard(woop.getSize());
        rows1.resizeDiscard(woop.getSize());
        nodes1.clear(0xCD);
        rows0.clear(0xCD);
        rows1.clear(0xCD);
    }
    void refit(CudaInstancedBVH& a, const std::vector<NtrPlocBatchMesh>& meshes, const S32* sel, S32 num, Buffer& tri, S32 numVerts, Buffer& pos0,
               Buffer& pos1)
    {
        numNodes = numLeaves = numRows = 0;
        U8 *n0 = (U8*)nodes0.getMutableCudaPtr(), *n1 = (U8*)nodes1.getMutableCudaPtr(), *w = (U8*)woop.getMutableCudaPtr();
        U8 *r0 = (U8*)rows0.getMutableCudaPtr(), *r1 = (U8*)rows1.getMutableCudaPtr();
        const U8* index = (const U8*)a.getPoolTriIndexBuffer().getCudaPtr();
        for (S32 i = 0; i < num; i++) {
            const S32 b = sel[i];
            const NtrBlasRange r = a.getBLASRange(b);
            NtrBvhRefitResult res;
            CHECK(ntr_bvh_motion_refit(n0 + r.nodesOffset, r.nodesBytes, n1 + r.nodesOffset, w + r.triWoopOffset, r.triWoopBytes,
                                       (const int32_t*)(index + r.triWoopOffset / 4), r.triWoopBytes / 4, r0 + r.triWoopOffset, r1 + r.triWoopOffset,
                                       meshes[(size_t)b].numTris, (const int32_t*)tri.getCudaPtr() + 3 * (size_t)meshes[(size_t)b].firstTri, numVerts,
                                       (const float*)pos0.getCudaPtr(), (const float*)pos1.getCudaPtr(), 0.0f, NULL, &res, NULL) == NTR_OK);
            numNodes += res.numNodes;
            numLeaves += res.numLeaves;
            numRows += res.numRows;
        }
    }
    // the mirror's five buffers against these: nodes0 and the Woop rows whole, the key-1 buffers over the BLASes in `deforming`
    void same(CudaInstancedBVH& a, const std::vector<S32>& deforming, const char* what)
    {
        const bool whole = a.getPoolNodeBuffer().getSize() == nodes0.getSize() && a.getPoolTriWoopBuffer().getSize() == woop.getSize() &&
                           std::memcmp(a.getPoolNodeBuffer().getPtr(), nodes0.getPtr(), (size_t)nodes0.getSize()) == 0 &&
                           std::memcmp(a.getPoolTriWoopBuffer().getPtr(), woop.getPtr(), (size_t)woop.getSize()) == 0;
        bool key1 = a.getPoolNode1Buffer().getSize() == nodes1.getSize() && a.getPoolVertRowBuffer(0).getSize() == rows0.getSize() &&
                    a.getPoolVertRowBuffer(1).getSize() == rows1.getSize();
        for (size_t i = 0; key1 && i < deforming.size(); i++) {
            const NtrBlasRange r = a.getBLASRange(deforming[i]);
            key1 = std::memcmp((const U8*)a.getPoolNode1Buffer().getPtr() + r.nodesOffset, (const U8*)nodes1.getPtr() + r.nodesOffset, (size_t)r.nodesBytes) == 0 &&
                   std::memcmp((const U8*)a.getPoolVertRowBuffer(0).getPtr() + r.triWoopOffset, (const U8*)rows0.getPtr() + r.triWoopOffset, (size_t)r.triWoopBytes) == 0 &&
                   std::memcmp((const U8*)a.getPoolVertRowBuffer(1).getPtr() + r.triWoopOffset, (const U8*)rows1.getPtr() + r.triWoopOffset, (size_t)r.triWoopBytes) == 0;
        }
        const NtrBvhRefitBatchResult& res = a.getBLASMotionRefitResult();
        const bool sums = res.numNodes == numNodes && res.numLeaves == numLeaves && res.numRows == numRows && res.firstBadEntry == -1 &&
                          res.errBits == 0 && res.seconds > 0.0f && (res.lanesPerLeaf == 1 || res.lanesPerLeaf == 4 || res.lanesPerLeaf == 8);
        if (whole && key1 && sums) std::printf("%s: the five pool buffers and the sums equal the loop's\n", what);
        else { std::printf("%s: DIFFERS from the loop (nodes0/woop %d, key 1 %d, sums %d)\n", what, (int)whole, (int)key1, (int)sums); g_failed++; }
    }
};

static void gpuTests(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
    std::vector<float> vtx = load<float>(dir, "pos.bin"), vtx1 = load<float>(dir, "pos1.bin"), vtx2 = load<float>(dir, "pos2.bin");
    std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
    std::vector<float> xf = load<float>(dir, "transforms.bin");
    std::vector<S32> which = load<S32>(dir, "blas.bin");
    std::vector<float> rays = load<float>(dir, "rays.bin"), times = load<float>(dir, "times.bin");
    std::vector<U8> wantResults = load<U8>(dir, "want_results.bin"), wantIds = load<U8>(dir, "want_ids.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size(), n = (S32)rays.size() / 8;
    CHECK(numTris > 0 && B == 5 && N > 0 && (S32)xf.size() == 12 * N && vtx1.size() == vtx.size() && vtx2.size() == vtx.size());
    CHECK(n > 0 && (S32)times.size() == n && wantResults.size() == (size_t)n * 16 && wantIds.size() == (size_t)n * 4);
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12), pos1(vtx1.data(), (S64)numVerts * 12),
           pos2(vtx2.data(), (S64)numVerts * 12);

    // every BLAS in one call
    {
        CudaInstancedBVH a;
        a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
        Loop loop;
        loop.start(a);
        const S32 all[5] = {0, 1, 2, 3, 4};
        a.refitBLASesMotion(tri, numVerts, pos, pos1);
        loop.refit(a, meshes, all, 5, tri, numVerts, pos, pos1);
        loop.same(a, std::vector<S32>(all, all + 5), "all five BLASes");
        CHECK(a.hasDeform() && a.getBLASMotionRefitResult().numEntries == 5);
    }

    // a subset in scrambled order, then a second call that keeps it
    CudaInstancedBVH a;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    Loop loop;
    loop.start(a);
    const S32 first[2] = {3, 1}, second[1] = {4};
    a.refitBLASesMotion(tri, numVerts, pos, pos1, first, 2);
    loop.refit(a, meshes, first, 2, tri, numVerts, pos, pos1);
    loop.same(a, std::vector<S32>(first, first + 2), "BLASes 3 and 1 of five");
    CHECK(a.hasDeform() && a.getBLASMotionRefitResult().numEntries == 2);
    a.refitBLASesMotion(tri, numVerts, pos, pos2, second, 1);
    loop.refit(a, meshes, second, 1, tri, numVerts, pos, pos2);
    const S32 kept[3] = {3, 1, 4};
    loop.same(a, std::vector<S32>(kept, kept + 3), "then BLAS 4: the earlier two are kept");
    CHECK(a.hasDeform() && a.getBLASMotionRefitResult().numEntries == 1);
    const U32 wantFlags[5] = {0u, 1u, 0u, 1u, 1u};
    CHECK(a.getBLASDeformingBuffer().getSize() == 20 && std::memcmp(a.getBLASDeformingBuffer().getPtr(), wantFlags, 20) == 0);

    // one traced batch: the top-level tree over the refitted pool, the lazy deform refit, the driver's rays at the driver's times
    a.build();
    RayBuffer p(n);
    for (S32 i = 0; i < n; i++) {
        Ray r;
        static_assert(sizeof(Ray) == 32, "a ray is eight words");
        std::memcpy((void*)&r, &rays[(size_t)i * 8], 32);
        p.setRay(i, r);
    }
    Buffer rayTimes(times.data(), (S64)n * 4), ids;
    a.setRayTimes(&rayTimes);
    p.getResultBuffer().clear(0x33);
    CHECK(a.isMotionStale());
    CHECK(a.traceBatch(p, ids) > 0.0f);
    CHECK(!a.isMotionStale() && a.getDeformRefitResult().numDeforming > 0);
    const bool same = std::memcmp(p.getResultBuffer().getPtr(), wantResults.data(), (size_t)n * 16) == 0 && ids.getSize() == (S64)n * 4 &&
                      std::memcmp(ids.getPtr(), wantIds.data(), (size_t)n * 4) == 0;
    int hits = 0;
    const NtrRayResult* res = (const NtrRayResult*)p.getResultBuffer().getPtr();
    for (S32 i = 0; i < n; i++) hits += res[i].id != -1 ? 1 : 0;
    if (same && hits > 0) std::printf("the traced batch equals the rule: %d rays, %d hits\n", (int)n, hits);
    else { std::printf("the traced batch DIFFERS from the rule (%d hits)\n", hits); g_failed++; }
    dump(dir, "out_results.bin", p.getResultBuffer().getPtr(), (size_t)n * 16);
    dump(dir, "out_ids.bin", ids.getPtr(), (size_t)ids.getSize());
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
    if (g_failed) { std::printf("motion_refit_batch_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("motion_refit_batch_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
