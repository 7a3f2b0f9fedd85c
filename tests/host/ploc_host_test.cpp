// ploc_host_test.cpp -- the host mirror's PLOC path: Renderer("PLOCBVH") is a BVH builder traced by CudaBVHTracer, its cache file
// name carries the builder and the radius, the C-ABI checks its arguments before touching a device, and valid arguments without a
// device are NTR_ERR_NO_DEVICE / NTR_ERR_HIP with a zeroed result and untouched buffers (`cpu`); on a GPU (`gpu <dir>`)
// CudaPLOCBuilder through the Renderer, its CudaBVH stream round trip, getGPUTime / getBuildResult, primary + AO frames whose buffers
// and records are dumped for tests/test_bvh_ploc_host.py, then refit, optimizeBVH and reorderBVH on the same tree.  Compiled with
// plain g++ against libntrace_amd.so.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "Renderer.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

// a closed box room with two blocks inside, nTess^2 * 2 triangles per face
static void makeScene(std::vector<Vec3i>& tris, std::vector<Vec3f>& verts, int nTess)
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
    auto box = [&](Vec3f lo, Vec3f hi) {
        const Vec3f d = hi - lo;
        quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
        quad(Vec3f(lo.x, lo.y, hi.z), Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
        quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
        quad(Vec3f(lo.x, hi.y, lo.z), Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
        quad(lo, Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
        quad(Vec3f(hi.x, lo.y, lo.z), Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
    };
    box(Vec3f(-10.5f, -10.25f, -10.75f), Vec3f(10.25f, 10.5f, 10.125f));
    box(Vec3f(-3.5f, -10.25f, 1.5f), Vec3f(0.5f, -4.0f, 5.25f));
    box(Vec3f(2.25f, -10.25f, -2.0f), Vec3f(5.0f, -1.5f, 1.75f));
}

static CameraView makeCamera(int w, int h)
{
    CameraView c;
    c.position = Vec3f(0.3f, 0.7f, -9.0f);
    const float th = std::tan(0.5f), aspect = (float)w / h;
    const float m[16] = {th * aspect, 0, 0, c.position.x, 0, -th, 0, c.position.y, 0, 0, 0, c.position.z + 1.0f, 0, 0, 0, 1};
    std::memcpy(c.nscreenToWorld.m, m, sizeof(m));
    c.cameraFar = 100.0f;
    c.width = w;
    c.height = h;
    return c;
}

static bool sameBytes(Buffer& a, Buffer& b)
{
    return a.getSize() == b.getSize() && std::memcmp(a.getPtr(), b.getPtr(), (size_t)a.getSize()) == 0;
}

static void cpuTests()
{
    // the builder name selects the BVH data structure and its tracer; nothing is built without a scene
    Renderer r("PLOCBVH");
    CHECK(!r.isKDTree());
    CHECK(dynamic_cast<CudaBVHTracer*>(&r.getCudaTracer()) != NULL);
    CHECK(r.getCudaBVH() == NULL);
    // the cache file name carries the builder, and differs from every other builder's over the same scene
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 2);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Renderer::Params prm;
    prm.kernelName = "fermi_speculative_while_while";
    r.setScene(&scene);
    r.setParams(prm);
    CHECK(std::strstr(r.getCacheFileName().c_str(), "_PLOCBVH.dat") != NULL);
    const std::string mine = r.getCacheFileName().c_str();
    for (const char* other : {"SAHBVH", "HLBVH", "PersistentBVH", "DeviceSAHBVH"}) {
        Renderer o(other);
        o.setScene(&scene);
        o.setParams(prm);
        const std::string theirs = o.getCacheFileName().c_str();
        CHECK(theirs.substr(0, theirs.find('_')) != mine.substr(0, mine.find('_')));   // the hash, not only the name behind it
    }
    CHECK((int)CudaPLOCBuilder::DefaultRadius == 8);
    // arguments are checked before any device work, and a failed call zeroes its result
    NtrPlocResult res;
    int dummy = 0;
    const float mn[3] = {0, 0, 0}, mx[3] = {1, 1, 1}, inf[3] = {1, INFINITY, 1}, below[3] = {1, 1, -1};
    auto call = [&](int n, int nv, const float* lo, const float* hi, int radius, int64_t capN) {
        std::memset(&res, 0x5A, sizeof(res));
        return ntr_ploc_build(n, &dummy, nv, (const float*)&dummy, lo, hi, radius, &dummy, capN, &dummy, 1 << 20, &dummy, 1 << 20, &res, NULL);
    };
    CHECK(call(0, 3, mn, mx, 8, 1 << 20) == NTR_ERR_INVALID);
    CHECK(res.numNodes == 0 && res.nodesBytes == 0 && res.seconds == 0.0f && res.tailClusters == 0);
    CHECK(call(1, 0, mn, mx, 8, 1 << 20) == NTR_ERR_INVALID);
    CHECK(call(1, 3, NULL, mx, 8, 1 << 20) == NTR_ERR_INVALID);
    CHECK(call(1, 3, mn, mx, 0, 1 << 20) == NTR_ERR_INVALID && std::strstr(ntr_last_error(), "radius") != NULL);
    CHECK(call(1, 3, mn, mx, 65, 1 << 20) == NTR_ERR_INVALID && std::strstr(ntr_last_error(), "radius") != NULL);
    CHECK(call(1, 3, mn, inf, 8, 1 << 20) == NTR_ERR_INVALID && std::strstr(ntr_last_error(), "scene box") != NULL);
    CHECK(call(1, 3, mn, below, 8, 1 << 20) == NTR_ERR_INVALID && std::strstr(ntr_last_error(), "scene box") != NULL);
    CHECK(call(1, 3, mn, mx, 8, 64) == NTR_ERR_INVALID && std::strstr(ntr_last_error(), "ntr_lbvh_capacity") != NULL);
    CHECK(res.numNodes == 0 && res.nodesBytes == 0);
    CHECK(ntr_ploc_build(1, &dummy, 3, (const float*)&dummy, mn, mx, 8, &dummy, 1 << 20, &dummy, 1 << 20, &dummy, 1 << 20, NULL, NULL) ==
          NTR_ERR_INVALID);
    CHECK(ntr_ploc_scratch_bytes(NULL) == NTR_ERR_INVALID);
    // valid arguments and no device: there is no CPU fallback; the result is zeroed and no buffer is touched
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        int64_t capN, capW, capI;
        CHECK(ntr_lbvh_capacity(2, &capN, &capW, &capI) == NTR_OK);
        const int32_t tri[6] = {0, 1, 2, 1, 2, 3};
        const float pos[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1};
        std::vector<unsigned char> nodes((size_t)capN, 0xAB), woop((size_t)capW, 0xAB), index((size_t)capI, 0xAB);
        std::memset(&res, 0x5A, sizeof(res));
        const int rc = ntr_ploc_build(2, tri, 4, pos, mn, mx, 8, nodes.data(), capN, woop.data(), capW, (int32_t*)index.data(), capI, &res, NULL);
        CHECK(rc == NTR_ERR_NO_DEVICE || rc == NTR_ERR_HIP);
        const NtrPlocResult zero = NtrPlocResult();
        CHECK(std::memcmp(&res, &zero, sizeof(res)) == 0);
        auto untouched = [](const std::vector<unsigned char>& b) { for (unsigned char c : b) if (c != 0xAB) return false; return true; };
        CHECK(untouched(nodes) && untouched(woop) && untouched(index));
        int64_t held = -1;
        CHECK(ntr_ploc_scratch_bytes(&held) == NTR_OK && held == 0);
        std::printf("no device: ntr_ploc_build returned %d (%s)\n", rc, ntr_last_error());
    }
}

static void dump(const char* dir, const std::string& name, const void* data, size_t bytes)
{
    const std::string path = std::string(dir) + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != NULL);
    if (!f) return;
    if (bytes) std::fwrite(data, 1, bytes, f);
    std::fclose(f);
}
static void dump(const char* dir, const std::string& name, Buffer& b) { dump(dir, name, b.getPtr(), (size_t)b.getSize()); }

static void gpuTests(const char* dir)
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 24);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    dump(dir, "tris.bin", tris.data(), tris.size() * sizeof(Vec3i));
    dump(dir, "verts.bin", verts.data(), verts.size() * sizeof(Vec3f));
    const int W = 320, H = 200;
    const CameraView cam = makeCamera(W, H);
    Renderer::Params p;
    p.kernelName = "fermi_speculative_while_while";
    Renderer r("PLOCBVH");
    r.setScene(&scene);
    r.setParams(p);
    CudaPLOCBuilder* bvh = dynamic_cast<CudaPLOCBuilder*>(r.getCudaBVH());
    CHECK(bvh != NULL);
    if (!bvh) return;
    const NtrPlocResult& res = bvh->getBuildResult();
    CHECK(bvh->getLayout() == BVHLayout_Compact);
    CHECK(bvh->getNodeBuffer().getSize() == res.nodesBytes && bvh->getTriWoopBuffer().getSize() == res.triWoopBytes &&
          bvh->getTriIndexBuffer().getSize() == res.triIndexBytes);
    CHECK(bvh->getGPUTime() > 0.0f);
    CHECK(bvh->getRadius() == 8);
    CHECK(res.numNodes == (S32)tris.size() - 1 && res.numLeaves == (S32)tris.size());   // one triangle per leaf
    CHECK(res.numRounds >= res.height && res.height >= 1 && res.height <= 100);
    CHECK(res.tailClusters > 0 && res.tailClusters <= NTR_PLOC_TAIL);
    CHECK(res.triWoopBytes == 64 * (S64)tris.size() && res.triIndexBytes == 16 * (S64)tris.size());
    std::printf("PLOCBVH: %d inner nodes, %d rounds (tail from %d clusters), height %d, GPU %.3f ms\n", res.numNodes, res.numRounds,
                res.tailClusters, res.height, bvh->getGPUTime() * 1e3f);

    // serialize -> CudaBVH(std::istream&): the same buffers and layout, and the same stream again
    std::stringstream ss;
    bvh->serialize(ss);
    CudaBVH back(ss);
    CHECK(!hasError());
    CHECK(back.getLayout() == BVHLayout_Compact);
    CHECK(sameBytes(back.getNodeBuffer(), bvh->getNodeBuffer()));
    CHECK(sameBytes(back.getTriWoopBuffer(), bvh->getTriWoopBuffer()));
    CHECK(sameBytes(back.getTriIndexBuffer(), bvh->getTriIndexBuffer()));
    std::stringstream again;
    back.serialize(again);
    CHECK(again.str() == ss.str());
    dump(dir, "stream.bin", ss.str().data(), ss.str().size());
    dump(dir, "nodes.bin", bvh->getNodeBuffer());
    dump(dir, "woop.bin", bvh->getTriWoopBuffer());
    dump(dir, "index.bin", bvh->getTriIndexBuffer());

    // a primary frame
    r.beginFrame(cam);
    int batches = 0;
    while (r.nextBatch()) { r.traceBatch(); batches++; }
    CHECK(batches == 1);
    dump(dir, "primary_rays.bin", r.getPrimaryRays().getRayBuffer());
    dump(dir, "primary_results.bin", r.getPrimaryRays().getResultBuffer());

    // an AO frame over the same tree: every batch's rays and records, in batch order
    Renderer::Params ao = p;
    ao.rayType = Renderer::RayType_AO;
    ao.numSamples = 8;
    ao.aoRadius = 2.0f;
    r.setParams(ao);
    r.beginFrame(cam);
    std::string aoRays, aoResults;
    S64 numAo = 0, aoHits = 0;
    while (r.nextBatch()) {
        r.traceBatch();
        RayBuffer* rb = r.getBatchRays();
        aoRays.append((const char*)rb->getRayBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRay));
        aoResults.append((const char*)rb->getResultBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRayResult));
        const NtrRayResult* rr = (const NtrRayResult*)rb->getResultBuffer().getPtr();
        for (S32 i = 0; i < rb->getSize(); i++) aoHits += rr[i].id >= 0;
        numAo += rb->getSize();
    }
    CHECK(numAo == (S64)W * H * ao.numSamples && aoHits > 0 && aoHits < numAo);
    dump(dir, "ao_rays.bin", aoRays.data(), aoRays.size());
    dump(dir, "ao_results.bin", aoResults.data(), aoResults.size());
    std::printf("PLOCBVH: AO %lld rays, %lld hits\n", (long long)numAo, (long long)aoHits);

    // refit, the treelet passes and the reorder take the tree as any other Compact tree; it still traces
    r.refit();
    CHECK(dynamic_cast<CudaBVH*>(r.getCudaBVH())->getRefitResult().numNodes == res.numNodes);
    r.optimizeBVH(1);
    r.reorderBVH();
    r.setParams(p);
    r.beginFrame(cam);
    while (r.nextBatch()) r.traceBatch();
    const NtrRayResult* pr = (const NtrRayResult*)r.getPrimaryRays().getResultBuffer().getPtr();
    S64 hits = 0;
    for (int i = 0; i < W * H; i++) hits += pr[i].id >= 0;
    CHECK(hits == (S64)W * H);   // a closed room: every primary ray hits
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) gpuTests(argc > 2 ? argv[2] : "."); else cpuTests();
    } catch (const FatalError& e) {
        std::printf("unexpected FW::fail: %s\n", e.message.c_str());
        return 2;
    }
    std::printf("ploc_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
