// kdtree_host_test.cpp -- the host mirror's kd-tree path: KDTree + CudaKDTree and their stream round trip (`cpu`), and Renderer frames
// over "SAHKDTree" (primary + AO) beside an "SAHBVH" frame (`gpu <dir>`: buffers and records dumped for tests/test_kdtree_host.py).
// Compiled with plain g++ against libntrace_amd.so.
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
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 6);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Platform platform("GPU");
    platform.setLeafPreferences(1, 1);
    for (const char* builder : {"SpatialMedianKDTree", "SAHKDTree"}) {
        KDTree::Stats st;
        KDTree::BuildParams params;
        params.builder = builder;
        params.stats = &st;
        KDTree kdtree(&scene, platform, params);
        CudaKDTree kd(kdtree);
        CHECK(kd.getNodeBuffer().getSize() == (S64)st.numInnerNodes * 16 && st.numInnerNodes > 1);
        CHECK(kd.getTriWoopBuffer().getSize() == (((S64)tris.size() * 48 + 4095) & ~(S64)4095));
        CHECK(st.maxDepth >= 1 && st.numLeafNodes == st.numInnerNodes + 1);
        // serialize -> CudaKDTree(InputStream&): the same buffers and box
        std::stringstream ss;
        kd.serialize(ss);
        CudaKDTree back(ss);
        CHECK(!hasError());
        CHECK(sameBytes(back.getNodeBuffer(), kd.getNodeBuffer()));
        CHECK(sameBytes(back.getTriWoopBuffer(), kd.getTriWoopBuffer()));
        CHECK(sameBytes(back.getTriIndexBuffer(), kd.getTriIndexBuffer()));
        CHECK(std::memcmp(&back.getBBox(), &kd.getBBox(), sizeof(AABB)) == 0);
        CHECK(back.getDelta() == kd.getDelta());
        std::stringstream cut(ss.str().substr(0, 40));
        CudaKDTree truncated(cut);
        CHECK(hasError());
        clearError();
        // the Renderer builds the same tree through getCudaKDTree and picks the kd-tree tracer
        Renderer r(builder);
        r.setScene(&scene);
        Renderer::Params p;
        p.kernelName = "any name selects the kd-tree kernel";
        r.setParams(p);
        CHECK(r.isKDTree());
        CudaKDTree* built = dynamic_cast<CudaKDTree*>(r.getCudaBVH());
        CHECK(built && sameBytes(built->getNodeBuffer(), kd.getNodeBuffer()) && sameBytes(built->getTriIndexBuffer(), kd.getTriIndexBuffer()));
        CudaKDTreeTracer* tr = dynamic_cast<CudaKDTreeTracer*>(&r.getCudaTracer());
        CHECK(tr && tr->getKernelConfig().bvhLayout == BVHLayout_Compact && tr->getKernelConfig().blockWidth == 64 &&
              tr->getKernelConfig().blockHeight == 1 && tr->getKernelConfig().usePersistentThreads == 0);
        bool failed = false;
        try { built->trace(r.getPrimaryRays(), r.getPrimaryRays().getResultBuffer()); } catch (const FatalError&) { failed = true; }
        CHECK(failed);   // no host kd-tree tracer
    }
    Renderer bvh("SAHBVH");
    CHECK(!bvh.isKDTree() && dynamic_cast<CudaBVHTracer*>(&bvh.getCudaTracer()) != NULL);
}

static void dump(const char* dir, const std::string& name, const void* data, size_t bytes)
{
    const std::string path = std::string(dir) + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != NULL);
    if (!f) return;
    std::fwrite(data, 1, bytes, f);
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
    for (const char* builder : {"SAHKDTree", "SAHBVH"}) {
        const std::string b(builder);
        Renderer::Params p;
        p.kernelName = "fermi_speculative_while_while";
        Renderer r(builder);
        r.setScene(&scene);
        r.setParams(p);
        r.beginFrame(cam);
        int batches = 0;
        while (r.nextBatch()) { r.traceBatch(); batches++; }
        CHECK(batches == 1);
        dump(dir, b + "_rays.bin", r.getPrimaryRays().getRayBuffer());
        dump(dir, b + "_results.bin", r.getPrimaryRays().getResultBuffer());
        if (r.isKDTree()) {
            CudaKDTree* kd = dynamic_cast<CudaKDTree*>(r.getCudaBVH());
            CHECK(kd != NULL);
            dump(dir, b + "_nodes.bin", kd->getNodeBuffer());
            dump(dir, b + "_woop.bin", kd->getTriWoopBuffer());
            dump(dir, b + "_index.bin", kd->getTriIndexBuffer());
            dump(dir, b + "_bbox.bin", &kd->getBBox(), sizeof(AABB));
        }
        // an AO frame over the same tree: every batch traces, the ray count follows the primary hits
        Renderer::Params ao = p;
        ao.rayType = Renderer::RayType_AO;
        ao.numSamples = 8;
        ao.aoRadius = 2.0f;
        r.setParams(ao);
        r.beginFrame(cam);
        int aoBatches = 0;
        S64 aoRays = 0, aoHits = 0;
        while (r.nextBatch()) {
            r.traceBatch();
            aoBatches++;
            RayBuffer* rb = r.getBatchRays();
            aoRays += rb->getSize();
            const NtrRayResult* res = (const NtrRayResult*)rb->getResultBuffer().getPtr();
            for (S32 i = 0; i < rb->getSize(); i++) aoHits += res[i].id >= 0;
        }
        // every primary slot gets numSamples AO slots; getTotalNumRays counts those of primary hits only
        CHECK(aoBatches >= 1 && aoRays == (S64)W * H * ao.numSamples && r.getTotalNumRays() <= aoRays && aoHits > 0 && aoHits < aoRays);
        std::printf("%s: AO %lld rays, %lld hits\n", builder, (long long)aoRays, (long long)aoHits);
    }
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
    std::printf("kdtree_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
