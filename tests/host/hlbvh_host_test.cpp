// hlbvh_host_test.cpp -- the host mirror's HLBVH path: HLBVHBuilder with hlbvh = true, Renderer::setHLBVHParams, and the BVH cache
// names of the two builders.  `hlbvh_host_test cpu` needs no GPU (cache names); `hlbvh_host_test gpu` builds and renders.
// Compiled with plain g++ against libntrace_amd.so (tests/test_hlbvh_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "HLBVHBuilder.hpp"
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

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 4);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Renderer::Params p;
    p.kernelName = "fermi_speculative_while_while";
    Renderer lbvh("HLBVH"), hl("HLBVH"), hl6("HLBVH");
    for (Renderer* r : {&lbvh, &hl, &hl6}) { r->setScene(&scene); r->setParams(p); r->setCachePath("/tmp"); }
    const String def = lbvh.getCacheFileName();
    HLBVHParams hp;
    CHECK(!hp.hlbvh && !lbvh.getHLBVHParams().hlbvh);
    lbvh.setHLBVHParams(hp);                 // the default parameters, set explicitly: the name stays
    CHECK(lbvh.getCacheFileName() == def);
    hp.hlbvh = true;
    hp.hlbvhBits = 4;
    hl.setHLBVHParams(hp);
    CHECK(hl.getCacheFileName() != def && hl.getCacheFileName().find("_HLBVH.dat") != String::npos);
    hp.hlbvhBits = 6;
    hl6.setHLBVHParams(hp);
    CHECK(hl6.getCacheFileName() != def && hl6.getCacheFileName() != hl.getCacheFileName());
    std::printf("default cache name: %s\n", def.c_str() + 5);
}

static void dump(const char* dir, const std::string& name, Buffer& b)
{
    const std::string path = std::string(dir) + "/" + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != NULL);
    if (!f) return;
    std::fwrite(b.getPtr(), 1, (size_t)b.getSize(), f);
    std::fclose(f);
}

static void gpuTests(const char* dir)
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 24);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    HLBVHParams hp;
    hp.hlbvh = true;
    hp.hlbvhBits = 4;
    HLBVHBuilder hb(&scene, Platform("GPU"), hp);
    const NtrHlbvhResult& hr = hb.getHlbvhResult();
    CHECK(hr.numClusters > 1 && hr.topNodes == hr.numClusters - 1 && hr.topLevels > 0);
    CHECK(hb.getNodeBuffer().getSize() == hb.getBuildResult().nodesBytes && hb.getBuildResult().numLeaves == hb.getBuildResult().numNodes + 1);
    CHECK(hb.getTriWoopBuffer().getSize() == (3 * (S64)tris.size() + hb.getBuildResult().numLeaves) * 16);
    HLBVHBuilder lb(&scene, Platform("GPU"), HLBVHParams());
    CHECK(lb.getHlbvhResult().numClusters == 0);

    const int W = 320, H = 200;
    const CameraView cam = makeCamera(W, H);
    for (const char* kernel : {"fermi_speculative_while_while", "kepler_dynamic_fetch"}) {
        Renderer::Params p;
        p.kernelName = kernel;
        Renderer hl("HLBVH");
        hl.setScene(&scene);
        hl.setParams(p);
        hl.setHLBVHParams(hp);
        hl.beginFrame(cam);
        int batches = 0;
        while (hl.nextBatch()) { hl.traceBatch(); batches++; }
        CHECK(batches == 1);
        CudaAS* as = hl.getCudaBVH();
        const HLBVHBuilder* built = dynamic_cast<const HLBVHBuilder*>(as);
        CHECK(built && built->getHlbvhResult().numClusters == hr.numClusters);
        const std::string k(kernel);
        dump(dir, k + "_nodes.bin", as->getNodeBuffer());
        dump(dir, k + "_woop.bin", as->getTriWoopBuffer());
        dump(dir, k + "_index.bin", as->getTriIndexBuffer());
        dump(dir, k + "_rays.bin", hl.getPrimaryRays().getRayBuffer());
        dump(dir, k + "_results.bin", hl.getPrimaryRays().getResultBuffer());
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
    std::printf("hlbvh_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
