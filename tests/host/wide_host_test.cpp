// wide_host_test.cpp -- the host mirror's 4-wide tree (CudaWideBVH): it shares its CudaBVH's Woop and index buffers, owns only the wide
// node buffer and refuses to build without a device (`cpu`); on a GPU (`gpu <dir>`) it widens a host SAH tree with leaves of several
// triangles and traces closest-hit and any-hit batches, whose buffers and records are dumped for tests/test_bvh_wide_host.py.
// Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaWideBVH.hpp"
#include "bvh/Platform.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

// a box room with a block inside, nTess^2 * 2 triangles per face
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
    box(Vec3f(-1.5f, -1.25f, -1.75f), Vec3f(1.25f, 1.5f, 1.125f));
    box(Vec3f(-0.5f, -1.25f, 0.25f), Vec3f(0.5f, -0.25f, 0.75f));
}

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 2);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH cbvh(bvh, BVHLayout_Compact);

    CudaWideBVH wide(cbvh);
    // the Woop rows and the index are the binary tree's own buffers, not copies; only the wide node buffer is this object's
    CHECK(&wide.getTriWoopBuffer() == &cbvh.getTriWoopBuffer() && &wide.getTriIndexBuffer() == &cbvh.getTriIndexBuffer());
    CHECK(&wide.getBVH() == &cbvh && &wide.getWideNodeBuffer() != &cbvh.getNodeBuffer());
    CHECK(!wide.isBuilt() && wide.getWideNodeBuffer().getSize() == 0 && wide.getWidenResult().numNodes == 0);
    int64_t cap = 0;
    CHECK(ntr_bvh_widen_capacity(cbvh.getNodeBuffer().getSize(), &cap) == NTR_OK && cap == 2 * cbvh.getNodeBuffer().getSize());
    bool threw = false;
    RayBuffer rays(64, true);
    try { wide.traceBatch(rays); } catch (const FatalError&) { threw = true; }   // no wide tree yet
    CHECK(threw);
    RayBuffer none(0, true);
    CHECK(wide.traceBatch(none) == 0.0f);
    CudaBVH other((BVHLayout)0);
    threw = false;
    try { CudaWideBVH bad(other); bad.build(); } catch (const FatalError&) { threw = true; }
    CHECK(threw);
    // valid arguments and no device: the build is refused
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        threw = false;
        try { wide.build(); } catch (const FatalError& e) { threw = true; std::printf("no device: build refused (%s)\n", e.message.c_str()); }
        CHECK(threw && !wide.isBuilt());
        int64_t held = -1;
        CHECK(ntr_bvh_widen_scratch_bytes(&held) == NTR_OK && held == 0);
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
    makeScene(tris, verts, 6);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH cbvh(bvh, BVHLayout_Compact);   // leaves of several triangles

    CudaWideBVH wide(cbvh);
    wide.build();
    const NtrBvhWideResult& res = wide.getWidenResult();
    CHECK(wide.isBuilt() && res.numNodes >= 1 && res.nodesBytes == 128 * (int64_t)res.numNodes && wide.getWideNodeBuffer().getSize() == res.nodesBytes);
    CHECK(res.counts[0] + res.counts[1] + res.counts[2] == res.numNodes && res.height >= 1 && res.stackBound <= 104 && res.seconds > 0.0f);
    std::printf("wide: %d nodes (%d %d %d), %d leaf links, height %d, stackBound %d, %.3f ms\n", res.numNodes, res.counts[0], res.counts[1],
                res.counts[2], res.numLeafLinks, res.height, res.stackBound, res.seconds * 1e3f);
    dump(dir, "nodes.bin", cbvh.getNodeBuffer());
    dump(dir, "woop.bin", cbvh.getTriWoopBuffer());
    dump(dir, "index.bin", cbvh.getTriIndexBuffer());
    dump(dir, "wide.bin", wide.getWideNodeBuffer());

    const int W = 96, H = 64;
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        RayBuffer rays(W * H, anyHit == 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                Ray r;
                r.origin = Vec3f(0.3f, 0.7f, -6.0f);
                r.direction = Vec3f(((x + 0.5f) / W - 0.5f) * 0.9f, ((y + 0.5f) / H - 0.5f) * 0.9f, 1.0f);
                r.tmin = 0.0f;
                r.tmax = anyHit ? 5.5f : 100.0f;
                rays.setRay(y * W + x, r);
            }
        const F32 sec = wide.traceBatch(rays);
        CHECK(sec > 0.0f);
        S64 hits = 0;
        for (int i = 0; i < W * H; i++) hits += rays.getResultForSlot(i).id >= 0;
        CHECK(hits > W * H / 8 && hits < W * H);
        const std::string kind = anyHit ? "any" : "closest";
        dump(dir, kind + "_rays.bin", rays.getRayBuffer());
        dump(dir, kind + "_results.bin", rays.getResultBuffer());
        std::printf("wide %s hit: %d rays, %lld hits, %.3f ms\n", kind.c_str(), W * H, (long long)hits, sec * 1e3f);
    }
    uint32_t bits = 1;
    CHECK(ntr_trace_status(NULL, &bits) == NTR_OK && bits == 0);
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
    std::printf("wide_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
