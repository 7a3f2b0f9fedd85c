// optimize_host_test.cpp -- the host mirror's treelet optimiser and SAH cost: CudaBVH::optimize / calcSAHCost,
// HLBVHBuilder::calcSAHGPU and Renderer::optimizeBVH.  Without a device (`cpu`): the calls that must fail do, with their messages, and
// the results start as zero.  On a GPU (`gpu <dir>`), for Renderer("SAHBVH"), ("HLBVH") and ("PersistentBVH"): frame -> optimizeBVH ->
// frame; the second frame's primary records and its AO batches' records equal those of a second Renderer that adopted a copy of the
// first tree optimised through ntr_bvh_optimize directly, the trees are equal byte for byte, and calcSAHCost / calcSAHGPU equal
// ntr_bvh_sah_cost.  Trees are dumped for tests/test_bvh_optimize_host.py.  Compiled with plain g++ against libntrace_amd.so.
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

// a closed room with two blocks inside, nTess^2 * 2 triangles per face
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
    c.position = Vec3f(0.3f, 0.7f, -8.0f);
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

static bool sameFloat(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }

template <class Fn>
static std::string failureOf(Fn fn)
{
    try {
        fn();
    } catch (const FatalError& e) {
        return e.message;
    }
    return "";
}

static void cpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 6);
    Scene a((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    // the kd-tree has no optimiser; a BVH builder needs a scene; nothing touches a device before these answers
    for (const char* name : {"SAHKDTree", "SpatialMedianKDTree", "PersistentKDTree"}) {
        Renderer kd(name);
        kd.setScene(&a);
        CHECK(failureOf([&] { kd.optimizeBVH(); }) == "Renderer::optimizeBVH: the kd-tree has no treelet optimiser");
    }
    for (const char* name : {"SAHBVH", "HLBVH", "PersistentBVH"}) {
        Renderer r(name);
        CHECK(failureOf([&] { r.optimizeBVH(1); }) == "Renderer: no scene");
    }
    CudaBVH plain(BVHLayout_Compact);
    CHECK(plain.getOptimizeResult().passes == 0 && plain.getOptimizeResult().seconds == 0.0f && plain.getSAHResult().numNodes == 0);
    CHECK(CudaBVH::DefaultOptimizePasses >= 1 && CudaBVH::DefaultOptimizePasses <= 8);
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

struct Frames {
    std::string primary, ao;   // result records: the primary batch; every AO batch in order
    S64 primaryHits = 0, aoRays = 0, aoHits = 0;
};

static Frames renderFrames(Renderer& r, const CameraView& cam)
{
    Frames f;
    Renderer::Params p;
    p.kernelName = "fermi_speculative_while_while";
    r.setParams(p);
    r.beginFrame(cam);
    while (r.nextBatch()) {
        r.traceBatch();
        RayBuffer& rb = r.getPrimaryRays();
        f.primary.assign((const char*)rb.getResultBuffer().getPtr(), (size_t)rb.getSize() * sizeof(NtrRayResult));
        const NtrRayResult* rr = (const NtrRayResult*)rb.getResultBuffer().getPtr();
        for (S32 i = 0; i < rb.getSize(); i++) f.primaryHits += rr[i].id >= 0;
    }
    Renderer::Params ao = p;
    ao.rayType = Renderer::RayType_AO;
    ao.numSamples = 8;
    ao.aoRadius = 2.0f;
    r.setParams(ao);
    r.beginFrame(cam);
    while (r.nextBatch()) {
        r.traceBatch();
        RayBuffer* rb = r.getBatchRays();
        f.ao.append((const char*)rb->getRayBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRay));
        f.ao.append((const char*)rb->getResultBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRayResult));
        const NtrRayResult* rr = (const NtrRayResult*)rb->getResultBuffer().getPtr();
        for (S32 i = 0; i < rb->getSize(); i++) f.aoHits += rr[i].id >= 0;
        f.aoRays += rb->getSize();
    }
    return f;
}

static void gpuBuilder(const char* dir, const std::string& builder, const std::vector<Vec3i>& tris, const std::vector<Vec3f>& verts)
{
    const int W = 320, H = 200, passes = 2;
    const CameraView cam = makeCamera(W, H);
    Scene sceneA((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Renderer rA(builder);
    rA.setScene(&sceneA);
    const Frames before = renderFrames(rA, cam);
    CudaBVH* treeA = dynamic_cast<CudaBVH*>(rA.getCudaBVH());
    CHECK(treeA != NULL);
    if (!treeA) return;
    std::stringstream built;
    treeA->serialize(built);
    dump(dir, builder + "_nodes0.bin", treeA->getNodeBuffer());
    dump(dir, builder + "_woop.bin", treeA->getTriWoopBuffer());
    const F32 sah0 = treeA->calcSAHCost();
    const NtrBvhSahResult s0 = treeA->getSAHResult();
    CHECK(s0.numTris == (int32_t)tris.size() && s0.numLeaves == s0.numNodes + 1 && s0.height > 0 && s0.seconds > 0.0f);
    if (HLBVHBuilder* hb = dynamic_cast<HLBVHBuilder*>(treeA)) CHECK(sameFloat(hb->calcSAHGPU(), sah0));   // the reference's name

    rA.optimizeBVH(passes);
    CHECK(dynamic_cast<CudaBVH*>(rA.getCudaBVH()) == treeA);                 // the same tree object, restructured in place
    const NtrBvhOptimizeResult ro = treeA->getOptimizeResult();
    CHECK(ro.passes == passes && ro.numNodes == s0.numNodes && ro.heightBefore[0] == s0.height && ro.seconds > 0.0f);
    CHECK(ro.formed[0] > 0 && ro.rewritten[0] > 0 && ro.rewritten[0] <= ro.formed[0]);
    const F32 sah1 = treeA->calcSAHCost();
    CHECK(sah1 < sah0 && treeA->getSAHResult().height == ro.heightAfter[passes - 1] && treeA->getSAHResult().numTris == s0.numTris);
    const Frames after = renderFrames(rA, cam);
    CHECK(after.primary == before.primary);                                  // closest hits do not depend on the topology
    CHECK(after.aoRays == before.aoRays && after.aoHits == before.aoHits && after.aoHits > 0);
    dump(dir, builder + "_nodes1.bin", treeA->getNodeBuffer());

    // the second Renderer: a copy of the tree as it was built, optimised through the C-ABI
    CudaBVH* treeB = new CudaBVH(built);
    CHECK(!hasError());
    NtrBvhOptimizeResult res;
    CHECK(ntr_bvh_optimize(treeB->getNodeBuffer().getMutableCudaPtr(), treeB->getNodeBuffer().getSize(), passes, &res, NULL) == NTR_OK);
    treeB->invalidateTraceFlags();
    CHECK(sameBytes(treeB->getNodeBuffer(), treeA->getNodeBuffer()) && sameBytes(treeB->getTriWoopBuffer(), treeA->getTriWoopBuffer()) &&
          sameBytes(treeB->getTriIndexBuffer(), treeA->getTriIndexBuffer()));
    CHECK(std::memcmp(res.rewritten, ro.rewritten, sizeof(res.rewritten)) == 0 && std::memcmp(res.heightAfter, ro.heightAfter, sizeof(res.heightAfter)) == 0);
    NtrBvhSahResult sr;
    CHECK(ntr_bvh_sah_cost(treeB->getNodeBuffer().getCudaPtr(), treeB->getNodeBuffer().getSize(), treeB->getTriWoopBuffer().getCudaPtr(),
                           treeB->getTriWoopBuffer().getSize(), &sr, NULL) == NTR_OK);
    CHECK(sameFloat(sr.sahCost, sah1) && sr.numNodes == s0.numNodes);
    Renderer rB(builder);
    rB.setScene(&sceneA);
    rB.adoptCudaBVH(treeB);
    const Frames direct = renderFrames(rB, cam);
    CHECK(direct.primary == after.primary);
    CHECK(direct.ao == after.ao);
    std::printf("%s: %d nodes, SAH %.4f -> %.4f in %d passes (%d + %d of %d treelets rewritten, height %d -> %d), %.1f us; AO %lld rays %lld hits\n",
                builder.c_str(), ro.numNodes, sah0, sah1, passes, ro.rewritten[0], ro.rewritten[1], ro.formed[0], ro.heightBefore[0],
                ro.heightAfter[passes - 1], ro.seconds * 1e6f, (long long)after.aoRays, (long long)after.aoHits);
    std::FILE* f = std::fopen((std::string(dir) + "/" + builder + "_sah.txt").c_str(), "w");
    if (f) { std::fprintf(f, "%.9g %.9g\n", sah0, sah1); std::fclose(f); }
}

static void gpuTests(const char* dir)
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 24);
    for (const char* builder : {"SAHBVH", "HLBVH", "PersistentBVH"}) gpuBuilder(dir, builder, tris, verts);
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
    std::printf("optimize_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
