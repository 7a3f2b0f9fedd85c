// refit_host_test.cpp -- the host mirror's refit path: Scene::setVertexPositions, CudaBVH::refit and Renderer::refit.  Without a
// device (`cpu`): setVertexPositions gives the normals and the box of a Scene constructed from the moved mesh, and the calls that
// must fail do, with their messages.  On a GPU (`gpu <dir>`), for Renderer("SAHBVH"), ("HLBVH") and ("PersistentBVH"): frame ->
// setVertexPositions -> refit -> frame; the second frame's primary records and its AO batches' records equal those of a second
// Renderer that was given a Scene made from the moved mesh and a copy of the first tree refitted through ntr_bvh_refit directly.
// Trees and meshes are dumped for tests/test_bvh_refit_host.py.  Compiled with plain g++ against libntrace_amd.so.
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

// pos + a * d * sin(k * pos.yzx + phase), d the scene diagonal
static std::vector<Vec3f> deform(const std::vector<Vec3f>& v, float a)
{
    Vec3f lo = v[0], hi = v[0];
    for (const Vec3f& p : v) {
        lo = Vec3f(std::fmin(lo.x, p.x), std::fmin(lo.y, p.y), std::fmin(lo.z, p.z));
        hi = Vec3f(std::fmax(hi.x, p.x), std::fmax(hi.y, p.y), std::fmax(hi.z, p.z));
    }
    const Vec3f e = hi - lo;
    const float d = std::sqrt(e.x * e.x + e.y * e.y + e.z * e.z), k = 9.0f / d, s = a * d;
    std::vector<Vec3f> out(v.size());
    for (size_t i = 0; i < v.size(); i++)
        out[i] = Vec3f(v[i].x + s * std::sin(k * v[i].y + 0.3f), v[i].y + s * std::sin(k * v[i].z + 1.1f), v[i].z + s * std::sin(k * v[i].x + 2.3f));
    return out;
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
    const std::vector<Vec3f> moved = deform(verts, 0.02f);
    Scene a((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    Scene b((S32)tris.size(), tris.data(), (S32)moved.size(), moved.data());
    Vec3f lo0, hi0, lo1, hi1;
    a.getBBox(lo0, hi0);
    CHECK(!sameBytes(a.getTriNormalBuffer(), b.getTriNormalBuffer()));
    a.setVertexPositions(moved.data());
    a.getBBox(lo1, hi1);
    b.getBBox(lo0, hi0);
    CHECK(std::memcmp(&lo0, &lo1, sizeof(lo0)) == 0 && std::memcmp(&hi0, &hi1, sizeof(hi0)) == 0);
    CHECK(sameBytes(a.getVtxPosBuffer(), b.getVtxPosBuffer()));
    CHECK(sameBytes(a.getTriNormalBuffer(), b.getTriNormalBuffer()));
    CHECK(sameBytes(a.getTriVtxIndexBuffer(), b.getTriVtxIndexBuffer()));
    CHECK(a.hash() == b.hash());
    CHECK(failureOf([&] { a.setVertexPositions(NULL); }).find("null positions") != std::string::npos);

    // the kd-tree has no refit; a BVH builder needs a scene; nothing touches a device before these answers
    for (const char* name : {"SAHKDTree", "SpatialMedianKDTree", "PersistentKDTree"}) {
        Renderer kd(name);
        kd.setScene(&a);
        CHECK(failureOf([&] { kd.refit(); }) == "Renderer::refit: the kd-tree has no refit");
    }
    for (const char* name : {"SAHBVH", "HLBVH", "PersistentBVH"}) {
        Renderer r(name);
        CHECK(failureOf([&] { r.refit(); }) == "Renderer: no scene");
    }
    // the default leaf epsilon of a refit: the exact union, except for the builder that grew its leaves
    CudaBVH plain(BVHLayout_Compact);
    CHECK(plain.getRefitEpsilon() == 0.0f && plain.getRefitResult().numNodes == 0);
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
        f.ao.append((const char*)rb->getRayBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRay));   // the rays carry the normals
        f.ao.append((const char*)rb->getResultBuffer().getPtr(), (size_t)rb->getSize() * sizeof(NtrRayResult));
        const NtrRayResult* rr = (const NtrRayResult*)rb->getResultBuffer().getPtr();
        for (S32 i = 0; i < rb->getSize(); i++) f.aoHits += rr[i].id >= 0;
        f.aoRays += rb->getSize();
    }
    return f;
}

static void gpuBuilder(const char* dir, const std::string& builder, const std::vector<Vec3i>& tris, const std::vector<Vec3f>& verts,
                       const std::vector<Vec3f>& moved)
{
    const int W = 320, H = 200;
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
    dump(dir, builder + "_woop0.bin", treeA->getTriWoopBuffer());
    dump(dir, builder + "_index.bin", treeA->getTriIndexBuffer());
    const F32 eps = treeA->getRefitEpsilon();
    CHECK(eps == (builder == "HLBVH" ? 0.001f : 0.0f));

    sceneA.setVertexPositions(moved.data());
    rA.refit();
    CHECK(dynamic_cast<CudaBVH*>(rA.getCudaBVH()) == treeA);                 // the same tree object, refitted in place
    CHECK(treeA->getRefitResult().numNodes == (int32_t)(treeA->getNodeBuffer().getSize() / 64) || builder == "HLBVH");
    CHECK(treeA->getRefitResult().numRows > 3 * (int32_t)tris.size() && treeA->getRefitResult().seconds > 0.0f);
    const Frames after = renderFrames(rA, cam);
    CHECK(after.primary != before.primary && after.primaryHits > 0);
    CHECK(after.aoRays == after.primaryHits * 8 && after.aoHits > 0 && after.aoHits < after.aoRays);
    dump(dir, builder + "_nodes1.bin", treeA->getNodeBuffer());
    dump(dir, builder + "_woop1.bin", treeA->getTriWoopBuffer());

    // the second Renderer: a Scene made from the moved mesh, a copy of the tree as it was built, refitted through the C-ABI
    Scene sceneB((S32)tris.size(), tris.data(), (S32)moved.size(), moved.data());
    CudaBVH* treeB = new CudaBVH(built);
    CHECK(!hasError());
    NtrBvhRefitResult res;
    const int rc = ntr_bvh_refit(treeB->getNodeBuffer().getMutableCudaPtr(), treeB->getNodeBuffer().getSize(),
                                 treeB->getTriWoopBuffer().getMutableCudaPtr(), treeB->getTriWoopBuffer().getSize(),
                                 (const int32_t*)treeB->getTriIndexBuffer().getCudaPtr(), treeB->getTriIndexBuffer().getSize(), (int32_t)tris.size(),
                                 (const int32_t*)sceneB.getTriVtxIndexBuffer().getCudaPtr(), (int32_t)moved.size(),
                                 (const float*)sceneB.getVtxPosBuffer().getCudaPtr(), eps, NULL, &res, NULL);
    CHECK(rc == NTR_OK);
    treeB->invalidateTraceFlags();
    CHECK(sameBytes(treeB->getNodeBuffer(), treeA->getNodeBuffer()) && sameBytes(treeB->getTriWoopBuffer(), treeA->getTriWoopBuffer()) &&
          sameBytes(treeB->getTriIndexBuffer(), treeA->getTriIndexBuffer()));
    CHECK(sameBytes(sceneA.getTriNormalBuffer(), sceneB.getTriNormalBuffer()));
    Renderer rB(builder);
    rB.setScene(&sceneB);
    rB.adoptCudaBVH(treeB);
    const Frames direct = renderFrames(rB, cam);
    CHECK(direct.primary == after.primary);
    CHECK(direct.ao == after.ao);
    std::printf("%s: %d nodes, refit %.1f us; primary hits %lld -> %lld, AO %lld rays %lld hits\n", builder.c_str(), res.numNodes,
                res.seconds * 1e6f, (long long)before.primaryHits, (long long)after.primaryHits, (long long)after.aoRays, (long long)after.aoHits);
}

static void gpuTests(const char* dir)
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 24);
    const std::vector<Vec3f> moved = deform(verts, 0.02f);
    dump(dir, "tris.bin", tris.data(), tris.size() * sizeof(Vec3i));
    dump(dir, "verts.bin", moved.data(), moved.size() * sizeof(Vec3f));
    for (const char* builder : {"SAHBVH", "HLBVH", "PersistentBVH"}) gpuBuilder(dir, builder, tris, verts, moved);
    Renderer kd("SAHKDTree");
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    kd.setScene(&scene);
    CHECK(failureOf([&] { kd.refit(); }) == "Renderer::refit: the kd-tree has no refit");
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
    std::printf("refit_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
