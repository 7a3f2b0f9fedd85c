// reorder_host_test.cpp -- the host mirror's renumbering: CudaBVH::reorder and Renderer::reorderBVH.  Without a device (`cpu`): the
// calls that must fail do, with their messages, and the result starts as zero.  On a GPU (`gpu <dir>`), for Renderer("DeviceSAHBVH"),
// ("HLBVH") and ("PersistentBVH") on the mesh and camera tests/test_bvh_reorder_host.py left in <dir> (the Cornell box): frame ->
// reorderBVH -> frame; the second frame's primary records and its AO batches' rays and records equal the first frame's bit for bit
// (the tree is the same, so is the visiting order), and the tree's three buffers are dumped before and after for the numpy spec.
// Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "Renderer.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

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
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(0, 2, 3)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0), Vec3f(1, 1, 0), Vec3f(0, 1, 0)};
    Scene a(2, tris, 4, verts);
    // the kd-tree has no node order to restore; a BVH builder needs a scene; nothing touches a device before these answers
    for (const char* name : {"SAHKDTree", "SpatialMedianKDTree", "PersistentKDTree"}) {
        Renderer kd(name);
        kd.setScene(&a);
        CHECK(failureOf([&] { kd.reorderBVH(); }) == "Renderer::reorderBVH: the kd-tree has no node order to restore");
    }
    for (const char* name : {"SAHBVH", "HLBVH", "PersistentBVH", "DeviceSAHBVH"}) {
        Renderer r(name);
        CHECK(failureOf([&] { r.reorderBVH(); }) == "Renderer: no scene");
    }
    CudaBVH other((BVHLayout)0);
    CHECK(failureOf([&] { other.reorder(); }) == "CudaBVH::reorder: only BVHLayout_Compact is supported");
    CudaBVH plain(BVHLayout_Compact);
    const NtrBvhReorderResult& r = plain.getReorderResult();
    CHECK(r.numNodes == 0 && r.numRows == 0 && r.nodesBytes == 0 && r.seconds == 0.0f);
}

template <class T>
static std::vector<T> readFile(const std::string& path)
{
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    CHECK(f != NULL);
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (bytes) CHECK(std::fread(v.data(), 1, (size_t)bytes, f) == (size_t)bytes);
    std::fclose(f);
    return v;
}

static void dump(const std::string& path, Buffer& b)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != NULL);
    if (!f) return;
    if (b.getSize()) std::fwrite(b.getPtr(), 1, (size_t)b.getSize(), f);
    std::fclose(f);
}

struct Frames {
    std::string primary, ao;   // result records of the primary batch; rays and records of every AO batch in order
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
    ao.aoRadius = 150.0f;
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

static void gpuBuilder(const std::string& dir, const std::string& builder, Scene& scene, const CameraView& cam)
{
    Renderer r(builder);
    r.setScene(&scene);
    const Frames before = renderFrames(r, cam);
    CudaBVH* tree = dynamic_cast<CudaBVH*>(r.getCudaBVH());
    CHECK(tree != NULL);
    if (!tree) return;
    dump(dir + "/" + builder + "_nodes0.bin", tree->getNodeBuffer());
    dump(dir + "/" + builder + "_woop0.bin", tree->getTriWoopBuffer());
    dump(dir + "/" + builder + "_index0.bin", tree->getTriIndexBuffer());
    const U32 flags0 = tree->getTraceFlags();
    const S64 slots0 = tree->getNodeBuffer().getSize() / 64;

    r.reorderBVH();
    CHECK(dynamic_cast<CudaBVH*>(r.getCudaBVH()) == tree);                    // the same tree object with new buffers
    const NtrBvhReorderResult ro = tree->getReorderResult();
    CHECK(ro.numNodes > 0 && ro.numLeaves > 0 && ro.numRows > 0 && ro.seconds > 0.0f && ro.numNodes + ro.numDroppedSlots == slots0);
    CHECK(tree->getNodeBuffer().getSize() == ro.nodesBytes && tree->getTriWoopBuffer().getSize() == ro.triWoopBytes &&
          tree->getTriIndexBuffer().getSize() == ro.triIndexBytes);            // trimmed to the result's extents
    CHECK(tree->getTraceFlags() == flags0);                                    // revalidated on the new buffer
    const Frames after = renderFrames(r, cam);
    CHECK(before.primaryHits > 0 && after.primary == before.primary);
    CHECK(after.aoRays == before.aoRays && after.aoHits == before.aoHits && after.aoHits > 0 && after.ao == before.ao);
    dump(dir + "/" + builder + "_nodes1.bin", tree->getNodeBuffer());
    dump(dir + "/" + builder + "_woop1.bin", tree->getTriWoopBuffer());
    dump(dir + "/" + builder + "_index1.bin", tree->getTriIndexBuffer());
    std::printf("%s: %d nodes (%d slots dropped), %d leaves, %d rows, reorder %.1f us; primary %lld hits, AO %lld rays %lld hits\n",
                builder.c_str(), ro.numNodes, ro.numDroppedSlots, ro.numLeaves, ro.numRows, ro.seconds * 1e6f, (long long)after.primaryHits,
                (long long)after.aoRays, (long long)after.aoHits);
}

static void gpuTests(const std::string& dir)
{
    const std::vector<Vec3i> tris = readFile<Vec3i>(dir + "/tri.bin");
    const std::vector<Vec3f> verts = readFile<Vec3f>(dir + "/pos.bin");
    const std::vector<float> c = readFile<float>(dir + "/cam.bin");           // eye[3], nscreenToWorld[16] row-major, far, width, height
    CHECK(!tris.empty() && !verts.empty() && c.size() == 22);
    if (g_failed) return;
    CameraView cam;
    cam.position = Vec3f(c[0], c[1], c[2]);
    std::memcpy(cam.nscreenToWorld.m, &c[3], 16 * sizeof(float));
    cam.cameraFar = c[19];
    cam.width = (int)c[20];
    cam.height = (int)c[21];
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    for (const char* builder : {"DeviceSAHBVH", "HLBVH", "PersistentBVH"}) gpuBuilder(dir, builder, scene, cam);
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
    std::printf("reorder_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
