// bvh_motion_host_test.cpp -- the host mirror's deformation motion blur: CudaBVH::refitMotion / hasMotion and CudaBVHTracer::setTime /
// setRayTimes.  Without a device (`cpu`): the calls that must fail do, by name, before anything touches a device.  On a GPU
// (`gpu <dir>`): the tree, the mesh's two keys and the rays that tests/test_bvh_motion_host.py wrote into <dir> are loaded, the tree is
// refitted to the two keys and traced at time 0.5 and at per-ray times, a later refit() drops the motion state, and the records and
// buffers are dumped for the Python side, which compares them with the spec (tests/np_bvh_motion.py).  Plain g++ against
// libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaBVHTracer.hpp"
#include "CudaKDTree.hpp"
#include "RayBuffer.hpp"
#include "Scene.hpp"

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

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static void cpuTests()
{
    const Vec3i tri(0, 1, 2);
    const Vec3f verts[3] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0), Vec3f(0, 1, 0)};
    Scene scene(1, &tri, 3, verts);
    CudaBVH plain(BVHLayout_Compact);
    CHECK(!plain.hasMotion() && plain.getMotionNodeBuffer().getSize() == 0 && plain.getVertRowsBuffer(0).getSize() == 0);
    CHECK(has(failureOf([&] { plain.refitMotion(scene, NULL, 0.0f); }), "CudaBVH::refitMotion: no key-1 positions"));
    CudaBVH aos(BVHLayout_AOS_AOS);
    CHECK(has(failureOf([&] { aos.refitMotion(scene, verts, 0.0f); }), "CudaBVH::refitMotion: only BVHLayout_Compact"));
    CHECK(!plain.hasMotion() && !aos.hasMotion());

    // ray times over something that is not a Compact CudaBVH: refused by name
    CudaKDTree kd;
    CudaBVHTracer tracer;
    tracer.setKernel("fermi_speculative_while_while");
    tracer.setBVH(&kd);
    RayBuffer rays(1);
    Buffer times(NULL, 4);
    tracer.setTime(0.5f);
    CHECK(has(failureOf([&] { tracer.traceBatch(rays); }), "a kd-tree or a wide tree has no deformation motion blur"));
    tracer.clearTime();
    tracer.setRayTimes(&times);
    CHECK(has(failureOf([&] { tracer.traceBatch(rays); }), "a kd-tree or a wide tree has no deformation motion blur"));
}

static std::vector<char> slurp(const std::string& path)
{
    std::vector<char> out;
    FILE* f = std::fopen(path.c_str(), "rb");
    CHECK(f != NULL);
    if (!f) return out;
    std::fseek(f, 0, SEEK_END);
    out.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (!out.empty()) CHECK(std::fread(out.data(), 1, out.size(), f) == out.size());
    std::fclose(f);
    return out;
}

static void dump(const std::string& dir, const char* name, Buffer& b)
{
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    CHECK(f != NULL);
    if (!f) return;
    if (b.getSize()) std::fwrite(b.getPtr(), 1, (size_t)b.getSize(), f);
    std::fclose(f);
}

static void gpuTests(const std::string& dir)
{
    const std::vector<char> tris = slurp(dir + "/tris.bin"), pos0 = slurp(dir + "/pos0.bin"), pos1 = slurp(dir + "/pos1.bin");
    const std::vector<char> nodes = slurp(dir + "/nodes.bin"), woop = slurp(dir + "/woop.bin"), index = slurp(dir + "/index.bin");
    const std::vector<char> rayBytes = slurp(dir + "/rays.bin"), timeBytes = slurp(dir + "/times.bin");
    const S32 numTris = (S32)(tris.size() / sizeof(Vec3i)), numVerts = (S32)(pos0.size() / sizeof(Vec3f)), numRays = (S32)(rayBytes.size() / sizeof(Ray));
    CHECK(numTris > 0 && numVerts > 0 && numRays > 0 && pos1.size() == pos0.size() && timeBytes.size() == (size_t)numRays * 4);
    if (g_failed) return;

    Scene scene(numTris, (const Vec3i*)tris.data(), numVerts, (const Vec3f*)pos0.data());
    CudaBVH bvh(BVHLayout_Compact);
    bvh.getNodeBuffer().set(nodes.data(), (S64)nodes.size());
    bvh.getTriWoopBuffer().set(woop.data(), (S64)woop.size());
    bvh.getTriIndexBuffer().set(index.data(), (S64)index.size());

    RayBuffer rays(numRays);
    for (S32 i = 0; i < numRays; i++) rays.setRay(i, ((const Ray*)rayBytes.data())[i]);
    CudaBVHTracer tracer;
    tracer.setKernel("fermi_speculative_while_while");
    tracer.setBVH(&bvh);

    // a time on a tree without motion: the static launch, as ever
    tracer.setTime(0.5f);
    tracer.traceBatch(rays);
    dump(dir, "static_before.bin", rays.getResultBuffer());

    bvh.refitMotion(scene, (const Vec3f*)pos1.data(), 0.0f);
    CHECK(bvh.hasMotion() && bvh.getMotionNodeBuffer().getSize() == bvh.getNodeBuffer().getSize() &&
          bvh.getVertRowsBuffer(0).getSize() == bvh.getTriWoopBuffer().getSize() && bvh.getVertRowsBuffer(1).getSize() == bvh.getTriWoopBuffer().getSize());
    CHECK(bvh.getRefitResult().numNodes > 0 && bvh.getRefitResult().seconds > 0.0f);
    dump(dir, "nodes0.bin", bvh.getNodeBuffer());
    dump(dir, "nodes1.bin", bvh.getMotionNodeBuffer());
    dump(dir, "woop0.bin", bvh.getTriWoopBuffer());
    dump(dir, "vrows0.bin", bvh.getVertRowsBuffer(0));
    dump(dir, "vrows1.bin", bvh.getVertRowsBuffer(1));

    const F32 sec = tracer.traceBatch(rays);
    CHECK(sec > 0.0f);
    dump(dir, "half.bin", rays.getResultBuffer());

    Buffer times(timeBytes.data(), (S64)timeBytes.size());
    tracer.clearTime();
    tracer.setRayTimes(&times);
    tracer.traceBatch(rays);
    dump(dir, "per_ray.bin", rays.getResultBuffer());
    Buffer tooFew(NULL, (S64)timeBytes.size() - 4);
    tracer.setRayTimes(&tooFew);
    CHECK(has(failureOf([&] { tracer.traceBatch(rays); }), "fewer than one float per ray"));
    tracer.setRayTimes(&times);

    // neither set: the static launch over key 0
    tracer.setRayTimes(NULL);
    tracer.traceBatch(rays);
    dump(dir, "key0.bin", rays.getResultBuffer());

    // a later refit drops the motion state: the times are ignored again
    bvh.refit(scene, 0.0f);
    CHECK(!bvh.hasMotion() && bvh.getMotionNodeBuffer().getSize() == 0 && bvh.getVertRowsBuffer(1).getSize() == 0);
    tracer.setTime(0.5f);
    tracer.traceBatch(rays);
    dump(dir, "static_after.bin", rays.getResultBuffer());
    std::printf("%d tris, %d nodes, %d rays, motion trace %.1f us\n", (int)numTris, (int)bvh.getRefitResult().numNodes, (int)numRays, sec * 1e6f);
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
    std::printf("bvh_motion_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
