// instanced_seeded_host_test.cpp -- the host mirror's static world (CudaInstancedBVH::setWorld / clearWorld, InstancedRenderer over it;
// DESIGN.md 6u).  `cpu`: setWorld refuses a BLAS index outside the pool, the world's NtrInstance is appended behind the instances' and
// follows setInstances, clearWorld takes it away, and traceBatch still needs a TLAS.  `gpu <dir>`: the scene of the seeded trace's
// tests, which the test driver writes into <dir> (a static world, one BLAS of the pool, and 32 small instances); traceBatch with a world
// equals the C-ABI sequence ntr_trace_bvh + ntr_trace_instanced_seeded / ntr_trace_instanced_wide_seeded byte for byte, for closest hit
// and any hit, with and without masks; a primary and an AO frame of InstancedRenderer equal the same frames rendered with the world as
// an ordinary identity instance: instance ids, resolved ids and t of every primary ray, every word where the hit lies in a real
// instance, hit or miss of every AO ray, and every pixel.  Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"
#include "bvh/Platform.hpp"

using namespace FW;

static int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

template <class Call>
static bool refused(Call call, const char* word)
{
    try { call(); } catch (const FatalError& e) {
        if (std::strstr(e.message.c_str(), word)) return true;
        std::printf("refused with another message: %s\n", e.message.c_str());
    }
    return false;
}

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

static bool isWorldRecord(const NtrInstance& w, S32 blas)
{
    NtrInstance e;
    std::memset(&e, 0, sizeof(e));
    e.objectToWorld[0] = e.objectToWorld[5] = e.objectToWorld[10] = 1.0f;
    e.worldToObject[0] = e.worldToObject[5] = e.worldToObject[10] = 1.0f;
    e.blas = blas;
    return std::memcmp(&w, &e, sizeof(e)) == 0;
}

// a pinhole camera on the -z side looking along +z: nscreen (nx, ny, 0, 1) -> a world point one unit in front of the eye
static CameraView camera(int w, int h)
{
    CameraView cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position = Vec3f(0.5f, 0.75f, -34.0f);
    F32* m = cam.nscreenToWorld.m;
    m[0] = 0.4f;  m[3] = cam.position.x;
    m[5] = -0.2f; m[7] = cam.position.y;
    m[11] = cam.position.z + 1.0f;
    m[15] = 1.0f;
    cam.cameraFar = 200.0f;
    cam.width = w;
    cam.height = h;
    return cam;
}

static void cpuTests()
{
    CudaInstancedBVH a;
    CHECK(!a.hasWorld() && a.getWorldBLAS() == -1);
    CHECK(refused([&] { a.setWorld(0); }, "outside"));                                      // an empty pool has no BLAS 0
    a.clearWorld();                                                                         // nothing to clear: harmless
    // a pool of two host-built trees
    const Vec3i tris[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)};
    const Vec3f verts[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)};
    Scene scene(2, tris, 4, verts);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);
    CHECK(a.addBLAS(sah) == 0 && a.addBLAS(sah) == 1);
    CHECK(refused([&] { a.setWorld(2); }, "outside") && refused([&] { a.setWorld(-1); }, "outside"));
    CHECK(refused([&] { a.setWorld(1, ""); }, "kernel name") && !a.hasWorld());
    // before setInstances: the world's record is the only one
    a.setWorld(1);
    CHECK(a.hasWorld() && a.getWorldBLAS() == 1 && a.getNumInstances() == 0);
    CHECK(a.getInstanceBuffer().getSize() == (S64)sizeof(NtrInstance) && isWorldRecord(*(const NtrInstance*)a.getInstanceBuffer().getPtr(), 1));
    const float m[24] = {2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3, 1, 0, 0, -4, 0, 1, 0, 0, 0, 0, 1, 0};
    const S32 which[3] = {0, 1, 0};
    a.setInstances(2, m, which);
    CHECK(a.getNumInstances() == 2 && a.getInstanceBuffer().getSize() == 3 * (S64)sizeof(NtrInstance));
    {
        const NtrInstance* inst = (const NtrInstance*)a.getInstanceBuffer().getPtr();
        CHECK(inst[0].blas == 0 && inst[1].blas == 1 && inst[0].objectToWorld[3] == 1.0f && inst[0].worldToObject[0] == 0.5f);
        CHECK(isWorldRecord(inst[2], 1));
    }
    a.setWorld(0, "kepler_dynamic_fetch");                                                  // another world: the record follows
    CHECK(a.getWorldBLAS() == 0 && isWorldRecord(((const NtrInstance*)a.getInstanceBuffer().getPtr())[2], 0));
    a.clearWorld();
    CHECK(!a.hasWorld() && a.getInstanceBuffer().getSize() == 2 * (S64)sizeof(NtrInstance));
    CHECK(((const NtrInstance*)a.getInstanceBuffer().getPtr())[1].blas == 1);               // the instances' records stay
    a.setWorld(1);
    CHECK(a.getInstanceBuffer().getSize() == 3 * (S64)sizeof(NtrInstance));
    const float m3[36] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 5, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, -5, 0, 1, 0, 0, 0, 0, 1, 0};
    a.setInstances(3, m3, which);                                                           // another count: the record moves behind them
    CHECK(a.getInstanceBuffer().getSize() == 4 * (S64)sizeof(NtrInstance) && isWorldRecord(((const NtrInstance*)a.getInstanceBuffer().getPtr())[3], 1));
    CHECK(((const NtrInstance*)a.getInstanceBuffer().getPtr())[2].blas == 0 && !a.isBuilt());
    // the world is no instance: without a TLAS over at least one instance nothing is traced
    RayBuffer rays;
    Buffer ids;
    rays.resize(64);
    CHECK(refused([&] { a.traceBatch(rays, ids); }, "No TLAS"));
    CudaInstancedBVH b;
    CHECK(b.addBLAS(sah) == 0);
    b.setWorld(0);
    CHECK(refused([&] { b.traceBatch(rays, ids); }, "No TLAS") && refused([&] { b.build(); }, "nothing to build"));
    int count = -1;
    if (!(ntr_device_count(&count) == NTR_OK && count > 0)) std::printf("no device: the world is bookkeeping only\n");
}

struct Frame {
    std::vector<U8>  primary;       // resolved primary records
    std::vector<U32> pixels;
    std::vector<U8>  aoHit;         // per AO slot, in batch order: the record is a hit
    int hits;
};

static Frame render(CudaInstancedBVH& bvh, Buffer& tri, S32 numVerts, Buffer& pos, Buffer& mat, Buffer& shaded, InstancedRenderer::RayType type, bool wide,
                    int W, int H, int NS)
{
    Frame f;
    const int n = W * H;
    InstancedRenderer r(bvh);
    r.setGeometry(tri, numVerts, pos);
    r.setParams(type, 3.0f, NS);
    r.setWide(wide);
    Buffer pixels;
    pixels.resizeDiscard((S64)n * 4);
    pixels.clear(0);
    const CameraView cam = camera(W, H);
    r.beginFrame(cam, W, H);
    while (r.nextBatch()) {
        CHECK(r.traceBatch() > 0.0f);
        r.updateResult(pixels, mat, shaded);
        if (type != InstancedRenderer::RayType_Primary) {
            const S32 k = r.getBatchRays()->getSize();
            const NtrRayResult* res = (const NtrRayResult*)r.getBatchResolvedBuffer().getPtr();
            for (S32 i = 0; i < k; i++) f.aoHit.push_back(res[i].id != -1 ? 1 : 0);
        }
    }
    const U8* p = (const U8*)r.getPrimaryResolvedBuffer().getPtr();
    f.primary.assign(p, p + (size_t)n * 16);
    const U32* px = (const U32*)pixels.getPtr();
    f.pixels.assign(px, px + n);
    f.hits = r.getTotalNumRays();
    return f;
}

static void gpuTests(const std::string& dir)
{
    std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
    std::vector<float> vtx = load<float>(dir, "pos.bin");
    std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
    std::vector<float> xf = load<float>(dir, "transforms.bin");
    std::vector<S32> which = load<S32>(dir, "blas.bin");
    std::vector<S32> worldOf = load<S32>(dir, "world.bin");
    if (g_failed) return;
    const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, B = (S32)meshes.size(), N = (S32)which.size(), world = worldOf[0];
    CHECK(numTris > 0 && B == 3 && N == 32 && (S32)xf.size() == 12 * N && world >= 0 && world < B);
    Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12);
    std::vector<U32> mc((size_t)numTris), sc((size_t)numTris);
    for (S32 i = 0; i < numTris; i++) {
        mc[i] = 0xff000000u | (U32)(i * 2654435761u >> 8);
        sc[i] = 0xff000000u | (U32)((i + 77) * 40503u);
    }
    Buffer mat(mc.data(), (S64)numTris * 4), shaded(sc.data(), (S64)numTris * 4);

    // a: the N instances and a world.  b: N + 1 instances, the world being identity instance N
    CudaInstancedBVH a, b;
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    a.setInstances(N, xf.data(), which.data());
    a.build();
    CHECK(refused([&] { a.setWorld(B); }, "outside") && a.isBuilt());
    a.setWorld(world);
    CHECK(a.isBuilt() && a.hasWorld() && a.getNumInstances() == N);                         // the TLAS never sees the world
    CHECK(a.getInstanceBuffer().getSize() == (S64)(N + 1) * (S64)sizeof(NtrInstance));
    CHECK(isWorldRecord(((const NtrInstance*)a.getInstanceBuffer().getPtr())[N], world));
    std::vector<float> xfAll(xf);
    std::vector<S32> whichAll(which);
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    xfAll.insert(xfAll.end(), identity, identity + 12);
    whichAll.push_back(world);
    b.buildBLASes(B, meshes.data(), tri, numVerts, pos);
    b.setInstances(N + 1, xfAll.data(), whichAll.data());
    b.build();
    CHECK(std::memcmp(a.getInstanceBuffer().getPtr(), b.getInstanceBuffer().getPtr(), (size_t)N * sizeof(NtrInstance)) == 0);
    {
        // the world's record against the identity instance's: the same matrices as floats (ntr_instance_invert may sign its zeros)
        const NtrInstance &wa = ((const NtrInstance*)a.getInstanceBuffer().getPtr())[N], &wb = ((const NtrInstance*)b.getInstanceBuffer().getPtr())[N];
        bool same = wa.blas == wb.blas;
        for (int k = 0; k < 12; k++) same = same && wa.objectToWorld[k] == wb.objectToWorld[k] && wa.worldToObject[k] == wb.worldToObject[k];
        CHECK(same);
    }

    const int W = 64, H = 32, NS = 4, n = W * H;
    InstancedRenderer r(a);
    r.setGeometry(tri, numVerts, pos);
    r.beginFrame(camera(W, H), W, H);
    RayBuffer& p = r.getPrimaryRays();
    CHECK(p.getSize() == n);

    // traceBatch with a world equals the C-ABI sequence, binary and wide, closest and any, with and without masks
    a.widen();
    CHECK(a.isWide() && a.hasWorld());
    std::vector<U32> masks((size_t)N);
    for (S32 i = 0; i < N; i++) masks[i] = (i % 3 == 0) ? 0x80000001u : (i % 3 == 1 ? 2u : 3u);
    const NtrBlasRange wr = a.getBLASRange(world);
    std::vector<S32> idsSeeded;
    for (int pass = 0; pass < 2; pass++) {
        if (pass) a.setInstanceMasks(masks.data());
        for (int anyHit = 0; anyHit < 2; anyHit++)
            for (U32 rayMask : {0xFFFFFFFFu, 2u})
                for (int wide = 0; wide < 2; wide++) {
                    p.setNeedClosestHit(!anyHit);
                    a.setTraceWide(wide != 0);
                    Buffer ids, idsDirect;
                    p.getResultBuffer().clear(0x33);
                    const F32 sec = a.traceBatch(p, ids, rayMask);
                    CHECK(sec > 0.0f);
                    std::vector<U8> res((const U8*)p.getResultBuffer().getPtr(), (const U8*)p.getResultBuffer().getPtr() + (size_t)n * 16);
                    p.getResultBuffer().clear(0x5a);
                    idsDirect.resizeDiscard((S64)n * 4);
                    NtrInstanceVisibility vis;
                    vis.d_instanceMasks = pass ? (const uint32_t*)a.getInstanceMaskBuffer().getCudaPtr() : NULL;
                    vis.d_rayMasks = NULL;
                    vis.rayMask = rayMask;
                    vis.pad = 0;
                    float s0 = 0.0f, s1 = 0.0f;
                    const NtrRay* d_rays = (const NtrRay*)p.getRayBuffer().getCudaPtr();
                    NtrRayResult* d_res = (NtrRayResult*)p.getResultBuffer().getMutableCudaPtr();
                    int rc = ntr_trace_bvh("fermi_speculative_while_while", n, anyHit, d_rays, d_res,
                                           (const U8*)a.getPoolNodeBuffer().getCudaPtr() + wr.nodesOffset, wr.nodesBytes,
                                           (const U8*)a.getPoolTriWoopBuffer().getCudaPtr() + wr.triWoopOffset, wr.triWoopBytes,
                                           (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr() + wr.triWoopOffset / 16, BVHLayout_Compact, 0u, NULL,
                                           &s0);
                    CHECK(rc == NTR_OK);
                    if (wide)
                        rc = ntr_trace_instanced_wide_seeded(n, anyHit, d_rays, d_res, N, d_res, (int32_t*)idsDirect.getMutableCudaPtr(),
                                                             a.getWideTLASNodeBuffer().getCudaPtr(), a.getWideResult().nodesBytes, 0,
                                                             a.getWideRecordBuffer().getCudaPtr(), N, a.getWidePoolNodeBuffer().getCudaPtr(),
                                                             a.getWidePoolResult().nodesBytes, a.getPoolTriWoopBuffer().getCudaPtr(),
                                                             a.getPoolTriWoopBuffer().getSize(), (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(),
                                                             &vis, &s1, NULL);
                    else
                        rc = ntr_trace_instanced_seeded(n, anyHit, d_rays, d_res, N, d_res, (int32_t*)idsDirect.getMutableCudaPtr(),
                                                        a.getTLASNodeBuffer().getCudaPtr(), 64 * (S64)(N - 1), 0, a.getRecordBuffer().getCudaPtr(), N,
                                                        a.getPoolNodeBuffer().getCudaPtr(), a.getPoolNodeBuffer().getSize(),
                                                        a.getPoolTriWoopBuffer().getCudaPtr(), a.getPoolTriWoopBuffer().getSize(),
                                                        (const int32_t*)a.getPoolTriIndexBuffer().getCudaPtr(), &vis, &s1, NULL);
                    CHECK(rc == NTR_OK && s0 > 0.0f && s1 > 0.0f);
                    CHECK(std::memcmp(res.data(), p.getResultBuffer().getPtr(), (size_t)n * 16) == 0);
                    CHECK(ids.getSize() == (S64)n * 4 && std::memcmp(ids.getPtr(), idsDirect.getPtr(), (size_t)n * 4) == 0);
                    const S32* id = (const S32*)ids.getPtr();
                    int inWorld = 0, inInstance = 0;
                    for (int i = 0; i < n; i++) { inWorld += id[i] == N ? 1 : 0; inInstance += (id[i] >= 0 && id[i] < N) ? 1 : 0; }
                    CHECK(inWorld > 0 && (inInstance > 0 || anyHit || rayMask == 2u));
                    if (!pass && !anyHit && rayMask == 0xFFFFFFFFu && !wide) idsSeeded.assign(id, id + n);
                }
    }
    a.setTraceWide(false);
    a.setInstanceMasks(NULL);
    p.setNeedClosestHit(true);
    unsigned int status = 0;
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);

    // the world as an ordinary identity instance gives the same instance ids ...
    {
        Buffer ids;
        b.traceBatch(p, ids);
        int differ = 0;
        const S32* id = (const S32*)ids.getPtr();
        for (int i = 0; i < n; i++) differ += id[i] != idsSeeded[(size_t)i] ? 1 : 0;
        std::printf("primary instance ids: %d of %d differ\n", differ, n);
        CHECK(differ == 0);
    }
    // ... and the same frames
    for (int wide = 0; wide < 2; wide++) {
        const Frame pa = render(a, tri, numVerts, pos, mat, shaded, InstancedRenderer::RayType_Primary, wide != 0, W, H, NS);
        const Frame pb = render(b, tri, numVerts, pos, mat, shaded, InstancedRenderer::RayType_Primary, wide != 0, W, H, NS);
        const Frame aa = render(a, tri, numVerts, pos, mat, shaded, InstancedRenderer::RayType_AO, wide != 0, W, H, NS);
        const Frame ab = render(b, tri, numVerts, pos, mat, shaded, InstancedRenderer::RayType_AO, wide != 0, W, H, NS);
        int recDiff = 0, realDiff = 0, pixDiff = 0, aoPixDiff = 0, aoDiff = 0, lit = 0;
        for (int i = 0; i < n; i++) {
            const NtrRayResult *x = (const NtrRayResult*)pa.primary.data() + i, *y = (const NtrRayResult*)pb.primary.data() + i;
            recDiff += (x->id != y->id || std::memcmp(&x->t, &y->t, 4) != 0) ? 1 : 0;
            if (idsSeeded[(size_t)i] != N) realDiff += std::memcmp(x, y, 16) != 0 ? 1 : 0;   // (a world hit's u, v are the single-level kernel's)
            pixDiff += pa.pixels[(size_t)i] != pb.pixels[(size_t)i] ? 1 : 0;
            aoPixDiff += aa.pixels[(size_t)i] != ab.pixels[(size_t)i] ? 1 : 0;
            lit += pa.pixels[(size_t)i] != 0u ? 1 : 0;
        }
        CHECK(aa.aoHit.size() == ab.aoHit.size() && !aa.aoHit.empty());
        for (size_t i = 0; i < aa.aoHit.size() && i < ab.aoHit.size(); i++) aoDiff += aa.aoHit[i] != ab.aoHit[i] ? 1 : 0;
        std::printf("%s frames %dx%d, %d samples: world against identity instance: %d of %d primary records differ in id or t, %d in a real "
                    "instance's words, %d primary pixels, %d of %zu AO rays in hit or miss, %d AO pixels\n", wide ? "wide" : "binary", W, H, NS, recDiff,
                    n, realDiff, pixDiff, aoDiff, aa.aoHit.size(), aoPixDiff);
        CHECK(recDiff == 0 && realDiff == 0 && pixDiff == 0 && aoDiff == 0 && aoPixDiff == 0);
        CHECK(lit > n / 8 && pa.hits == pb.hits && aa.hits == ab.hits && aa.hits > 0);
        CHECK(std::memcmp(aa.primary.data(), pa.primary.data(), (size_t)n * 16) == 0);
        CHECK(!a.getTraceWide() && a.hasWorld());
    }
    CHECK(ntr_trace_status(NULL, &status) == NTR_OK && status == 0);
    // clearWorld: the N instances alone again, ntr_trace_instanced's bytes
    a.clearWorld();
    CHECK(a.isBuilt() && a.getInstanceBuffer().getSize() == (S64)N * (S64)sizeof(NtrInstance));
    {
        Buffer ids;
        a.traceBatch(p, ids);
        const S32* id = (const S32*)ids.getPtr();
        int inWorld = 0;
        for (int i = 0; i < n; i++) inWorld += id[i] == N ? 1 : 0;
        CHECK(inWorld == 0);
    }
    a.setWorld(world);
    a.buildBLASes(B, meshes.data(), tri, numVerts, pos);                                    // the pool is replaced: the world goes with it
    CHECK(!a.hasWorld());
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
    if (g_failed) { std::printf("instanced_seeded_host_test %s: %d check(s) FAILED\n", gpu ? "gpu" : "cpu", g_failed); return 1; }
    std::printf("instanced_seeded_host_test %s: ok\n", gpu ? "gpu" : "cpu");
    return 0;
}
