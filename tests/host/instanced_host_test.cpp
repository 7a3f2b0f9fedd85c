// instanced_host_test.cpp -- the host mirror's instanced scenes (CudaInstancedBVH): addBLAS copies a CudaBVH's buffers to aligned pool
// offsets without rewriting a word, setInstances inverts with ntr_instance_invert and refuses a singular transform, and a build without
// a device is refused (`cpu`); on a GPU (`gpu <dir>`) a pool of a device PLOC tree and a host SAH tree, seeded instances, the top-level
// build and closest-hit and any-hit batches, whose buffers and records are dumped for tests/test_instanced_host.py.  Compiled with
// plain g++ against libntrace_amd.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaInstancedBVH.hpp"
#include "CudaPLOCBuilder.hpp"
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

// rotation about (1, 2, 3) / |.| by `angle`, times diag(s), then the translation t
static void makeTransform(float angle, Vec3f s, Vec3f t, float* m)
{
    const double n = std::sqrt(14.0), x = 1 / n, y = 2 / n, z = 3 / n, c = std::cos((double)angle), sn = std::sin((double)angle), k = 1 - c;
    const double r[9] = {c + x * x * k, x * y * k - z * sn, x * z * k + y * sn, y * x * k + z * sn, c + y * y * k, y * z * k - x * sn,
                         z * x * k - y * sn, z * y * k + x * sn, c + z * z * k};
    const float sc[3] = {s.x, s.y, s.z}, tr[3] = {t.x, t.y, t.z};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) m[4 * i + j] = (float)(r[3 * i + j] * sc[j]);
        m[4 * i + 3] = tr[i];
    }
}

static bool sameRange(Buffer& pool, S64 ofs, Buffer& src)
{
    return std::memcmp(pool.getPtr(ofs), src.getPtr(), (size_t)src.getSize()) == 0;
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
    CudaBVH a(bvh, BVHLayout_Compact);
    platform.setLeafPreferences(1, 1);
    BVH bvh1(&scene, platform, params);
    CudaBVH b(bvh1, BVHLayout_Compact);

    CudaInstancedBVH inst;
    CHECK((int)CudaInstancedBVH::DefaultRadius == 8);
    CHECK(inst.addBLAS(a) == 0 && inst.addBLAS(b) == 1 && inst.getNumBLAS() == 2);
    const NtrBlasRange r0 = inst.getBLASRange(0), r1 = inst.getBLASRange(1);
    CHECK(r0.nodesOffset == 0 && r0.nodesBytes == a.getNodeBuffer().getSize() && r0.triWoopOffset == 0 && r0.triWoopBytes == a.getTriWoopBuffer().getSize());
    CHECK(r1.nodesOffset == r0.nodesBytes && r1.nodesOffset % 64 == 0 && r1.triWoopOffset == r0.triWoopBytes && r1.triWoopOffset % 16 == 0);
    CHECK(inst.getPoolNodeBuffer().getSize() == r1.nodesOffset + r1.nodesBytes);
    CHECK(inst.getPoolTriIndexBuffer().getSize() * 4 == inst.getPoolTriWoopBuffer().getSize());
    // no word is rewritten: each range is the BLAS byte for byte
    CHECK(sameRange(inst.getPoolNodeBuffer(), r0.nodesOffset, a.getNodeBuffer()) && sameRange(inst.getPoolNodeBuffer(), r1.nodesOffset, b.getNodeBuffer()));
    CHECK(sameRange(inst.getPoolTriWoopBuffer(), r1.triWoopOffset, b.getTriWoopBuffer()));
    CHECK(sameRange(inst.getPoolTriIndexBuffer(), r1.triWoopOffset / 4, b.getTriIndexBuffer()));
    CudaBVH other((BVHLayout)0);
    bool threw = false;
    try { inst.addBLAS(other); } catch (const FatalError&) { threw = true; }
    CHECK(threw);

    float m[24];
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(m, identity, sizeof(identity));
    makeTransform(0.7f, Vec3f(2.0f, -0.5f, 1.5f), Vec3f(3.0f, -4.0f, 5.0f), m + 12);
    const S32 which[2] = {0, 1};
    inst.setInstances(2, m, which);
    CHECK(inst.getNumInstances() == 2 && inst.getInstanceBuffer().getSize() == 2 * (S64)sizeof(NtrInstance));
    const NtrInstance* in = (const NtrInstance*)inst.getInstanceBuffer().getPtr();
    bool isIdentity = true;   // (the translation is -(0): equal to the identity's zero as a number, not as a word)
    for (int k = 0; k < 12; k++) isIdentity = isIdentity && in[0].worldToObject[k] == identity[k];
    CHECK(isIdentity && in[1].blas == 1);
    float w2o[12];
    CHECK(ntr_instance_invert(m + 12, w2o) == NTR_OK && std::memcmp(in[1].worldToObject, w2o, sizeof(w2o)) == 0);
    const float singular[12] = {1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0};
    CHECK(ntr_instance_invert(singular, w2o) == NTR_ERR_INVALID);
    threw = false;
    try { CudaInstancedBVH bad; bad.addBLAS(a); const S32 z = 0; bad.setInstances(1, singular, &z); } catch (const FatalError&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { CudaInstancedBVH empty; empty.build(); } catch (const FatalError&) { threw = true; }
    CHECK(threw);
    // valid arguments and no device: the build is refused
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        threw = false;
        try { inst.build(); } catch (const FatalError& e) { threw = true; std::printf("no device: build refused (%s)\n", e.message.c_str()); }
        CHECK(threw);
        int64_t held = -1;
        CHECK(ntr_tlas_scratch_bytes(&held) == NTR_OK && held == 0);
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
static void dump(const char* dir, const std::string& name, Buffer& b, S64 bytes = -1) { dump(dir, name, b.getPtr(), (size_t)(bytes < 0 ? b.getSize() : bytes)); }

static void gpuTests(const char* dir)
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 6);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    CudaPLOCBuilder ploc(&scene);
    Platform platform("GPU");
    BVH::BuildParams params;
    BVH bvh(&scene, platform, params);
    CudaBVH sah(bvh, BVHLayout_Compact);   // leaves of several triangles

    CudaInstancedBVH inst;
    CHECK(inst.addBLAS(ploc) == 0 && inst.addBLAS(sah) == 1);
    const int N = 27;
    std::vector<float> m(12 * N);
    std::vector<S32> which(N);
    for (int i = 0; i < N; i++) {
        const Vec3f t(4.5f * (i % 3 - 1), 4.5f * ((i / 3) % 3 - 1), 4.5f * (i / 9 - 1));
        makeTransform(0.37f * i, Vec3f(1.0f + 0.05f * i, (i % 5 == 0) ? -0.8f : 0.9f, 1.1f), t, &m[12 * i]);
        which[i] = i % 2;
    }
    inst.setInstances(N, m.data(), which.data());
    inst.build();
    const NtrTlasResult& res = inst.getBuildResult();
    CHECK(res.rootLink == 0 && res.numNodes == N - 1 && res.nodesBytes == 64 * (N - 1) && res.recordsBytes == 64 * N);
    CHECK(res.height >= 5 && res.height <= N - 1 && res.numRounds >= res.height && res.tailClusters == N);
    CHECK(inst.getTLASNodeBuffer().getSize() == res.nodesBytes);
    std::printf("TLAS: %d instances, %d rounds, height %d, %.3f ms\n", N, res.numRounds, res.height, res.seconds * 1e3f);
    dump(dir, "pool_nodes.bin", inst.getPoolNodeBuffer());
    dump(dir, "pool_woop.bin", inst.getPoolTriWoopBuffer());
    dump(dir, "pool_index.bin", inst.getPoolTriIndexBuffer());
    dump(dir, "instances.bin", inst.getInstanceBuffer());
    dump(dir, "tlas.bin", inst.getTLASNodeBuffer());
    dump(dir, "records.bin", inst.getRecordBuffer(), res.recordsBytes);
    std::vector<NtrBlasRange> ranges = {inst.getBLASRange(0), inst.getBLASRange(1)};
    dump(dir, "ranges.bin", ranges.data(), ranges.size() * sizeof(NtrBlasRange));

    const int W = 96, H = 64;
    for (int anyHit = 0; anyHit < 2; anyHit++) {
        RayBuffer rays(W * H, anyHit == 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                Ray r;
                r.origin = Vec3f(0.3f, 0.7f, -16.0f);
                r.direction = Vec3f((x + 0.5f) / W - 0.5f, (y + 0.5f) / H - 0.5f, 1.0f);
                r.tmin = 0.0f;
                r.tmax = anyHit ? 14.0f : 100.0f;
                rays.setRay(y * W + x, r);
            }
        Buffer ids;
        const F32 sec = inst.traceBatch(rays, ids);
        CHECK(sec > 0.0f && ids.getSize() == (S64)W * H * 4);
        const S32* id = (const S32*)ids.getPtr();
        S64 hits = 0;
        for (int i = 0; i < W * H; i++) {
            const RayResult& rr = rays.getResultForSlot(i);
            CHECK((rr.id >= 0) == (id[i] >= 0) && id[i] < N);
            hits += rr.id >= 0;
        }
        CHECK(hits > W * H / 8 && hits < W * H);
        const std::string kind = anyHit ? "any" : "closest";
        dump(dir, kind + "_rays.bin", rays.getRayBuffer());
        dump(dir, kind + "_results.bin", rays.getResultBuffer());
        dump(dir, kind + "_ids.bin", ids);
        std::printf("instanced %s hit: %d rays, %lld hits, %.3f ms\n", kind.c_str(), W * H, (long long)hits, sec * 1e3f);
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
    std::printf("instanced_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
