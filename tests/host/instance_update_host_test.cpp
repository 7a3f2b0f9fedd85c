// instance_update_host_test.cpp -- the host mirror's device-side instance update (CudaInstancedBVH::setInstancesDevice over
// ntr_instances_update): its argument refusals and its refusal without a device (`cpu`); on a GPU (`gpu`) the instance array equals
// ntr_instances_update_host's and what setInstances makes of the flattened matrices, and the state follows setInstances': isBuilt()
// falls, an unchanged count keeps the topology for refit() and the masks, another count drops both, a world's record is kept, and a
// singular node fails the checked form and shows in the status of the unchecked one.  Compiled with plain g++ against libntrace_amd.so.
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

// a tessellated unit-ish box
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
    const Vec3f lo(-1.0f, -0.75f, -0.5f), d(2.0f, 1.5f, 1.0f);
    quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
    quad(Vec3f(lo.x, lo.y, lo.z + d.z), Vec3f(d.x, 0, 0), Vec3f(0, d.y, 0));
    quad(lo, Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
    quad(Vec3f(lo.x, lo.y + d.y, lo.z), Vec3f(d.x, 0, 0), Vec3f(0, 0, d.z));
    quad(lo, Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
    quad(Vec3f(lo.x + d.x, lo.y, lo.z), Vec3f(0, d.y, 0), Vec3f(0, 0, d.z));
}

// rotation about (1, 2, 3) / |.| by `angle`, times the uniform scale s, then the translation t
static void makeTransform(float angle, float s, Vec3f t, float* m)
{
    const double n = std::sqrt(14.0), x = 1 / n, y = 2 / n, z = 3 / n, c = std::cos((double)angle), sn = std::sin((double)angle), k = 1 - c;
    const double r[9] = {c + x * x * k, x * y * k - z * sn, x * z * k + y * sn, y * x * k + z * sn, c + y * y * k, y * z * k - x * sn,
                         z * x * k - y * sn, z * y * k + x * sn, c + z * z * k};
    const float tr[3] = {t.x, t.y, t.z};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) m[4 * i + j] = (float)(r[3 * i + j] * s);
        m[4 * i + 3] = tr[i];
    }
}

// G group nodes under one root, one node per instance under the groups; the root comes last: parents after children
struct Hierarchy {
    int numNodes, num;
    std::vector<float> local;
    std::vector<S32> parent, node, blas;
    Hierarchy(int n, int groups) : numNodes(n + groups + 1), num(n), local(12 * (size_t)(n + groups + 1)), parent(n + groups + 1), node(n), blas(n, 0)
    {
        const int root = n + groups;
        for (int i = 0; i < n; i++) {
            makeTransform(0.37f * i, 0.5f + 0.03f * i, Vec3f(2.5f * (i % 3 - 1), 2.5f * ((i / 3) % 3 - 1), 0.25f * i), &local[12 * (size_t)i]);
            parent[i] = n + i % groups;
            node[i] = n - 1 - i;                     // a permutation
        }
        for (int g = 0; g < groups; g++) {
            makeTransform(1.1f * g, 1.0f + 0.125f * g, Vec3f(6.0f * (g - 1), 0.5f * g, -1.0f), &local[12 * (size_t)(n + g)]);
            parent[n + g] = root;
        }
        makeTransform(0.2f, 1.25f, Vec3f(0.5f, -0.25f, 3.0f), &local[12 * (size_t)root]);
        parent[root] = -1;
    }
};

struct DeviceInputs {
    Buffer local, parent, node, blas;
    explicit DeviceInputs(const Hierarchy& h)
    {
        local.set(h.local.data(), (S64)h.local.size() * 4);
        parent.set(h.parent.data(), (S64)h.parent.size() * 4);
        node.set(h.node.data(), (S64)h.node.size() * 4);
        blas.set(h.blas.data(), (S64)h.blas.size() * 4);
    }
};

static bool threwOn(CudaInstancedBVH& s, const Hierarchy& h, DeviceInputs& d, int numNodes, int num, bool useNode, std::string* msg = NULL)
{
    try { s.setInstancesDevice(numNodes, d.local, &d.parent, num, useNode ? &d.node : NULL, d.blas); }
    catch (const FatalError& e) { if (msg) *msg = e.message; return true; }
    (void)h;
    return false;
}

static void cpuTests()
{
    Hierarchy h(9, 3);
    DeviceInputs d(h);
    CudaInstancedBVH s;
    // refused whatever the machine has: counts below one, fewer nodes than instances without a node array, buffers below their counts
    CHECK(threwOn(s, h, d, h.numNodes, 0, true) && threwOn(s, h, d, 0, h.num, true) && threwOn(s, h, d, 4, 9, false));
    CHECK(threwOn(s, h, d, h.numNodes + 1, h.num, true) && threwOn(s, h, d, h.numNodes, h.num + 1, true));
    CHECK(s.getNumInstances() == 0);
    bool threw = false;
    U32 st[4];
    try { s.getInstanceStatus(st); } catch (const FatalError&) { threw = true; }
    CHECK(threw);
    int count = -1;
    if (ntr_device_count(&count) != NTR_OK || count < 1) {
        std::string msg;
        CHECK(threwOn(s, h, d, h.numNodes, h.num, true, &msg));
        std::printf("no device: setInstancesDevice refused (%s)\n", msg.c_str());
    }
}

static bool sameBytes(Buffer& a, Buffer& b) { return a.getSize() == b.getSize() && std::memcmp(a.getPtr(), b.getPtr(), (size_t)a.getSize()) == 0; }

static bool refitThrows(CudaInstancedBVH& s)
{
    try { s.refit(); } catch (const FatalError&) { return true; }
    return false;
}

static void gpuTests()
{
    std::vector<Vec3i> tris;
    std::vector<Vec3f> verts;
    makeScene(tris, verts, 4);
    Scene scene((S32)tris.size(), tris.data(), (S32)verts.size(), verts.data());
    CudaPLOCBuilder ploc(&scene);

    const int N = 9;
    Hierarchy h(N, 3);
    DeviceInputs d(h);
    // the rule on the host: the expected array, and the flattened matrices for setInstances
    std::vector<NtrInstance> want(N);
    uint32_t wst[4];
    CHECK(ntr_instances_update_host(h.numNodes, h.local.data(), h.parent.data(), N, h.node.data(), h.blas.data(), want.data(), wst) == NTR_OK);
    CHECK(wst[0] == 0 && wst[1] == 0xFFFFFFFFu && wst[2] == 0);
    std::vector<float> flat(12 * (size_t)N);
    for (int i = 0; i < N; i++) std::memcpy(&flat[12 * (size_t)i], want[i].objectToWorld, 48);

    CudaInstancedBVH a, b;
    CHECK(a.addBLAS(ploc) == 0 && b.addBLAS(ploc) == 0);
    a.setInstances(N, flat.data(), h.blas.data());
    b.setInstancesDevice(h.numNodes, d.local, &d.parent, N, &d.node, d.blas);
    CHECK(b.getNumInstances() == N && !b.isBuilt() && b.getInstanceBuffer().getSize() == N * (S64)sizeof(NtrInstance));
    CHECK(std::memcmp(b.getInstanceBuffer().getPtr(), want.data(), N * sizeof(NtrInstance)) == 0);
    CHECK(sameBytes(a.getInstanceBuffer(), b.getInstanceBuffer()));
    const NtrInstancesUpdateResult& ur = b.getInstancesUpdateResult();
    CHECK(ur.numInstances == N && ur.numNodes == h.numNodes && ur.statusBits == 0 && ur.firstBad == 0xFFFFFFFFu && ur.numBad == 0 && ur.updateMs > 0.0f);
    U32 st[4] = {7, 7, 7, 7};
    b.getInstanceStatus(st);
    CHECK(st[0] == 0 && st[1] == 0xFFFFFFFFu && st[2] == 0 && st[3] == 0);
    a.build();
    b.build();
    CHECK(a.isBuilt() && b.isBuilt() && sameBytes(a.getTLASNodeBuffer(), b.getTLASNodeBuffer()) && sameBytes(a.getRecordBuffer(), b.getRecordBuffer()));

    // an unchanged count: isBuilt() falls, the topology and the masks stay, refit() brings the tree to the moved group
    std::vector<U32> masks(N);
    for (int i = 0; i < N; i++) masks[i] = 1u << (i % 5);
    a.setInstanceMasks(masks.data());
    b.setInstanceMasks(masks.data());
    makeTransform(2.0f, 0.75f, Vec3f(-3.0f, 1.0f, 2.0f), &h.local[12 * (size_t)(N + 1)]);     // one group moves: 48 bytes
    d.local.setRange((S64)(N + 1) * 48, &h.local[12 * (size_t)(N + 1)], 48);
    CHECK(ntr_instances_update_host(h.numNodes, h.local.data(), h.parent.data(), N, h.node.data(), h.blas.data(), want.data(), wst) == NTR_OK);
    for (int i = 0; i < N; i++) std::memcpy(&flat[12 * (size_t)i], want[i].objectToWorld, 48);
    a.setInstances(N, flat.data(), h.blas.data());
    b.setInstancesDevice(h.numNodes, d.local, &d.parent, N, &d.node, d.blas, false);          // unchecked: nothing read back
    CHECK(!a.isBuilt() && !b.isBuilt());
    CHECK(b.getInstanceMaskBuffer().getSize() == N * 4 && sameBytes(a.getInstanceMaskBuffer(), b.getInstanceMaskBuffer()));
    CHECK(b.getInstancesUpdateResult().numInstances == 0);                                     // (zero after an unchecked call)
    b.getInstanceStatus(st);
    CHECK(st[0] == 0 && st[1] == 0xFFFFFFFFu && st[2] == 0 && st[3] == 0);
    CHECK(sameBytes(a.getInstanceBuffer(), b.getInstanceBuffer()));
    a.refit();
    b.refit();
    CHECK(a.isBuilt() && b.isBuilt() && sameBytes(a.getTLASNodeBuffer(), b.getTLASNodeBuffer()) && sameBytes(a.getRecordBuffer(), b.getRecordBuffer()));

    // a world's record is kept behind the instances
    a.setWorld(0);
    b.setWorld(0);
    a.setInstances(N, flat.data(), h.blas.data());
    b.setInstancesDevice(h.numNodes, d.local, &d.parent, N, &d.node, d.blas);
    CHECK(b.getInstanceBuffer().getSize() == (N + 1) * (S64)sizeof(NtrInstance) && sameBytes(a.getInstanceBuffer(), b.getInstanceBuffer()));
    const NtrInstance* rec = (const NtrInstance*)b.getInstanceBuffer().getPtr();
    CHECK(rec[N].blas == 0 && rec[N].objectToWorld[0] == 1.0f && rec[N].worldToObject[10] == 1.0f && rec[N].objectToWorld[3] == 0.0f);
    CHECK(b.getInstanceMaskBuffer().getSize() == N * 4);
    a.refit();
    b.refit();                                                                                  // (the count is unchanged: still refittable)
    CHECK(sameBytes(a.getTLASNodeBuffer(), b.getTLASNodeBuffer()));
    a.clearWorld();
    b.clearWorld();

    // another count: the topology and the masks go, as after setInstances
    a.setInstances(N - 1, flat.data(), h.blas.data());
    b.setInstancesDevice(h.numNodes, d.local, &d.parent, N - 1, &d.node, d.blas);
    CHECK(b.getNumInstances() == N - 1 && !b.isBuilt() && b.getInstanceMaskBuffer().getSize() == 0 && a.getInstanceMaskBuffer().getSize() == 0);
    CHECK(sameBytes(a.getInstanceBuffer(), b.getInstanceBuffer()));
    CHECK(refitThrows(a) && refitThrows(b));
    b.build();
    CHECK(b.isBuilt());

    // a singular node: the checked form fails with the instance's index, the unchecked one leaves the status
    std::memset(&h.local[12 * 4], 0, 48);                                                      // node 4 is instance N - 1 - 4's
    d.local.setRange(4 * 48, &h.local[12 * 4], 48);
    std::string msg;
    CHECK(threwOn(b, h, d, h.numNodes, N, true, &msg));
    CHECK(msg.find("instance 4 ") != std::string::npos && msg.find("ntr_instances_update") != std::string::npos);
    std::printf("singular node: %s\n", msg.c_str());
    CHECK(!b.isBuilt() && b.getNumInstances() == N);
    CHECK(b.getInstancesUpdateResult().statusBits == NTR_INSTANCE_ERR_SINGULAR && b.getInstancesUpdateResult().firstBad == 4 && b.getInstancesUpdateResult().numBad == 1);
    b.setInstancesDevice(h.numNodes, d.local, &d.parent, N, &d.node, d.blas, false);
    b.getInstanceStatus(st);
    CHECK(st[0] == NTR_INSTANCE_ERR_SINGULAR && st[1] == 4 && st[2] == 1 && st[3] == 0);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) gpuTests(); else cpuTests();
    } catch (const FatalError& e) {
        std::printf("unexpected FW::fail: %s\n", e.message.c_str());
        return 2;
    }
    std::printf("instance_update_host_test %s: %s\n", gpu ? "gpu" : "cpu", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
