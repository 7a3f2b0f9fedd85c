// instanced_state_host_test.cpp -- what CudaInstancedBVH reports after every call.  `gpu`: one walk over the class's
// public mutators and lazy readers, from four base states (empty; built; built, widened and both FAST flag sets validated; built, widened
// and both motion refits current): every single event from each, and every ordered pair of events from the last two.  After every call
// one line: the step, the event, `ok` or the FatalError's text, every public predicate, count and buffer size that tells the state, and
// after a traceBatch that ran an FNV-1a hash of the records and of the instance ids (the kernels are bit-exact, so another dispatch
// shows).  tests/golden/instanced_state_walk.txt is this output over the class as it stood before its freshness flags were derived from
// one table, in a lossless short form; tests/test_instanced_state_host.py compares.  Only the public API is used: the file compiles against either.
// Every event passes valid arguments; an out-of-order call is refused by the class on the host before any launch, and an error that the
// library reports, or anything that is no FatalError, ends the walk at once.  `cpu`: where InstancedState.hpp exists, exhausts the pure
// state object over all product subsets times all writes.  Compiled with plain g++ against libntrace_amd.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CudaInstancedBVH.hpp"
#include "bvh/Platform.hpp"
#if __has_include("InstancedState.hpp")
#include "InstancedState.hpp"
#define HAVE_INSTANCED_STATE 1
#endif

using namespace FW;

namespace {

// mesh 0: two quads (4 triangles) at z = 0 and z = 0.25; mesh 1: a cube (12 triangles); both inside [-0.5, 0.5]^3
const S32 kTris[16][3] = {{0, 1, 2}, {1, 3, 2}, {4, 5, 6}, {5, 7, 6},
                          {8, 10, 9}, {9, 10, 11}, {12, 13, 14}, {13, 15, 14}, {8, 9, 12}, {9, 13, 12}, {10, 14, 11}, {11, 14, 15},
                          {8, 12, 10}, {10, 12, 14}, {9, 11, 13}, {11, 15, 13}};
const F32 kVerts[16][3] = {{-0.5f, -0.5f, 0}, {0.5f, -0.5f, 0}, {-0.5f, 0.5f, 0}, {0.5f, 0.5f, 0},
                           {-0.5f, -0.5f, 0.25f}, {0.5f, -0.5f, 0.25f}, {-0.5f, 0.5f, 0.25f}, {0.5f, 0.5f, 0.25f},
                           {-0.5f, -0.5f, -0.5f}, {0.5f, -0.5f, -0.5f}, {-0.5f, 0.5f, -0.5f}, {0.5f, 0.5f, -0.5f},
                           {-0.5f, -0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {-0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, 0.5f}};
// two instances side by side and a third behind the gap between them, where a world (BLAS 0 in its own space) lies in front of it;
// key 1 moves the first one only
const F32 kXf[36] = {1, 0, 0, -1.5f, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1.5f, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2};
const F32 kXf1[36] = {1, 0, 0, -1.5f, 0, 1, 0, 0.25f, 0, 0, 1, 0, 1, 0, 0, 1.5f, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2};
const S32 kBlas[3] = {0, 1, 0};
const U32 kMasks[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u};   // the third instance invisible: dropped masks show in the records
const int kNumRays = 65;                             // two waves, the second partial

const char* const kEvents[] = {"addBLAS", "buildBLASes", "refitBLASes", "refitBLASesWide", "optimizeBLASes", "setInstances", "setInstancesCount",
                               "setInstancesDevice", "setInstanceMasks", "setMotionKey", "setMotionKeyDevice", "clearMotion", "build", "refit",
                               "refitMotion", "widen", "refitWide", "refitMotionWide", "setWorld", "clearWorld", "flipTraceWide", "flipTraceFast",
                               "flipTraceWideFast", "flipTraceWideMotion", "getFastFlags", "getWideFastFlags", "traceBatch"};
const int kNumEvents = (int)(sizeof(kEvents) / sizeof(kEvents[0]));
const char* const kBases[] = {"empty", "built", "wide", "motion"};

struct LibraryError { std::string message; };         // a failure the library reported: not a refusal of the class, the walk ends

U64 fnv(const void* data, size_t bytes, U64 h = 0xcbf29ce484222325ull)
{
    const U8* p = (const U8*)data;
    for (size_t i = 0; i < bytes; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// the inputs every event draws on, made once
struct Inputs {
    Buffer tri, pos, nodeLocal, blasDev, key1Dev;
    NtrPlocBatchMesh meshes[2];
    Scene scene;
    Platform platform;
    BVH bvh;
    CudaBVH hostTree;
    RayBuffer rays;

    static const Vec3i* hostTris(void) { static const Vec3i t[2] = {Vec3i(0, 1, 2), Vec3i(1, 3, 2)}; return t; }
    static const Vec3f* hostVerts(void) { static const Vec3f v[4] = {Vec3f(0, 0, 0), Vec3f(1, 0, 0.25f), Vec3f(0, 1, 0.5f), Vec3f(1, 1, 1)}; return v; }

    Inputs(void) : tri(kTris, sizeof(kTris)), pos(kVerts, sizeof(kVerts)), nodeLocal(kXf, sizeof(kXf)), blasDev(kBlas, sizeof(kBlas)),
                   scene(2, hostTris(), 4, hostVerts()), platform("GPU"), bvh(&scene, platform, BVH::BuildParams()),
                   hostTree(bvh, BVHLayout_Compact)
    {
        const NtrPlocBatchMesh m[2] = {{0, 4, {-0.5f, -0.5f, -0.5f}, {0.5f, 0.5f, 0.5f}}, {4, 12, {-0.5f, -0.5f, -0.5f}, {0.5f, 0.5f, 0.5f}}};
        std::memcpy(meshes, m, sizeof(m));
        NtrInstance k1[3];
        std::memset(k1, 0, sizeof(k1));
        for (int i = 0; i < 3; i++) std::memcpy(k1[i].objectToWorld, kXf1 + 12 * i, sizeof(k1[i].objectToWorld));
        key1Dev.set(k1, sizeof(k1));
        rays.resize(kNumRays);                       // a 13 x 5 grid of parallel rays along +z over the three instances
        for (int i = 0; i < kNumRays; i++) {
            Ray r;
            r.origin = Vec3f(-2.25f + 0.375f * (F32)(i % 13), -0.625f + 0.3125f * (F32)(i / 13), -5.0f);
            r.direction = Vec3f(0.0f, 0.0f, 1.0f);
            r.tmin = 0.0f;
            r.tmax = 100.0f;
            rays.setRay(i, r);
        }
    }
};

std::string stateOf(CudaInstancedBVH& a)
{
    char buf[256];
    std::snprintf(buf, sizeof(buf), "built=%d wide=%d widePool=%d fastStale=%d wideFastStale=%d motion=%d motionStale=%d motionWideStale=%d world=%d "
                  "n=%d,%d,%d val=%d,%d refits=%d,%d bytes=%lld,%lld,%lld",
                  (int)a.isBuilt(), (int)a.isWide(), (int)a.isWidePoolCurrent(), (int)a.isFastFlagsStale(), (int)a.isWideFastFlagsStale(),
                  (int)a.hasMotion(), (int)a.isMotionStale(), (int)a.isMotionWideStale(), (int)a.hasWorld(), a.getNumBLAS(), a.getNumInstances(),
                  a.getFirstMeshlessBLAS(), a.getFastValidations(), a.getWideFastValidations(), a.getMotionRefits(), a.getMotionWideRefits(),
                  (long long)a.getInstanceMaskBuffer().getSize(), (long long)a.getInstanceBuffer().getSize(),
                  (long long)a.getMotionInstanceBuffer().getSize());
    return buf;
}

int g_step = 0;

// one event on `a`; -> what it adds to the line (a traceBatch's hashes)
std::string apply(CudaInstancedBVH& a, Inputs& in, int event)
{
    const std::string name = kEvents[event];
    U32 t = 0, p = 0;
    char buf[96] = "";
    if (name == "addBLAS") a.addBLAS(in.hostTree);
    else if (name == "buildBLASes") a.buildBLASes(2, in.meshes, in.tri, 16, in.pos);
    else if (name == "refitBLASes") a.refitBLASes(in.tri, 16, in.pos);
    else if (name == "refitBLASesWide") a.refitBLASesWide(in.tri, 16, in.pos);
    else if (name == "optimizeBLASes") a.optimizeBLASes();
    else if (name == "setInstances") a.setInstances(3, kXf, kBlas);
    else if (name == "setInstancesCount") a.setInstances(2, kXf, kBlas);
    else if (name == "setInstancesDevice") a.setInstancesDevice(3, in.nodeLocal, NULL, 3, NULL, in.blasDev);
    else if (name == "setInstanceMasks") a.setInstanceMasks(kMasks);
    else if (name == "setMotionKey") a.setMotionKey(3, kXf1);
    else if (name == "setMotionKeyDevice") a.setMotionKeyDevice(3, in.key1Dev);
    else if (name == "clearMotion") a.clearMotion();
    else if (name == "build") a.build();
    else if (name == "refit") a.refit();
    else if (name == "refitMotion") a.refitMotion();
    else if (name == "widen") a.widen();
    else if (name == "refitWide") a.refitWide();
    else if (name == "refitMotionWide") a.refitMotionWide();
    else if (name == "setWorld") a.setWorld(0);
    else if (name == "clearWorld") a.clearWorld();
    else if (name == "flipTraceWide") a.setTraceWide(!a.getTraceWide());
    else if (name == "flipTraceFast") a.setTraceFast(!a.getTraceFast());
    else if (name == "flipTraceWideFast") a.setTraceWideFast(!a.getTraceWideFast());
    else if (name == "flipTraceWideMotion") a.setTraceWideMotion(!a.getTraceWideMotion());
    else if (name == "getFastFlags") { a.getFastFlags(t, p); std::snprintf(buf, sizeof(buf), " flags=%x,%x", t, p); }
    else if (name == "getWideFastFlags") { a.getWideFastFlags(t, p); std::snprintf(buf, sizeof(buf), " flags=%x,%x", t, p); }
    else {
        Buffer ids;
        in.rays.getResultBuffer().clear(0x33);
        a.setTime(1.0f);                             // the shutter's close: a motion trace's records are not the static ones
        a.traceBatch(in.rays, ids);
        std::snprintf(buf, sizeof(buf), " records=%016llx ids=%016llx",
                      (unsigned long long)fnv(in.rays.getResultBuffer().getPtr(), (size_t)kNumRays * sizeof(RayResult)),
                      (unsigned long long)fnv(ids.getPtr(), (size_t)kNumRays * sizeof(S32)));
    }
    return buf;
}

// applies the event and prints its line.  A FatalError that carries the library's last error is no refusal of the class: the walk ends
void step(CudaInstancedBVH& a, Inputs& in, const std::string& where, int event)
{
    std::string outcome = "ok", extra;
    try { extra = apply(a, in, event); } catch (const FatalError& e) {
        const char* last = ntr_last_error();
        if (last && last[0] && e.message.find(last) != std::string::npos) { LibraryError err; err.message = e.message; throw err; }
        outcome = e.message;
    }
    std::printf("%d %s %s | %s | %s%s\n", g_step++, where.c_str(), kEvents[event], outcome.c_str(), stateOf(a).c_str(), extra.c_str());
}

int eventNamed(const char* name)
{
    for (int e = 0; e < kNumEvents; e++)
        if (std::strcmp(kEvents[e], name) == 0) return e;
    throw std::string("no event ") + name;
}

// brings a fresh object to base state `base`; with `print`, every call of the set-up is a step of its own
void toBase(CudaInstancedBVH& a, Inputs& in, int base, bool print)
{
    static const char* const built[] = {"buildBLASes", "setInstances", "build", NULL};
    static const char* const wide[] = {"buildBLASes", "setInstances", "build", "widen", "flipTraceWide", "flipTraceFast", "flipTraceWideFast",
                                       "getFastFlags", "getWideFastFlags", NULL};
    static const char* const motion[] = {"buildBLASes", "setInstances", "build", "widen", "setMotionKey", "flipTraceWide", "flipTraceWideMotion",
                                         "refitMotionWide", NULL};
    static const char* const none[] = {NULL};
    const char* const* calls = base == 1 ? built : base == 2 ? wide : base == 3 ? motion : none;
    for (; *calls; calls++) {
        if (print) step(a, in, std::string(kBases[base]) + ":setup", eventNamed(*calls));
        else apply(a, in, eventNamed(*calls));
    }
}

int gpuWalk(void)
{
    Inputs in;
    for (int base = 0; base < 4; base++) {
        { CudaInstancedBVH a; toBase(a, in, base, true); }
        for (int e = 0; e < kNumEvents; e++) {
            CudaInstancedBVH a;
            toBase(a, in, base, false);
            step(a, in, kBases[base], e);
        }
    }
    for (int base = 2; base < 4; base++)
        for (int e1 = 0; e1 < kNumEvents; e1++)
            for (int e2 = 0; e2 < kNumEvents; e2++) {
                CudaInstancedBVH a;
                toBase(a, in, base, false);
                const std::string where = std::string(kBases[base]) + ":" + kEvents[e1] + ">" + kEvents[e2];
                step(a, in, where, e1);
                step(a, in, where, e2);
            }
    unsigned int status = 0;
    if (ntr_trace_status(NULL, &status) != NTR_OK || status != 0) { std::printf("trace status %u\n", status); return 1; }
    return 0;
}

#ifdef HAVE_INSTANCED_STATE
int g_failed = 0;
#define CHECK(X) do { if (!(X)) { std::printf("CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #X); g_failed++; } } while (0)

int cpuTable(void)
{
    typedef InstancedState::Write W;
    typedef InstancedState::Product P;
    const int NP = (int)P::Count, NW = (int)W::Count;
    CHECK(InstancedState().products() == 0u);        // nothing is current before anything was made
    for (U32 set = 0; set < (1u << NP); set++) {
        for (int w = 0; w < NW; w++) {
            InstancedState s(set);
            s.wrote((W)w);
            CHECK((s.products() & ~set) == 0u);                                        // wrote never sets a product
            for (int p = 0; p < NP; p++)                                               // ... and clears exactly the table's
                CHECK(s.has((P)p) == (((set >> p) & 1u) != 0u && !InstancedState::voids((W)w, (P)p)));
        }
        for (int p = 0; p < NP; p++) {
            InstancedState s(set), l(set);
            s.made((P)p);
            l.lost((P)p);
            CHECK(s.products() == (set | (1u << p)) && l.products() == (set & ~(1u << p)));   // made and lost change their own product only
        }
        const InstancedState s(set);
        CHECK(!s.isWide() || s.isBuilt());
        CHECK(s.isWide() == (s.has(P::TlasBoxes) && s.has(P::WidePool) && s.has(P::WideTlas)));
        CHECK(!s.mayRefitWide() || s.mayRefit());
        CHECK(s.isMotionWideStale() || !s.isMotionStale());
    }
    for (int w = 0; w < NW; w++) {
        CHECK(!InstancedState::voids((W)w, P::FastFlags) || InstancedState::voids((W)w, P::WideFastFlags));
        CHECK(!InstancedState::voids((W)w, P::WidePool) || InstancedState::voids((W)w, P::WideTlas));
        CHECK(InstancedState::voids((W)w, P::WideTopology) == InstancedState::voids((W)w, P::TlasTopology));
    }
    if (g_failed) { std::printf("instanced_state_host_test cpu: %d check(s) FAILED\n", g_failed); return 1; }
    std::printf("instanced_state_host_test cpu: ok, %d product sets x %d writes\n", 1 << NP, NW);
    return 0;
}
#endif

}  // namespace

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        if (gpu) {
            const int rc = gpuWalk();
            std::printf("instanced_state_host_test gpu: %s, %d steps\n", rc ? "FAILED" : "done", g_step);
            return rc;
        }
#ifdef HAVE_INSTANCED_STATE
        return cpuTable();
#else
        std::printf("instanced_state_host_test cpu: this checkout has no InstancedState.hpp\n");
        return 1;
#endif
    } catch (const LibraryError& e) {
        std::printf("the library failed, the walk ends: %s\n", e.message.c_str());
    } catch (const FatalError& e) {
        std::printf("FatalError outside an event, the walk ends: %s\n", e.message.c_str());
    } catch (...) {
        std::printf("an error that is no FatalError, the walk ends\n");
    }
    return 2;
}
