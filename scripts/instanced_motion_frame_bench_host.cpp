// instanced_motion_frame_bench_host.cpp -- the host-mirror half of scripts/instanced_motion_frame_bench.py: whole AO frames
// through InstancedRenderer over a CudaInstancedBVH with a motion key, setMotionBlur on against off over the same motion-refitted
// buffers.  `<dir> <name> <w> <h> <samples> <reps> <warmup>`: the scene the script wrote into <dir> (tri.bin, pos.bin, meshes.bin,
// transforms.bin, transforms1.bin, blas.bin); frames alternate (off, on, off, on, ...); one JSON line with the wall-clock milliseconds
// of each frame from beginFrame to its last updateResult (the mirror synchronises after every step) and the two-level trace's GPU
// milliseconds inside it.  Compiled by the script with plain g++ against libntrace_amd.so, and run as a child process of its own.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "InstancedRenderer.hpp"

using namespace FW;

template <class T>
static std::vector<T> load(const std::string& dir, const char* name)
{
    const std::string path = dir + "/" + name;
    std::vector<T> out;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)bytes / sizeof(T));
    if (std::fread(out.data(), 1, (size_t)bytes, f) != (size_t)bytes) { std::printf("short read of %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return out;
}

static void spread(const char* key, std::vector<double> v, int warmup)
{
    v.erase(v.begin(), v.begin() + warmup);
    std::sort(v.begin(), v.end());
    std::printf("\"%s\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}", key, v[v.size() / 2], v.front(), v.back());
}

int main(int argc, char** argv)
{
    if (argc < 8) { std::printf("usage: %s <dir> <name> <w> <h> <samples> <reps> <warmup>\n", argv[0]); return 2; }
    const std::string dir = argv[1], name = argv[2];
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), NS = std::atoi(argv[5]), reps = std::atoi(argv[6]), warmup = std::atoi(argv[7]);
    try {
        std::vector<S32> triIdx = load<S32>(dir, "tri.bin");
        std::vector<float> vtx = load<float>(dir, "pos.bin");
        std::vector<NtrPlocBatchMesh> meshes = load<NtrPlocBatchMesh>(dir, "meshes.bin");
        std::vector<float> xf = load<float>(dir, "transforms.bin"), xf1 = load<float>(dir, "transforms1.bin"), camf = load<float>(dir, "camera.bin");
        std::vector<S32> which = load<S32>(dir, "blas.bin");
        const S32 numTris = (S32)triIdx.size() / 3, numVerts = (S32)vtx.size() / 3, N = (S32)which.size();
        Buffer tri(triIdx.data(), (S64)numTris * 12), pos(vtx.data(), (S64)numVerts * 12);
        std::vector<U32> colours((size_t)numTris, 0xff808080u);
        Buffer mat(colours.data(), (S64)numTris * 4), shaded(colours.data(), (S64)numTris * 4);
        CameraView cam;                          // camera.bin: the eye, nscreenToWorld (row-major), the far plane
        cam.position = Vec3f(camf[0], camf[1], camf[2]);
        for (int k = 0; k < 16; k++) cam.nscreenToWorld.m[k] = camf[3 + (size_t)k];
        cam.cameraFar = camf[19];
        cam.width = W;
        cam.height = H;

        CudaInstancedBVH a;
        a.buildBLASes((S32)meshes.size(), meshes.data(), tri, numVerts, pos);
        a.setInstances(N, xf.data(), which.data());
        a.build();
        a.setMotionKey(N, xf1.data());
        a.refitMotion();
        a.setTime(0.0f);
        InstancedRenderer r(a);
        r.setGeometry(tri, numVerts, pos);
        r.setParams(InstancedRenderer::RayType_AO, 5.0f, NS);
        Buffer pixels;
        pixels.resizeDiscard((S64)W * H * 4);
        std::vector<double> wall[2], gpu[2];
        int rays = 0, batches = 0;
        for (int i = 0; i < 2 * (warmup + reps); i++) {
            const int on = i & 1;                // alternated: off, on, off, on, ...
            r.setMotionBlur(on != 0, (U32)i);
            const auto t0 = std::chrono::steady_clock::now();
            double sec = 0.0;
            r.beginFrame(cam, W, H);
            batches = 0;
            while (r.nextBatch()) {
                sec += r.traceBatch();
                r.updateResult(pixels, mat, shaded);
                batches++;
            }
            wall[on].push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            gpu[on].push_back(sec * 1e3);
            rays = r.getTotalNumRays();
        }
        std::printf("{\"part\": \"frame\", \"frame\": \"%s\", \"instances\": %d, \"moving\": %d, \"width\": %d, \"height\": %d, \"samples\": %d, "
                    "\"ao_rays\": %d, \"batches\": %d, ", name.c_str(), N, a.getMotionRefitResult().numMoving, W, H, NS, rays, batches);
        spread("off_wall_ms", wall[0], warmup); std::printf(", ");
        spread("on_wall_ms", wall[1], warmup); std::printf(", ");
        spread("off_secondary_trace_ms", gpu[0], warmup); std::printf(", ");
        spread("on_secondary_trace_ms", gpu[1], warmup);
        std::printf("}\n");
    } catch (const FatalError& e) {
        std::printf("FatalError: %s\n", e.message.c_str());
        return 1;
    }
    return 0;
}
