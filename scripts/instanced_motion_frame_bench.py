#!/usr/bin/env python
"""What a motion-blurred instanced frame costs beside the trace (ntr_instanced_hit_attributes_motion, ntr_ray_times_primary,
ntr_ray_times_secondary, InstancedRenderer::setMotionBlur), over the two frames of scripts/instanced_motion_bench.py:
ONE identity instance of atrium() and the forest of 4 096 instances of soup1000, each static (key 1 == key 0) and with every instance
moving (instanced_motion_bench.key1).
  * attributes  ntr_instanced_hit_attributes_motion against ntr_instanced_hit_attributes over the records of the 1920 x 1080 primary
                batch, which ntr_trace_instanced_motion wrote at random times in [0, 1): the price of six 16-byte key loads per hit and,
                where instances move, of twelve lerps and a binary64 inverse per moving HIT.  Where nothing moves the outputs must be
                equal
  * times       the two times kernels: 2 073 600 primary times, and their 8 copies each (16.6 M secondary times)
  * frame       a whole AO frame (--ao-samples rays of radius 5 per primary hit) through InstancedRenderer with setMotionBlur on against
                off over the same motion-refitted buffers, by the child program instanced_motion_frame_bench_host.cpp (compiled here):
                wall-clock from beginFrame to the last updateResult
Kernel launches are timed by stream events and alternated (static call, motion call, ...), five runs after two warm-ups; every figure is
the median with its minimum and maximum.  One JSON line per row; --out writes them as a list.  One process for the kernels and one
child per frame; every GPU step runs under a time limit of its own.

    timeout -k 10 900 python scripts/instanced_motion_frame_bench.py --out instanced_motion_frame.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from instanced_bench import Blas, Tlas, rotations, step, transforms, up  # noqa: E402
from instanced_motion_bench import key1, spread  # noqa: E402

F = np.float32
MESH_DTYPE = np.dtype([("firstTri", "<i4"), ("numTris", "<i4"), ("sceneMin", "<f4", (3,)), ("sceneMax", "<f4", (3,))])


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def build_host_program(tmp):
    out = os.path.join(tmp, "instanced_motion_frame_bench_host")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc +
                          [os.path.join(ROOT, "scripts", "instanced_motion_frame_bench_host.cpp"), "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-samples", type=int, default=8)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--no-frames", action="store_true", help="the kernels only: no child program")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def alternated(a, b):
        x, y = [], []
        for _ in range(args.warmup + args.reps):
            x.append(event_ms(a))
            y.append(event_ms(b))
        return spread(x[args.warmup:]), spread(y[args.warmup:])

    def times_rows():
        n, ns = args.width * args.height, args.ao_samples
        d_tab, d_t, d_s = up(scenes.pixel_table(args.width, args.height)), torch.zeros(n, dtype=torch.float32, device="cuda:0"), \
            torch.zeros(n * ns, dtype=torch.float32, device="cuda:0")
        p, s = step("times", args.limit, lambda: alternated(
            lambda: nt.ray_times_primary(n, d_tab.data_ptr(), 1, 0.0, 1.0, d_t.data_ptr(), stream),
            lambda: nt.ray_times_secondary(d_t.data_ptr(), 0, n, ns, d_s.data_ptr(), stream)))
        emit({"part": "times", "primary_rays": n, "secondary_rays": n * ns, "ray_times_primary_ms": p, "ray_times_secondary_ms": s,
              "primary_gb_per_s": 8e-6 * n / p["median"], "secondary_gb_per_s": 4e-6 * (n + n * ns) / s["median"]})

    def frame(name, t, tf, cam, tmp, exe):
        b, r = t.blas, t.res
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        d_rays, d_res, d_ids = up(rays), torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0"), torch.zeros(4 * n, dtype=torch.uint8, device="cuda:0")
        d_out, d_nrm, d_mout, d_mnrm = (torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0") for _ in range(4))
        d_times = up(np.random.default_rng(11).random(n).astype(F))
        d_keys = torch.zeros(128 * t.n, dtype=torch.uint8, device="cuda:0")
        blas = np.zeros(t.n, np.int32)
        inst0, tf1 = nt.make_instances(tf, blas), key1(tf)
        d_inst1 = up(inst0)
        motion = nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, d_times.data_ptr(), 0.0)
        geom = t.geometry()
        for part, k1 in (("static", inst0), ("moving", nt.make_instances(tf1, blas))):
            d_inst1.copy_(up(k1))

            def records():
                rr = nt.tlas_motion_refit(t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb,
                                          t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, r.rootLink, t.d_rec.data_ptr(), 64 * t.n,
                                          d_keys.data_ptr(), 128 * t.n, 0, stream, True)
                nt.trace_instanced_motion(*t.args(n, False, d_rays, d_res, d_ids), vis=None, motion=motion, stream=stream)
                return rr
            rr = step("%s %s refit and trace" % (name, part), args.limit, records)

            def plain():
                nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), geom, d_out.data_ptr(), d_nrm.data_ptr(), stream)

            def at_time():
                nt.instanced_hit_attributes_motion(n, d_res.data_ptr(), d_ids.data_ptr(), geom, motion, d_mout.data_ptr(), d_mnrm.data_ptr(), stream)
            p, m = step("%s %s attributes" % (name, part), args.limit, lambda: alternated(plain, at_time))
            torch.cuda.synchronize()
            hits = nt.count_hits(d_out.data_ptr(), n, stream)
            assert torch.equal(d_out, d_mout), "%s %s: the resolved records differ" % (name, part)
            same = bool(torch.equal(d_nrm, d_mnrm))
            assert same == (part == "static") or hits == 0, "%s %s: normals equal: %r" % (name, part, same)
            emit({"part": "attributes", "frame": name, "scene": part, "instances": t.n, "moving": int(rr.numMoving), "rays": n, "hits": hits,
                  "hit_attributes_ms": p, "hit_attributes_motion_ms": m, "motion_over_plain": m["median"] / p["median"]})
        assert nt.trace_status() == 0, "traversal stack overflow"
        if exe is None:
            return
        # the same scene for the child program: one mesh, the two keys, the camera
        d = os.path.join(tmp, name)
        os.makedirs(d)
        mesh = np.zeros(1, MESH_DTYPE)
        mesh[0] = (0, b.tri.shape[0], b.pos.min(axis=0), b.pos.max(axis=0))
        camf = np.concatenate([np.asarray(cam["eye"], F), scenes.nscreen_to_world(cam, args.width, args.height).reshape(-1), [F(cam["far"])]]).astype(F)
        for fn, a in (("tri.bin", b.tri), ("pos.bin", b.pos), ("meshes.bin", mesh), ("transforms.bin", tf.astype(F)), ("transforms1.bin", tf1.astype(F)),
                      ("blas.bin", blas), ("camera.bin", camf)):
            np.ascontiguousarray(a).tofile(os.path.join(d, fn))
        out = subprocess.run([exe, d, name, str(args.width), str(args.height), str(args.ao_samples), str(args.reps), str(args.warmup)],
                             capture_output=True, text=True, timeout=args.limit * 3)
        assert out.returncode == 0, out.stdout + out.stderr
        row = json.loads(out.stdout.strip().splitlines()[-1])
        row["on_over_off"] = row["on_wall_ms"]["median"] / row["off_wall_ms"]["median"]
        emit(row)

    with tempfile.TemporaryDirectory() as tmp:
        exe = None if args.no_frames else build_host_program(tmp)
        times_rows()
        tri, pos, cam = scenes.atrium()
        atrium = step("atrium BLAS", args.limit, lambda: Blas(tri, pos, stream))
        tf = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
        frame("identity", step("identity tlas", args.limit, lambda: Tlas(atrium, tf, stream)), tf, cam, tmp, exe)
        del atrium

        tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
        soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))
        rng = np.random.default_rng(4096)
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        tf = transforms(rotations(4096, rng), (g - 7.5) * 30.0)
        cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
        frame("forest", step("forest tlas", args.limit, lambda: Tlas(soup, tf, stream)), tf, cam, tmp, exe)

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
