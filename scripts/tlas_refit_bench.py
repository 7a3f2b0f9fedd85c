#!/usr/bin/env python3
"""The top-level refit (ntr_tlas_refit) against the only other way to bring a TLAS to moved instances: ntr_tlas_build.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  Every figure is the median of --reps runs after --warmup runs, with the minimum and
maximum beside it, taken by stream events:
  * cost      ntr_tlas_refit with result = NULL (asynchronous: two launches) over 1 025 and 65 536 instances of soup1000
              (scripts/instanced_bench.py's sets), after every instance got a new seeded transform; beside it ntr_tlas_build of the same
              instances in the same run (events around the blocking call, and the call's own wall clock), and the ratio
  * quality   the 4 096-instance forest of scripts/instanced_bench.py (a 16 x 16 x 16 grid, spacing 30): the instances are translated by
              seeded offsets of 1 %, 10 % and 100 % of the spacing; a 1920x1080 primary batch and one 2^20-ray AO batch are traced
              through the REFITTED tree (the tree of the unmoved grid, refitted) and through a tree REBUILT over the moved instances.
              The records of the two primary batches are compared.  frame_refit_ms / frame_rebuild_ms add the update's own cost, so
              the amplitude at which the second falls below the first is where a rebuild pays for itself within one frame
Prints one JSON line per row.

    timeout -k 10 600 python scripts/tlas_refit_bench.py --out tlas_refit.json
"""
import argparse
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

from instanced_bench import Blas, Tlas, host_ao_rays, rotations, transforms, up  # noqa: E402

F = np.float32
SPACING = 30.0


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("tlas_refit_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
        sys.stderr.flush()
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def refit(t, blocking=False):
    b = t.blas
    return nt.tlas_refit(t.n, t.d_inst.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb, t.d_nodes.data_ptr(), t.res.nodesBytes, t.res.rootLink,
                         t.d_rec.data_ptr(), t.caps[1], 0, t.stream, blocking)


def set_transforms(t, tf):
    t.d_inst.copy_(up(nt.make_instances(tf, np.zeros(tf.shape[0], np.int32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["cost", "quality"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-rays", type=int, default=1 << 20)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def measure(fn):
        return [event_ms(fn) for _ in range(args.warmup + args.reps)][args.warmup:]

    tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
    soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))

    if "cost" in args.parts:
        for n in (1025, 65536):
            def placed(seed):
                rng = np.random.default_rng(seed)
                return transforms(rotations(n, rng), rng.uniform(-25.0, 25.0, (n, 3)) * (n / 1025.0) ** (1.0 / 3.0))

            def run():
                t = Tlas(soup, placed(n), stream)
                set_transforms(t, placed(n + 1))
                refit_ms = measure(lambda: refit(t))
                res = refit(t, blocking=True)
                refitted = t.d_nodes.clone()
                walls = []

                def build():
                    walls.append(t.build().seconds * 1e3)
                build_ms = measure(build)
                return {"part": "cost", "instances": n, "refit_ms": stats(refit_ms), "refit_blocking_gpu_ms": res.seconds * 1e3,
                        "build_ms": stats(build_ms), "build_wall_ms": stats(walls[args.warmup:]),
                        "ratio_build_over_refit": float(np.median(build_ms) / np.median(refit_ms)), "numNodes": res.numNodes,
                        "boxes_changed": not bool(torch.equal(refitted, t.d_nodes)), "scratch_bytes": nt.tlas_refit_scratch_bytes()}
            emit(step("cost %d" % n, args.limit, run))

    if "quality" in args.parts:
        rng = np.random.default_rng(4096)
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        rot, home = rotations(4096, rng), (g - 7.5) * SPACING
        cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res, d_ids = (torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4))

        def traced(t, count, any_hit, d_r):
            secs = [t.trace(count, any_hit, d_r, d_res, d_ids) * 1e3 for _ in range(args.warmup + args.reps)][args.warmup:]
            return stats(secs)

        for amp in (0.01, 0.1, 1.0):
            offs = np.random.default_rng(int(amp * 1000)).uniform(-1.0, 1.0, (4096, 3)) * amp * SPACING
            moved = transforms(rot, home + offs)

            def run():
                # the refitted tree: the unmoved grid's topology
                r = Tlas(soup, transforms(rot, home), stream)
                set_transforms(r, moved)
                refit_ms = measure(lambda: refit(r))
                b = Tlas(soup, moved, stream)
                build_ms = measure(b.build)
                row = {"part": "quality", "instances": 4096, "amplitude": amp, "refit_ms": stats(refit_ms), "build_ms": stats(build_ms),
                       "height_refitted": r.res.height, "height_rebuilt": b.res.height}
                row["primary_rebuilt_ms"] = traced(b, n, False, d_rays)
                torch.cuda.synchronize()
                res = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
                row["primary_refitted_ms"] = traced(r, n, False, d_rays)
                torch.cuda.synchronize()
                same = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE)
                row["primary_hits"] = int((res["id"] >= 0).sum())
                row["primary_t_equal"] = bool(same["t"].tobytes() == res["t"].tobytes())
                d_ao = up(host_ao_rays(rays, res, na, 7))
                row["ao_rebuilt_ms"] = traced(b, na, True, d_ao)
                row["ao_refitted_ms"] = traced(r, na, True, d_ao)
                row["frame_refit_ms"] = row["refit_ms"]["median"] + row["primary_refitted_ms"]["median"] + row["ao_refitted_ms"]["median"]
                row["frame_rebuild_ms"] = row["build_ms"]["median"] + row["primary_rebuilt_ms"]["median"] + row["ao_rebuilt_ms"]["median"]
                assert nt.trace_status() == 0, "traversal stack overflow"
                return row
            emit(step("quality %g" % amp, args.limit, run))

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
