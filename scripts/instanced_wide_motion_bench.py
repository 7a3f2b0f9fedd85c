#!/usr/bin/env python
"""What motion blur costs over the 4-wide trees (ntr_trace_instanced_wide_motion, ntr_tlas_wide_motion_refit), by the
protocol of scripts/instanced_motion_bench.py and over its two frames: the 1920 x 1080 primary batch (closest hit) and 2^20 host-made AO
rays (any hit) through ONE identity instance of atrium() and through the forest of 4 096 instances of soup1000.
  * static    nothing moves (key 1 == key 0, so no record carries the moving flag) but a times array is given
  * moving    every instance moves (instanced_motion_bench.key1) and every ray has a random time in [0, 1)
  in both parts three launches over buffers refitted to the same two keys, alternated: the wide masked launch (the scene frozen at key
  0 inside the swept boxes), the wide motion launch, and the binary motion launch.  Where nothing moves the wide motion records must
  equal the wide masked ones.
  * refit     ntr_tlas_wide_motion_refit against ntr_tlas_wide_refit, both asynchronous (two launches each), by stream events
All launches get the same visibility, a ray mask of 0x7FFFFFFF that refuses nothing, so that the wide entry point launches its masked
kernel.  Five runs after two warm-ups; every figure is the median with its minimum and maximum.  One JSON line per row; --out writes them
as a list.  Every GPU step runs under a time limit of its own.

    timeout -k 10 600 python scripts/instanced_wide_motion_bench.py --out instanced_wide_motion.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from instanced_bench import Blas, Tlas, host_ao_rays, rotations, step, transforms, up  # noqa: E402
from instanced_motion_bench import key1, spread  # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
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

    def frame(name, t, tf, cam):
        b, r = t.blas, t.res
        step(name + " widen", args.limit, lambda: t.widen())
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = step(name + " rays", args.limit, lambda: up(rays))
        d_res, d_ids, d_wres, d_wids, d_bres, d_bids = step(name + " buffers", args.limit, lambda: [
            torch.zeros(max(n, na) * w, dtype=torch.uint8, device="cuda:0") for w in (16, 4, 16, 4, 16, 4)])
        d_times = up(np.random.default_rng(11).random(max(n, na)).astype(F))
        d_keys = torch.zeros(128 * t.n, dtype=torch.uint8, device="cuda:0")
        inst0 = nt.make_instances(tf, np.zeros(t.n, np.int32))
        inst1 = nt.make_instances(key1(tf), np.zeros(t.n, np.int32))
        d_inst1 = up(inst0)
        motion = nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, d_times.data_ptr(), 0.0)
        vis = nt.InstanceVisibility(0, 0, 0x7FFFFFFF)         # refuses nothing, and selects the masked loop
        wnb = t.wtlas_res.nodesBytes

        def wide_refit_args():
            return (b.ranges, t.wide_ranges, t.d_wpool.data_ptr(), t.wpool_res.nodesBytes, t.d_wtlas.data_ptr() if wnb else 0, wnb, r.rootLink,
                    t.d_wrec.data_ptr(), 64 * t.n)

        def wide_motion_refit(blocking):
            return nt.tlas_wide_motion_refit(t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), *wide_refit_args(), d_keys.data_ptr(), 128 * t.n, 0,
                                             stream, blocking)

        def wide_plain_refit():
            nt.tlas_wide_refit(t.n, t.d_inst.data_ptr(), *wide_refit_args(), 0, stream, False)

        def binary_motion_refit():
            return nt.tlas_motion_refit(t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb,
                                        t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, r.rootLink, t.d_rec.data_ptr(), 64 * t.n,
                                        d_keys.data_ptr(), 128 * t.n, 0, stream, True)

        def first_primary():
            t.trace(n, False, d_rays, d_res, d_ids)
            torch.cuda.synchronize()
            return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        res = step(name + " primary for the ao rays", args.limit, first_primary)
        d_ao = step(name + " ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

        def batch(what, count, any_hit, d_r, equal):
            def check():                                      # records (where nothing moves) and counters, before anything is timed
                st = nt.trace_instanced_wide_stats(*t.wide_args(count, any_hit, d_r, d_res, d_ids), vis=vis, stream=stream)
                mst, mm = nt.trace_instanced_wide_motion_stats(*t.wide_args(count, any_hit, d_r, d_wres, d_wids), vis=vis, motion=motion,
                                                               stream=stream)
                torch.cuda.synchronize()
                if equal:
                    assert torch.equal(d_res[:16 * count], d_wres[:16 * count]) and torch.equal(d_ids[:4 * count], d_wids[:4 * count]), \
                        "%s %s: the wide motion launch's records differ from the wide masked launch's" % (name, what)
                    assert st.as_dict() == mst.as_dict() and mm.as_dict() == dict(numMovingEntries=0, numSingular=0)
                return st, mst, mm
            st, mst, mm = step("%s %s records and counters" % (name, what), args.limit, check)

            def run():
                a, w, m = [], [], []
                for _ in range(args.warmup + args.reps):      # alternated: wide masked, wide motion, binary motion, ...
                    a.append(nt.trace_instanced_wide(*t.wide_args(count, any_hit, d_r, d_res, d_ids), vis=vis, stream=stream))
                    w.append(nt.trace_instanced_wide_motion(*t.wide_args(count, any_hit, d_r, d_wres, d_wids), vis=vis, motion=motion, stream=stream))
                    m.append(nt.trace_instanced_motion(*t.args(count, any_hit, d_r, d_bres, d_bids), vis=vis, motion=motion, stream=stream))
                return a[args.warmup:], w[args.warmup:], m[args.warmup:]
            a, w, m = step("%s %s" % (name, what), args.limit, run)
            out = {"rays": count, "wide_masked_ms": spread(a, 1e3), "wide_motion_ms": spread(w, 1e3), "binary_motion_ms": spread(m, 1e3),
                   "wide_masked_counters": st.as_dict(), "wide_motion_counters": dict(mst.as_dict(), **mm.as_dict()),
                   "wide_motion_algorithmic_bytes": int(mm.algorithmic_bytes(mst, ray_times=True))}
            out["wide_motion_over_wide_masked"] = out["wide_motion_ms"]["median"] / out["wide_masked_ms"]["median"]
            out["wide_motion_over_binary_motion"] = out["wide_motion_ms"]["median"] / out["binary_motion_ms"]["median"]
            out["entries_per_ray"] = mst.numInstanceEntries / count
            out["moving_entries_per_ray"] = mm.numMovingEntries / count
            return out

        for part, k1 in (("static", inst0), ("moving", inst1)):
            d_inst1.copy_(up(k1))
            step("%s %s binary motion refit" % (name, part), args.limit, binary_motion_refit)
            rr = step("%s %s wide motion refit" % (name, part), args.limit, lambda: wide_motion_refit(True))
            row = {"part": part, "frame": name, "instances": t.n, "moving": int(rr.numMoving)}
            row["primary"] = batch(part + " primary", n, False, d_rays, part == "static")
            row["ao"] = batch(part + " ao", na, True, d_ao, part == "static")
            emit(row)

        def refits():
            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            p, m = [], []
            for _ in range(args.warmup + args.reps):          # alternated: plain, motion, plain, motion, ...
                p.append(timed(wide_plain_refit))
                m.append(timed(lambda: wide_motion_refit(False)))
            return p[args.warmup:], m[args.warmup:]
        p, m = step(name + " refits", args.limit, refits)
        row = {"part": "refit", "frame": name, "instances": t.n, "tlas_wide_refit_ms": spread(p), "tlas_wide_motion_refit_ms": spread(m),
               "scratch_bytes": nt.tlas_wide_motion_refit_scratch_bytes()}
        row["motion_over_plain"] = row["tlas_wide_motion_refit_ms"]["median"] / row["tlas_wide_refit_ms"]["median"]
        emit(row)
        assert nt.trace_status() == 0, "traversal stack overflow"

    tri, pos, cam = scenes.atrium()
    atrium = step("atrium BLAS", args.limit, lambda: Blas(tri, pos, stream))
    tf = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
    frame("identity", step("identity tlas", args.limit, lambda: Tlas(atrium, tf, stream)), tf, cam)

    tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
    soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))
    rng = np.random.default_rng(4096)
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    tf = transforms(rotations(4096, rng), (g - 7.5) * 30.0)
    cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
    frame("forest", step("forest tlas", args.limit, lambda: Tlas(soup, tf, stream)), tf, cam)

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
