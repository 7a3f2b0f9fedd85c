#!/usr/bin/env python
"""What deformation motion blur costs (ntr_bvh_motion_refit, ntr_trace_bvh_motion) on the 262 k atrium: the 1920 x 1080
primary batch (closest hit) and 2^20 host-made AO rays (any hit), key 1 = key 0 deformed by pos + a d sin(k pos.yzx + phase) at
amplitude 0.02 (tests/np_bvh_refit.py's deform), the tree the host SAH tree refitted to both keys.
  * time0    every ray at time 0 (a times array of zeros): the motion launch against ntr_trace_bvh over the key-0 tree.  The records
             must be equal -- the price of the second key's fetches and of rebuilding the Woop rows per test, with nothing moving the rays
  * hashed   a hashed time per ray (ntr_ray_times_primary over the shutter [0, 1]): the motion launch against the same static launch,
             with the motion launch's counters and algorithmic bytes
  * refit    ntr_bvh_motion_refit against ONE ntr_bvh_refit, both asynchronous, by stream events
Launches are alternated (static, motion, static, motion, ...), five runs after two warm-ups; every figure is the median with its
minimum and maximum.  One JSON line per row; --out writes them as a list.  Every GPU step runs under a time limit of its own.

    timeout -k 10 600 python scripts/bvh_motion_bench.py --out bvh_motion.json
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
from bvh_refit_bench import deform  # noqa: E402
from instanced_bench import host_ao_rays, step, up  # noqa: E402

F = np.float32
KERNEL = "fermi_speculative_while_while"


def spread(v, scale=1.0):
    return {"median": float(np.median(v)) * scale, "min": float(min(v)) * scale, "max": float(max(v)) * scale}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-rays", type=int, default=1 << 20)
    ap.add_argument("--amplitude", type=float, default=0.02)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    tri, pos0, cam = scenes.atrium()
    tri, pos0 = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos0, F)
    pos1 = deform(pos0, args.amplitude)
    h = nt.sah_build(tri, pos0)
    nb, wb, ib = h.nodes.nbytes, h.woop.nbytes, h.tri_index.nbytes
    d_nodes0, d_woop, d_idx, d_tri, d_pos0, d_pos1 = step("uploads", args.limit, lambda: [up(a) for a in (h.nodes, h.woop, h.tri_index, tri, pos0, pos1)])
    d_nodes1, d_v0, d_v1 = (torch.empty(b, dtype=torch.uint8, device="cuda:0") for b in (nb, wb, wb))
    # the static side: a copy of the tree refitted to key 0 by ntr_bvh_refit itself
    d_snodes, d_swoop = d_nodes0.clone(), d_woop.clone()

    def motion_refit(blocking):
        return nt.bvh_motion_refit(d_nodes0.data_ptr(), nb, d_nodes1.data_ptr(), d_woop.data_ptr(), wb, d_idx.data_ptr(), ib, d_v0.data_ptr(),
                                   d_v1.data_ptr(), tri.shape[0], d_tri.data_ptr(), pos0.shape[0], d_pos0.data_ptr(), d_pos1.data_ptr(), 0.0, 0,
                                   stream, blocking)

    def static_refit(blocking):
        return nt.bvh_refit(d_snodes.data_ptr(), nb, d_swoop.data_ptr(), wb, d_idx.data_ptr(), ib, tri.shape[0], d_tri.data_ptr(), pos0.shape[0],
                            d_pos0.data_ptr(), 0.0, 0, stream, blocking)

    rr = step("motion refit", args.limit, lambda: motion_refit(True))
    step("static refit", args.limit, lambda: static_refit(True))
    flags = step("validate", args.limit, lambda: nt.bvh_validate(d_snodes.data_ptr(), nb))

    rays, _ = scenes.primary_rays(cam, args.width, args.height)
    n, na = rays.shape[0], args.ao_rays
    d_rays = up(rays)
    d_res, d_mres = (torch.zeros(max(n, na) * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    d_times = torch.zeros(max(n, na), dtype=torch.float32, device="cuda:0")

    def static_trace(count, any_hit, d_r):
        return nt.trace_bvh(KERNEL, count, any_hit, d_r.data_ptr(), d_res.data_ptr(), d_snodes.data_ptr(), nb, d_swoop.data_ptr(), wb,
                            d_idx.data_ptr(), bvh_flags=flags, stream=stream)

    def motion_args(count, any_hit, d_r):
        return (count, any_hit, d_r.data_ptr(), d_mres.data_ptr(), d_nodes0.data_ptr(), nb, wb, d_idx.data_ptr(),
                nt.BvhMotion(d_nodes1.data_ptr(), d_v0.data_ptr(), d_v1.data_ptr(), d_times.data_ptr(), 0.0), stream)

    def first_primary():
        static_trace(n, False, d_rays)
        torch.cuda.synchronize()
        return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
    res = step("primary for the ao rays", args.limit, first_primary)
    d_ao = step("ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

    def batch(what, count, any_hit, d_r, equal):
        def check():                                          # records (where no ray moves in time) and counters, before anything is timed
            static_trace(count, any_hit, d_r)
            st = nt.trace_bvh_motion_stats(*motion_args(count, any_hit, d_r))
            torch.cuda.synchronize()
            if equal and not any_hit:
                assert torch.equal(d_res[:16 * count], d_mres[:16 * count]), "%s: the motion launch's records differ from the static launch's" % what
            elif equal:   # any hit: which hit ends a ray depends on the static launch's route; whether there is one does not
                a, m = d_res[:16 * count].view(torch.int32)[0::4], d_mres[:16 * count].view(torch.int32)[0::4]
                assert torch.equal(a >= 0, m >= 0), "%s: the motion launch's hits differ from the static launch's" % what
            return st
        st = step(what + " records and counters", args.limit, check)

        def run():
            a, m = [], []
            for _ in range(args.warmup + args.reps):          # alternated: static, motion, static, motion, ...
                a.append(static_trace(count, any_hit, d_r))
                m.append(nt.trace_bvh_motion(*motion_args(count, any_hit, d_r)))
            return a[args.warmup:], m[args.warmup:]
        a, m = step(what, args.limit, run)
        c = dict(numInnerVisits=int(st.numInnerVisits), numTriTests=int(st.numTriTests), numLeafVisits=int(st.numLeafVisits), numHits=int(st.numHits))
        out = {"rays": count, "static_ms": spread(a, 1e3), "motion_ms": spread(m, 1e3), "motion_counters": c,
               "motion_algorithmic_bytes": 128 * c["numInnerVisits"] + 96 * c["numTriTests"] + 16 * c["numLeafVisits"] + 52 * count}
        out["static_mrays"] = count / out["static_ms"]["median"] / 1e3
        out["motion_mrays"] = count / out["motion_ms"]["median"] / 1e3
        out["motion_over_static"] = out["motion_ms"]["median"] / out["static_ms"]["median"]
        return out

    for part in ("time0", "hashed"):
        if part == "hashed":
            step("ray times", args.limit, lambda: (nt.ray_times_primary(max(n, na), 0, 11, 0.0, 1.0, d_times.data_ptr(), stream), torch.cuda.synchronize()))
        row = {"part": part, "scene": "atrium", "triangles": int(tri.shape[0]), "nodes": int(rr.numNodes), "amplitude": args.amplitude}
        row["primary"] = batch(part + " primary", n, False, d_rays, part == "time0")
        row["ao"] = batch(part + " ao", na, True, d_ao, part == "time0")
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
        for _ in range(args.warmup + args.reps):              # alternated: plain, motion, plain, motion, ...
            p.append(timed(lambda: static_refit(False)))
            m.append(timed(lambda: motion_refit(False)))
        return p[args.warmup:], m[args.warmup:]
    p, m = step("refits", args.limit, refits)
    row = {"part": "refit", "scene": "atrium", "bvh_refit_ms": spread(p), "bvh_motion_refit_ms": spread(m),
           "scratch_bytes": nt.bvh_motion_refit_scratch_bytes()}
    row["motion_over_plain"] = row["bvh_motion_refit_ms"]["median"] / row["bvh_refit_ms"]["median"]
    emit(row)
    assert nt.trace_status() == 0, "traversal stack overflow"

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
