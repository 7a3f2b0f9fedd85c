#!/usr/bin/env python3
"""The on-device PLOC build (ntr_ploc_build): what it costs, and what its tree is worth in SAH cost and in trace rate, beside the
other device builds of the same mesh.

For each scene, everything of a row in one process and over the same rays:
  * build time: ntr_ploc_build at --radius, the median of --reps calls after --warmup calls, wall clock of the blocking call and the
    result's phases (vertex check, codes + sort, leaves, rounds before the tail, tail), with the rounds and the list length at the
    hand-over; beside ntr_lbvh_build, ntr_lbvh_build + two ntr_bvh_optimize passes, ntr_hlbvh_build (bits 4) and the binned build
    (ntr_persistent_bvh_build), each timed the same way (the seconds its blocking call reports);
  * quality: SAH cost (ntr_bvh_sah_cost), height and ntr_trace_bvh Mrays/s with freshly validated flags for PLOC, PLOC + two optimise
    passes, LBVH, LBVH + 2, HLBVH (bits 4) and the binned tree, with the PLOC tree a second time at the end as the run-to-run spread, on
    a 1920x1080 primary batch and the 8 x AO batch made from the LBVH's primary hits (ntr_raygen_ao, radius 5 as bench.py).  A rate is
    the rays over the sum of the kernel times of --reps launches after --warmup launches.
Prints one JSON line per scene.  One scene per process keeps a run short; on a shared GPU box give every process its own time limit
and chain them:

    timeout -k 10 300 python scripts/bvh_ploc_bench.py --scenes atrium --out a.json && \\
    timeout -k 10 300 python scripts/bvh_ploc_bench.py --scenes conference_room --out c.json && \\
    timeout -k 10 300 python scripts/bvh_ploc_bench.py --scenes hairball --out h.json

--once makes one PLOC build and nothing else: the workload of a kernel-trace profile.
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

from bvh_optimize_bench import SCENES, Tree, rate, up  # noqa: E402

F = np.float32
PHASES = ("mortonMs", "sortMs", "emitMs", "roundsMs", "tailMs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--kernel", default="fermi_speculative_while_while")
    ap.add_argument("--once", action="store_true", help="one PLOC build, nothing else (the workload of a kernel-trace profile)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in args.scenes:
        tri, pos, cam = SCENES[name]()
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        n_tri, n_vert = tri.shape[0], pos.shape[0]
        d_tri, d_pos = up(tri), up(pos)
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        capn, capw, capi = nt.lbvh_capacity(n_tri)
        row = {"scene": name, "tris": int(n_tri), "radius": args.radius}

        def build(kind):
            """(Tree, the call's result) of one build into fresh buffers."""
            bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
            ptrs = (bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw, bufs[2].data_ptr(), capi)
            geo = (n_tri, d_tri.data_ptr(), n_vert, d_pos.data_ptr(), mn, mx)
            if kind == "ploc":
                r = nt.ploc_build(*geo, *ptrs, args.radius, stream)
            elif kind == "lbvh":
                r = nt.lbvh_build(*geo, 8, 0.001, *ptrs, stream)
            elif kind == "hlbvh4":
                r = nt.hlbvh_build(*geo, 8, 0.001, 4, *ptrs, stream).lbvh
            else:
                r = nt.persistent_bvh_build(*geo, *ptrs, None, stream)
            return Tree(bufs, r.nodesBytes, r.triWoopBytes, r.triIndexBytes), r

        if args.once:
            print(json.dumps({"scene": name, "ploc": build("ploc")[1].as_dict()}), flush=True)
            continue

        def timed(kind, passes=0):
            """Medians of the build's milliseconds (and of the PLOC phases); `passes` optimise passes on top count into the time."""
            runs = []
            for i in range(args.warmup + args.reps):
                t, r = build(kind)
                ms = float(r.seconds) * 1e3
                if passes:
                    ms += float(t.optimize(passes, stream).seconds) * 1e3
                if i >= args.warmup:
                    runs.append((ms, r))
            out = {"ms_median": float(np.median([m for m, _ in runs]))}
            if kind == "ploc":
                out.update({p: float(np.median([getattr(r, p) for _, r in runs])) for p in PHASES})
                r = runs[-1][1]
                out.update(numRounds=r.numRounds, tailClusters=r.tailClusters, height=r.height)
            return out

        row["build"] = {"ploc": timed("ploc"), "lbvh": timed("lbvh"), "lbvh+2": timed("lbvh", 2), "hlbvh4": timed("hlbvh4"),
                        "binned": timed("binned"), "ploc+2": timed("ploc", 2)}
        row["ploc_scratch_bytes"] = nt.ploc_scratch_bytes()

        ploc, lbvh, hlbvh, binned = (build(k)[0] for k in ("ploc", "lbvh", "hlbvh4", "binned"))
        trees = {"ploc": ploc, "ploc+2": ploc.optimized(2, stream), "lbvh": lbvh, "lbvh+2": lbvh.optimized(2, stream), "hlbvh4": hlbvh,
                 "binned": binned, "ploc again": ploc}
        flags = {k: nt.bvh_validate(t.bufs[0].data_ptr(), t.nb, stream) for k, t in trees.items()}
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, ns = rays.shape[0], args.samples
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        d_ao_res = torch.zeros(n * ns * 16, dtype=torch.uint8, device="cuda:0")

        def trace(key, count, any_hit, d_r, d_out):
            t = trees[key]
            return nt.trace_bvh(args.kernel, count, any_hit, d_r.data_ptr(), d_out.data_ptr(), t.bufs[0].data_ptr(), t.nb,
                                t.bufs[1].data_ptr(), t.wb, t.bufs[2].data_ptr(), bvh_flags=flags[key], stream=stream)

        trace("lbvh", n, False, d_rays, d_res)
        d_nrm = up(scenes.tri_normals(tri, pos))
        nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns, 5.0,
                     0xFFF2D5E4, stream)
        torch.cuda.synchronize()
        row["quality"] = {}
        for key, t in trees.items():
            s = t.sah(stream)
            row["quality"][key] = {"sah": float(s.sahCost), "height": s.height,
                                   "primary": rate(lambda: trace(key, n, False, d_rays, d_res), n, args.reps, args.warmup),
                                   "ao": rate(lambda: trace(key, n * ns, True, d_ao, d_ao_res), n * ns, args.reps, args.warmup)}
        assert nt.trace_status() == 0, "traversal stack overflow"
        print(json.dumps(row), flush=True)
        results.append(row)
        nt.lbvh_release_workspace()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
