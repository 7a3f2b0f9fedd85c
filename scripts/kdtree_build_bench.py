#!/usr/bin/env python3
"""The on-device kd-tree build (ntr_kdtree_device_build) against the host SAH kd-tree: build times, tree statistics and trace rates.

For each scene: the device build's time (GPU events and the call's wall clock, median of --reps builds after --warmup builds), its
duplicate percentage, depth and node counts; the host SAH kd-tree's build time beside it (skipped with --no-host, and by default for
scenes above --host-max triangles); and ntr_trace_kdtree Mrays/s of both trees on the same rays -- a 1920x1080 primary batch and the
8 x AO batch made from the BVH's primary hits (ntr_raygen_ao, radius 5 as bench.py).  Prints one JSON line per scene.

    python scripts/kdtree_build_bench.py [--scenes atrium conference_room hairball_1m hairball] [--reps 5] [--warmup 2] [--out f.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def rate(fn, n, reps, warmup):
    for _ in range(warmup):
        fn()
    total = 0.0
    for _ in range(reps):
        total += fn()
    return n * reps / total / 1e6


SCENES = {"atrium": scenes.atrium, "conference_room": scenes.conference_room, "hairball_1m": lambda: scenes.hairball(1_000_000),
          "hairball": scenes.hairball}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--host-max", type=int, default=400_000, help="largest scene for the host SAH kd-tree (seconds per build)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in args.scenes:
        tri, pos, cam = SCENES[name]()
        d_tri, d_pos = up(tri), up(pos)
        for _ in range(args.warmup):
            nt.kdtree_device_build(d_tri.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0]).close()
        runs = []
        for _ in range(args.reps):
            t = nt.kdtree_device_build(d_tri.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0])
            runs.append((t.seconds, t.prepMs, t.levelsMs, t.emitMs))
            t.close()
        runs = np.array(runs)
        dev = nt.kdtree_device_build(d_tri.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0])
        info = dev.info
        row = {"scene": name, "tris": int(tri.shape[0]),
               "device_build": {"wall_ms_median": float(np.median(runs[:, 0]) * 1e3), "prep_ms": float(np.median(runs[:, 1])),
                                "levels_ms": float(np.median(runs[:, 2])), "emit_ms": float(np.median(runs[:, 3])),
                                **{k: info[k] for k in ("numInnerNodes", "numLeafNodes", "numEmptyLeaves", "numTriRefs", "maxDepth",
                                                        "numLevels", "percentDuplicates")}}}
        host = None
        if not args.no_host and tri.shape[0] <= args.host_max:
            t0 = time.time()
            host = nt.kdtree_build(tri, pos, "SAHKDTree")
            row["host_sah_build"] = {"s": time.time() - t0, **{k: host.info[k] for k in ("numInnerNodes", "numLeafNodes", "numTriRefs",
                                                                                         "maxDepth", "percentDuplicates")}}
        # rays: primary, then 8 x AO from the BVH's primary hits
        bvh = nt.sah_build(tri, pos) if tri.shape[0] <= args.host_max else None
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        dev.trace(n, False, d_rays.data_ptr(), d_res.data_ptr(), stream)
        if bvh is not None:
            d_bn, d_bw, d_bi = up(bvh.nodes), up(bvh.woop), up(bvh.tri_index)
            view = nt.BvhView(d_bn.data_ptr(), bvh.nodes.nbytes, d_bw.data_ptr(), bvh.woop.nbytes, d_bi.data_ptr())
            view.validate()
            view.trace("fermi_speculative_while_while", n, False, d_rays.data_ptr(), d_res.data_ptr(), stream)
        ns = args.samples
        d_nrm = up(scenes.tri_normals(tri, pos))
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                     5.0, 0xFFF2D5E4, stream)
        torch.cuda.synchronize()
        n_ao = n * ns
        d_ao_res = torch.zeros(n_ao * 16, dtype=torch.uint8, device="cuda:0")
        m = {"device_primary": rate(lambda: dev.trace(n, False, d_rays.data_ptr(), d_res.data_ptr(), stream), n, args.reps, args.warmup),
             "device_ao": rate(lambda: dev.trace(n_ao, True, d_ao.data_ptr(), d_ao_res.data_ptr(), stream), n_ao, args.reps, args.warmup)}
        if host is not None:
            d_kn, d_kw, d_ki = up(host.nodes), up(host.woop), up(host.tri_index)
            m["host_sah_primary"] = rate(lambda: host.trace(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_kn.data_ptr(), d_kw.data_ptr(),
                                                            d_ki.data_ptr(), stream), n, args.reps, args.warmup)
            m["host_sah_ao"] = rate(lambda: host.trace(n_ao, True, d_ao.data_ptr(), d_ao_res.data_ptr(), d_kn.data_ptr(), d_kw.data_ptr(),
                                                       d_ki.data_ptr(), stream), n_ao, args.reps, args.warmup)
            m["device_over_host"] = {"primary": m["device_primary"] / m["host_sah_primary"], "ao": m["device_ao"] / m["host_sah_ao"]}
        row["mrays_s"] = m
        row["ao_rays_from"] = "bvh" if bvh is not None else "device kd-tree"
        dev.close()
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
