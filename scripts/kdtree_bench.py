#!/usr/bin/env python3
"""kd-tree against BVH on the device, with the reference's protocol: rays / sum of kernel times, after warm-up launches.

For each scene (atrium(), conference_room()): SAH kd-tree (ntr_trace_kdtree) and SAH BVH (ntr_trace_bvh, per-ray kernel
fermi_speculative_while_while) on a 1920x1080 primary batch and on the 8 x AO batch generated from the BVH's primary hits
(ntr_raygen_ao, radius 5 as bench.py), both structures tracing the same rays; plus the build times and statistics of the SAH and
spatial-median kd-trees.  Prints one JSON line per scene (and the whole list with --out).

    python scripts/kdtree_bench.py [--scenes atrium conference_room] [--reps 10] [--warmup 3] [--out file.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["atrium", "conference_room"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--ao-radius", type=float, default=5.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in args.scenes:
        tri, pos, cam = getattr(scenes, name)()
        t0 = time.time()
        sah = nt.kdtree_build(tri, pos, "SAHKDTree")
        t_sah = time.time() - t0
        t0 = time.time()
        med = nt.kdtree_build(tri, pos, "SpatialMedianKDTree")
        t_med = time.time() - t0
        bvh = nt.sah_build(tri, pos)
        d_kn, d_kw, d_ki = up(sah.nodes), up(sah.woop), up(sah.tri_index)
        d_bn, d_bw, d_bi = up(bvh.nodes), up(bvh.woop), up(bvh.tri_index)
        view = nt.BvhView(d_bn.data_ptr(), bvh.nodes.nbytes, d_bw.data_ptr(), bvh.woop.nbytes, d_bi.data_ptr())
        view.validate()

        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        view.trace("fermi_speculative_while_while", n, False, d_rays.data_ptr(), d_res.data_ptr(), stream)
        # AO batch from the BVH's primary hits; every input ray gets `samples` slots
        ns = args.samples
        d_nrm = up(scenes.tri_normals(tri, pos))
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                     args.ao_radius, 0xFFF2D5E4, stream)
        torch.cuda.synchronize()
        n_ao = n * ns
        d_ao_res = torch.zeros(n_ao * 16, dtype=torch.uint8, device="cuda:0")

        def kd(dr, dres, cnt, any_hit):
            return lambda: sah.trace(cnt, any_hit, dr.data_ptr(), dres.data_ptr(), d_kn.data_ptr(), d_kw.data_ptr(), d_ki.data_ptr(), stream)

        def bv(dr, dres, cnt, any_hit):
            return lambda: view.trace("fermi_speculative_while_while", cnt, any_hit, dr.data_ptr(), dres.data_ptr(), stream)

        row = {
            "scene": name, "tris": int(tri.shape[0]), "primary_rays": n, "ao_rays": n_ao,
            "mrays_s": {
                "kdtree_primary": rate(kd(d_rays, d_res, n, False), n, args.reps, args.warmup),
                "bvh_primary": rate(bv(d_rays, d_res, n, False), n, args.reps, args.warmup),
                "kdtree_ao": rate(kd(d_ao, d_ao_res, n_ao, True), n_ao, args.reps, args.warmup),
                "bvh_ao": rate(bv(d_ao, d_ao_res, n_ao, True), n_ao, args.reps, args.warmup),
            },
            "build": {
                "sah_kdtree_s": t_sah, "spatial_median_kdtree_s": t_med, "sah_kdtree": sah.info, "spatial_median_kdtree": med.info,
                "sah_bvh_s": bvh.info.get("buildSeconds"),
            },
        }
        m = row["mrays_s"]
        row["kdtree_over_bvh"] = {"primary": m["kdtree_primary"] / m["bvh_primary"], "ao": m["kdtree_ao"] / m["bvh_ao"]}
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
