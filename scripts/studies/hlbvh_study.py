#!/usr/bin/env python3
"""LBVH against HLBVH (hlbvhBits 2, 4, 6) trees on the config 2-5 stand-ins: build ms by phase, SAH cost, trace ms of a primary,
an 8 x AO and a diffuse batch through each tree under two kernels, and mismatches against the oracle on a ray subset.

Usage: python scripts/studies/hlbvh_study.py [--scenes atrium,conference,hairball,courtyard] [--bits 2,4,6] [--check 65536]
Prints one JSON line per (scene, builder)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from oracle import oracle  # noqa: E402

KERNELS = ("fermi_speculative_while_while", "kepler_dynamic_fetch")
SCENES = {"atrium": scenes.atrium, "conference": scenes.conference_room, "hairball": scenes.hairball, "courtyard": scenes.courtyard}


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def sah_cost(nodes, woop):
    """Sum over inner nodes of (area(child 0) + area(child 1)) / area(root) plus, per leaf, triangles * area(leaf) / area(root)."""
    f = nodes.view(np.float32).reshape(-1, 16).astype(np.float64)
    ref = nodes.view(np.int32).reshape(-1, 16)[:, 12:14]

    def area(lo, hi):
        d = np.maximum(hi - lo, 0)
        return 2 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    a0 = area(f[:, [0, 2, 8]], f[:, [1, 3, 9]])
    a1 = area(f[:, [4, 6, 10]], f[:, [5, 7, 11]])
    root = area(np.minimum(f[0, [0, 2, 8]], f[0, [4, 6, 10]]), np.maximum(f[0, [1, 3, 9]], f[0, [5, 7, 11]]))
    w = woop.view(np.uint32).reshape(-1, 4)
    term = np.flatnonzero((w == 0x80000000).all(axis=1))
    cost = (a0 + a1).sum()
    for k, a in ((0, a0), (1, a1)):
        leaf = ref[:, k] < 0
        start = ~ref[leaf, k]
        ntri = (term[np.searchsorted(term, start)] - start) // 3
        cost += (ntri * a[leaf]).sum()
    return float(cost / root)


def secondary(cam_rays, res, n_per, seed, tmax):
    hit = res["id"] >= 0
    r = cam_rays[hit]
    t = res["t"][hit]
    rng = np.random.default_rng(seed)
    o = np.stack([r["ox"] + t * r["dx"], r["oy"] + t * r["dy"], r["oz"] + t * r["dz"]], axis=1).astype(np.float32)
    o = np.repeat(o, n_per, axis=0)
    d = rng.normal(size=o.shape).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros(o.shape[0], dtype=cam_rays.dtype)
    out["ox"], out["oy"], out["oz"] = o[:, 0] + 1e-3 * d[:, 0], o[:, 1] + 1e-3 * d[:, 1], o[:, 2] + 1e-3 * d[:, 2]
    out["dx"], out["dy"], out["dz"] = d[:, 0], d[:, 1], d[:, 2]
    out["tmin"] = 0.0
    out["tmax"] = tmax
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="atrium,conference,hairball,courtyard")
    ap.add_argument("--bits", default="2,4,6")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=65536, help="rays per batch compared with the oracle")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    for name in args.scenes.split(","):
        tri, pos, cam = SCENES[name]()
        n = tri.shape[0]
        d_tri, d_pos = up(tri), up(pos)
        mn, mx = oracle.scene_bbox(pos)
        capn, capw, capi = nt.lbvh_capacity(n)
        d_nodes = torch.zeros(capn, dtype=torch.uint8, device="cuda")
        d_woop = torch.zeros(capw, dtype=torch.uint8, device="cuda")
        d_idx = torch.zeros(capi, dtype=torch.uint8, device="cuda")
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        diag = float(np.linalg.norm(mx - mn))
        batches = None
        for builder in ["lbvh"] + ["hlbvh%s" % b for b in args.bits.split(",")]:
            best = None
            for _ in range(args.reps):
                if builder == "lbvh":
                    r = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, d_nodes.data_ptr(), capn,
                                      d_woop.data_ptr(), capw, d_idx.data_ptr(), capi, stream)
                    sec, info = r.seconds, r.as_dict()
                    nb, wb, ib = r.nodesBytes, r.triWoopBytes, r.triIndexBytes
                else:
                    r = nt.hlbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, int(builder[5:]),
                                       d_nodes.data_ptr(), capn, d_woop.data_ptr(), capw, d_idx.data_ptr(), capi, stream)
                    sec, info = r.lbvh.seconds, r.as_dict()
                    nb, wb, ib = r.lbvh.nodesBytes, r.lbvh.triWoopBytes, r.lbvh.triIndexBytes
                if best is None or sec < best[0]:
                    best = (sec, info)
            torch.cuda.synchronize()
            h_nodes = d_nodes[:nb].cpu().numpy()
            h_woop = d_woop[:wb].cpu().numpy()
            h_idx = d_idx[:ib].cpu().numpy().view(np.int32)
            view = nt.BvhView(d_nodes.data_ptr(), nb, d_woop.data_ptr(), wb, d_idx.data_ptr())
            view.validate(stream)
            if batches is None:   # secondary rays from the LBVH tree's primary hits, shared by every builder of this scene
                d_r = up(rays)
                d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda")
                view.trace(KERNELS[0], rays.shape[0], False, d_r.data_ptr(), d_res.data_ptr(), stream)
                prim = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
                batches = {"primary": (rays, False), "ao8": (secondary(rays, prim, 8, 1, 0.05 * diag), True),
                           "diffuse": (secondary(rays, prim, 1, 2, 1e30), False)}
            out = dict(scene=name, triangles=n, builder=builder, build_ms=best[0] * 1e3, build=best[1], sah_cost=sah_cost(h_nodes, h_woop),
                       trace_ms={}, mismatches=0)
            for bname, (rs, any_hit) in batches.items():
                d_r = up(rs)
                d_res = torch.zeros(rs.shape[0] * 16, dtype=torch.uint8, device="cuda")
                for kernel in KERNELS:
                    ts = [view.trace(kernel, rs.shape[0], any_hit, d_r.data_ptr(), d_res.data_ptr(), stream) for _ in range(4)]
                    out["trace_ms"]["%s/%s" % (bname, kernel)] = min(ts[1:]) * 1e3
                    got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)[:args.check]
                    ref, _ = oracle.trace(h_nodes, h_woop, h_idx, rs[:args.check], any_hit=any_hit, threads=16)
                    out["mismatches"] += int((got["id"] != ref["id"]).sum() + (got["t"].view(np.uint32) != ref["t"].view(np.uint32)).sum())
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
