#!/usr/bin/env python3
"""The 4-wide BVH (ntr_bvh_widen, ntr_trace_wide) beside the binary tree it was made from: what widening costs, what the wide tree looks
like, and what a batch costs through either.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung).  Every time is the median of --reps runs after --warmup runs, by stream events (the calls' own seconds).  Per scene
(atrium(), the hairball stand-in) and per tree (host SAH uploaded, ntr_lbvh_build, ntr_ploc_build):
  * widen      ntr_bvh_widen's time, the counts of 2-, 3- and 4-child nodes, height, stackBound, node bytes beside the binary tree's
  * batches    a 1920x1080 primary batch, a 2^20-ray AO batch (from the primary hits: uniform directions, length 5, any hit) and a
               2^20-ray batch of random rays through the scene's box, each through ntr_trace_wide with the binary tree's validated
               flags and with flags 0, and through ntr_trace_bvh("fermi_speculative_while_while") on the binary tree
  * counters   ntr_trace_wide_stats and ntr_trace_bvh_stats on the same rays: node fetches and triangle tests per ray
Prints one JSON line per (scene, tree).

    timeout -k 10 900 python scripts/bvh_wide_bench.py --out bvh_wide.json
"""
import argparse
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

F = np.float32
KERNEL = "fermi_speculative_while_while"


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("bvh_wide_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
        sys.stderr.flush()
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


class Tree:
    """A binary Compact tree on the device (bufs: nodes, woop, index; nb, wb: the extents) and its wide node buffer."""

    def __init__(self, kind, tri, pos, stream):
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        n = tri.shape[0]
        if kind == "sah":
            b = nt.sah_build(tri, pos)
            self.bufs = [up(b.nodes), up(b.woop), up(b.tri_index)]
            self.nb, self.wb = b.nodes.nbytes, b.woop.nbytes
        else:
            caps = nt.lbvh_capacity(n)
            self.bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps]
            d_tri, d_pos = up(tri), up(pos)
            mn, mx = pos.min(axis=0), pos.max(axis=0)
            ptrs = (self.bufs[0].data_ptr(), caps[0], self.bufs[1].data_ptr(), caps[1], self.bufs[2].data_ptr(), caps[2])
            if kind == "lbvh":
                r = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, *ptrs, stream)
            else:
                r = nt.ploc_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, *ptrs, 8, stream)
            self.nb, self.wb = r.nodesBytes, r.triWoopBytes
        self.stream = stream
        self.flags = nt.bvh_validate(self.bufs[0].data_ptr(), self.nb, stream)
        self.cap = nt.bvh_widen_capacity(self.nb)
        self.d_wide = torch.zeros(self.cap, dtype=torch.uint8, device="cuda:0")
        self.res = self.widen()

    def widen(self):
        return nt.bvh_widen(self.bufs[0].data_ptr(), self.nb, self.d_wide.data_ptr(), self.cap, self.stream)

    def _wide_args(self, count, any_hit, d_rays, d_res, flags):
        return (count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.d_wide.data_ptr(), self.res.nodesBytes, self.bufs[1].data_ptr(), self.wb,
                self.bufs[2].data_ptr(), flags, self.stream)

    def trace_wide(self, count, any_hit, d_rays, d_res, flags):
        return nt.trace_wide(*self._wide_args(count, any_hit, d_rays, d_res, flags))

    def trace_binary(self, count, any_hit, d_rays, d_res):
        return nt.trace_bvh(KERNEL, count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.bufs[0].data_ptr(), self.nb, self.bufs[1].data_ptr(),
                            self.wb, self.bufs[2].data_ptr(), bvh_flags=self.flags, stream=self.stream)

    def stats(self, count, any_hit, d_rays, d_res):
        w = nt.trace_wide_stats(*self._wide_args(count, any_hit, d_rays, d_res, self.flags))
        b = nt.trace_bvh_stats(KERNEL, count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.bufs[0].data_ptr(), self.nb,
                               self.bufs[1].data_ptr(), self.wb, self.bufs[2].data_ptr(), 4, self.flags, self.stream)
        per = lambda s: {"nodes_per_ray": s.numInnerVisits / count, "tris_per_ray": s.numTriTests / count}   # noqa: E731
        return {"wide": per(w), "binary": per(b)}


def median_rate(fn, count, reps, warmup):
    """fn() -> the launch's GPU seconds; -> dict(ms_median, mrays_per_s, ms_min, ms_max)."""
    secs = [fn() for _ in range(warmup + reps)][warmup:]
    ms = float(np.median(secs)) * 1e3
    return {"ms_median": ms, "mrays_per_s": count / ms / 1e3, "ms_min": float(min(secs)) * 1e3, "ms_max": float(max(secs)) * 1e3}


def host_ao_rays(rays, res, count, seed, radius=5.0):
    """`count` occlusion rays from the hit points of a primary batch: uniform directions, tmin 1e-3, tmax radius."""
    rng = np.random.default_rng(seed)
    hit = np.flatnonzero(res["id"] >= 0)
    pick = hit[rng.integers(0, hit.size, count)]
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros(count, nt.RAY_DTYPE)
    for k, dk, col in zip(("ox", "oy", "oz"), ("dx", "dy", "dz"), range(3)):
        out[k] = rays[k][pick] + res["t"][pick] * rays[dk][pick]
        out[dk] = d[:, col].astype(F)
    out["tmin"], out["tmax"] = F(1e-3), F(radius)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["atrium", "hairball"])
    ap.add_argument("--trees", nargs="+", default=["sah", "lbvh", "ploc"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=1 << 20, help="rays of the AO batch and of the random batch")
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for scene in args.scenes:
        tri, pos, cam = getattr(scenes, scene)()
        prim, _ = scenes.primary_rays(cam, args.width, args.height)
        rnd = scenes.box_rays(pos, args.rays, 11)
        d_prim, d_rnd = up(prim), up(rnd)
        d_res = torch.zeros(max(prim.shape[0], args.rays) * 16, dtype=torch.uint8, device="cuda:0")
        for kind in args.trees:
            what = "%s %s" % (scene, kind)
            t = step(what + " build", max(args.limit, 600), lambda: Tree(kind, tri, pos, stream))
            runs = step(what + " widen", args.limit, lambda: [t.widen() for _ in range(args.warmup + args.reps)][args.warmup:])
            r = runs[-1]
            row = {"scene": scene, "tree": kind, "tris": int(tri.shape[0]), "flags": t.flags, "binary_nodes_bytes": t.nb,
                   "widen_ms": float(np.median([x.seconds for x in runs])) * 1e3, "wide": r.as_dict(), "scratch_bytes": nt.bvh_widen_scratch_bytes()}
            row["wide"].pop("seconds")
            t.trace_binary(prim.shape[0], False, d_prim, d_res)
            torch.cuda.synchronize()
            res = d_res.cpu().numpy()[:16 * prim.shape[0]].view(nt.RESULT_DTYPE).copy()
            d_ao = up(host_ao_rays(prim, res, args.rays, 7))
            for batch, d_rays, count, any_hit in (("primary", d_prim, prim.shape[0], False), ("ao", d_ao, args.rays, True), ("random", d_rnd, args.rays, False)):
                name = what + " " + batch
                out = {"rays": count}
                out["wide_flags"] = step(name + " wide", args.limit, lambda: median_rate(lambda: t.trace_wide(count, any_hit, d_rays, d_res, t.flags), count, args.reps, args.warmup))
                out["wide_flags0"] = step(name + " wide flags 0", args.limit, lambda: median_rate(lambda: t.trace_wide(count, any_hit, d_rays, d_res, 0), count, args.reps, args.warmup))
                torch.cuda.synchronize()
                wide_res = d_res.cpu().numpy()[:16 * count].copy()
                out["binary"] = step(name + " binary", args.limit, lambda: median_rate(lambda: t.trace_binary(count, any_hit, d_rays, d_res), count, args.reps, args.warmup))
                torch.cuda.synchronize()
                bin_res = d_res.cpu().numpy()[:16 * count]
                out["records_differ"] = int((wide_res.view(np.uint64).reshape(-1, 2) != bin_res.view(np.uint64).reshape(-1, 2)).any(axis=1).sum())
                out["counters"] = step(name + " stats", args.limit, lambda: t.stats(count, any_hit, d_rays, d_res))
                row[batch] = out
            assert nt.trace_status() == 0, "traversal stack overflow"
            print(json.dumps(row), flush=True)
            rows.append(row)
            del t
            nt.lbvh_release_workspace()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
