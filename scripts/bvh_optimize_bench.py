#!/usr/bin/env python3
"""The on-device treelet optimiser (ntr_bvh_optimize) and SAH cost (ntr_bvh_sah_cost): what a pass costs, what it buys in SAH cost and
in trace rate, and whether it repairs a refitted tree.

For each scene, everything of a row in one process and over the same rays:
  * times: ntr_bvh_optimize of the LBVH tree with 1, 2 and 3 passes and ntr_bvh_sah_cost (the GPU time the blocking calls report: their
    own stream events around every launch and read-back of the call), beside ntr_lbvh_build, the binned SAH build and the host SAH
    build of the same mesh; each device time a median of --reps calls after --warmup calls, every optimise on a fresh copy of the tree;
  * quality: SAH cost (ntr_bvh_sah_cost) and ntr_trace_bvh Mrays/s with freshly validated flags for LBVH, LBVH + 1 / 2 / 3 passes,
    HLBVH (bits 4), binned SAH, binned SAH + 3, host SAH, host SAH + 3, and LBVH, LBVH + 2 and binned SAH copied into the host
    builder's node order by ntr_bvh_reorder ("... reordered"; the optimiser hands a rewritten treelet's slots out wherever they
    lie), with the host SAH tree a second time at the end as its run-to-run spread, on a 1920x1080 primary batch and the 8 x AO batch made from
    the LBVH's primary hits (ntr_raygen_ao, radius 5 as bench.py).  A rate is the rays over the sum of the kernel times of --reps
    launches after --warmup launches;
  * repair: at every a of --amplitudes, with pos' = pos + a * d * sin(k * pos.yzx + phase) as scripts/bvh_refit_bench.py: the host SAH
    tree and the LBVH of the undeformed mesh refitted, each also with --repair-passes passes on top, against a fresh LBVH of the
    deformed mesh; SAH cost and both rates of each.
Prints one JSON line per scene.  One scene per process keeps a run short; on a shared GPU box give every process its own time limit
and chain them:

    timeout -k 10 600 python scripts/bvh_optimize_bench.py --scenes atrium --out a.json && \\
    timeout -k 10 600 python scripts/bvh_optimize_bench.py --scenes conference_room --out c.json && \\
    timeout -k 10 900 python scripts/bvh_optimize_bench.py --scenes hairball --out h.json
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

F = np.float32
PHASE = np.array([0.3, 1.1, 2.3], F)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def deform(pos, a):
    pos = np.ascontiguousarray(pos, F)
    e = (pos.max(axis=0) - pos.min(axis=0)).astype(np.float64)
    d = F(np.sqrt((e * e).sum()))
    k = F(F(9.0) / d)
    s = np.sin((k * pos[:, (1, 2, 0)]).astype(F) + PHASE).astype(F)
    return np.ascontiguousarray((pos + (F(F(a) * d) * s).astype(F)).astype(F))


def slab(sizes):
    """Buffers of `sizes` bytes as 256-byte aligned slices of ONE allocation: the trace's flat fetch needs a tree's node and row
    buffers inside one 4 GiB window (csrc/trace_plan.h), which must not depend on where the allocator puts three late allocations."""
    offs = np.concatenate([[0], np.cumsum([(int(c) + 255) & ~255 for c in sizes])])
    t = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda:0")
    return [t[int(o):int(o) + int(c)] for o, c in zip(offs, sizes)]


def rate(fn, n, reps, warmup):
    for _ in range(warmup):
        fn()
    total = 0.0
    for _ in range(reps):
        total += fn()
    return n * reps / total / 1e6


def median_of(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


class Tree:
    """A Compact tree on the device: [nodes, woop, index] tensors and the extents in use."""

    def __init__(self, bufs, nodes_bytes, woop_bytes, idx_bytes):
        self.bufs, self.nb, self.wb, self.ib = bufs, int(nodes_bytes), int(woop_bytes), int(idx_bytes)

    @staticmethod
    def host_sah(tri, pos):
        t0 = time.time()
        h = nt.sah_build(tri, pos)
        ms = (time.time() - t0) * 1e3
        return Tree([up(h.nodes), up(h.woop), up(h.tri_index)], h.nodes.nbytes, h.woop.nbytes, h.tri_index.nbytes), ms

    def clone(self):
        bufs = slab([b.numel() for b in self.bufs])
        for d, b in zip(bufs, self.bufs):
            d.copy_(b)
        return Tree(bufs, self.nb, self.wb, self.ib)

    def refit(self, n_tri, d_tri, n_vert, d_pos, eps, stream):
        return nt.bvh_refit(self.bufs[0].data_ptr(), self.nb, self.bufs[1].data_ptr(), self.wb, self.bufs[2].data_ptr(), self.ib, n_tri,
                            d_tri.data_ptr(), n_vert, d_pos.data_ptr(), eps, 0, stream, True)

    def optimize(self, passes, stream):
        return nt.bvh_optimize(self.bufs[0].data_ptr(), self.nb, passes, stream)

    def optimized(self, passes, stream):
        t = self.clone()
        t.optimize(passes, stream)
        return t

    def reordered(self, stream):
        """This tree in the host builder's node and row order (ntr_bvh_reorder), in buffers of its own."""
        bufs = slab((self.nb, self.wb, self.ib))
        r = nt.bvh_reorder(self.bufs[0].data_ptr(), self.nb, self.bufs[1].data_ptr(), self.wb, self.bufs[2].data_ptr(), self.ib,
                           bufs[0].data_ptr(), self.nb, bufs[1].data_ptr(), self.wb, bufs[2].data_ptr(), self.ib, stream)
        return Tree(bufs, r.nodesBytes, r.triWoopBytes, r.triIndexBytes)

    def sah(self, stream):
        return nt.bvh_sah_cost(self.bufs[0].data_ptr(), self.nb, self.bufs[1].data_ptr(), self.wb, stream)


SCENES = {"atrium": scenes.atrium, "conference_room": scenes.conference_room, "hairball": scenes.hairball}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--kernel", default="fermi_speculative_while_while")
    ap.add_argument("--amplitudes", type=float, nargs="*", default=[0.02, 0.1, 0.3])
    ap.add_argument("--repair-passes", type=int, default=2)
    ap.add_argument("--once", action="store_true", help="one optimise of the LBVH tree with 3 passes and one SAH cost, nothing else "
                    "(the workload of a kernel-trace profile)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in args.scenes:
        tri, pos, cam = SCENES[name]()
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        n_tri, n_vert = tri.shape[0], pos.shape[0]
        d_tri = up(tri)
        capn, capw, capi = nt.lbvh_capacity(n_tri)
        row = {"scene": name, "tris": int(n_tri)}

        def device_build(kind, d_pos, p):
            bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
            mn, mx = p.min(axis=0), p.max(axis=0)
            ptrs = (bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw, bufs[2].data_ptr(), capi)
            if kind == "lbvh":
                r = nt.lbvh_build(n_tri, d_tri.data_ptr(), n_vert, d_pos.data_ptr(), mn, mx, 8, 0.001, *ptrs, stream)
            elif kind == "hlbvh":
                r = nt.hlbvh_build(n_tri, d_tri.data_ptr(), n_vert, d_pos.data_ptr(), mn, mx, 8, 0.001, 4, *ptrs, stream).lbvh
            else:
                r = nt.persistent_bvh_build(n_tri, d_tri.data_ptr(), n_vert, d_pos.data_ptr(), mn, mx, *ptrs, None, stream)
            return Tree(bufs, r.nodesBytes, r.triWoopBytes, r.triIndexBytes), float(r.seconds) * 1e3

        d_pos0 = up(pos)
        lbvh0, _ = device_build("lbvh", d_pos0, pos)
        if args.once:
            r = lbvh0.optimize(3, stream)
            s = lbvh0.sah(stream)
            print(json.dumps({"scene": name, "optimize": r.as_dict(), "sah": s.as_dict()}), flush=True)
            continue
        hlbvh0, _ = device_build("hlbvh", d_pos0, pos)
        binned0, _ = device_build("binned", d_pos0, pos)
        sah0, host_ms = Tree.host_sah(tri, pos)
        row["host_sah_build_ms"] = host_ms
        row["lbvh_build_ms_median"] = median_of(lambda: device_build("lbvh", d_pos0, pos)[1], args.reps, args.warmup)
        row["binned_build_ms_median"] = median_of(lambda: device_build("binned", d_pos0, pos)[1], args.reps, args.warmup)

        # what the passes cost and do, on the LBVH tree
        opt = {}
        for passes in (1, 2, 3):
            def run():
                t = lbvh0.clone()
                run.last = t.optimize(passes, stream)
                return run.last.seconds * 1e3
            opt["%d" % passes] = {"ms_median": median_of(run, args.reps, args.warmup), **run.last.as_dict()}
        row["optimize_lbvh"] = opt
        row["sah_cost_ms_median"] = median_of(lambda: lbvh0.sah(stream).seconds * 1e3, args.reps, args.warmup)
        row["optimize_scratch_bytes"] = nt.bvh_optimize_scratch_bytes()

        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        ns = args.samples
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        d_ao_res = torch.zeros(n * ns * 16, dtype=torch.uint8, device="cuda:0")

        def measure(trees, ao_from, p):
            """{name: dict(sah, height, primary, ao)} for the trees; the AO batch comes from ao_from's primary hits."""
            flags = {k: nt.bvh_validate(t.bufs[0].data_ptr(), t.nb, stream) for k, t in trees.items()}

            def trace(key, count, any_hit, d_r, d_out):
                t = trees[key]
                return nt.trace_bvh(args.kernel, count, any_hit, d_r.data_ptr(), d_out.data_ptr(), t.bufs[0].data_ptr(), t.nb,
                                    t.bufs[1].data_ptr(), t.wb, t.bufs[2].data_ptr(), bvh_flags=flags[key], stream=stream)

            trace(ao_from, n, False, d_rays, d_res)
            d_nrm = up(scenes.tri_normals(tri, p))
            nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                         5.0, 0xFFF2D5E4, stream)
            torch.cuda.synchronize()
            out = {}
            for key, t in trees.items():
                s = t.sah(stream)
                out[key] = {"sah": float(s.sahCost), "height": s.height,
                            "primary": rate(lambda: trace(key, n, False, d_rays, d_res), n, args.reps, args.warmup),
                            "ao": rate(lambda: trace(key, n * ns, True, d_ao, d_ao_res), n * ns, args.reps, args.warmup)}
            assert nt.trace_status() == 0, "traversal stack overflow"
            return out

        trees = {"lbvh": lbvh0, "lbvh+1": lbvh0.optimized(1, stream), "lbvh+2": lbvh0.optimized(2, stream),
                 "lbvh+3": lbvh0.optimized(3, stream), "hlbvh4": hlbvh0, "binned": binned0, "binned+3": binned0.optimized(3, stream),
                 "host_sah": sah0, "host_sah+3": sah0.optimized(3, stream)}
        trees.update({"lbvh reordered": lbvh0.reordered(stream), "lbvh+2 reordered": trees["lbvh+2"].reordered(stream),
                      "binned reordered": binned0.reordered(stream), "host_sah again": sah0})
        row["quality"] = measure(trees, "lbvh", pos)

        row["repair"] = {}
        k = args.repair_passes
        for a in args.amplitudes:
            p = deform(pos, a)
            d_pos = up(p)
            rs, rl = sah0.clone(), lbvh0.clone()
            rs.refit(n_tri, d_tri, n_vert, d_pos, 0.0, stream)
            rl.refit(n_tri, d_tri, n_vert, d_pos, 0.001, stream)
            fresh, _ = device_build("lbvh", d_pos, p)
            trees = {"refitted_sah": rs, "refitted_sah+%d" % k: rs.optimized(k, stream), "refitted_lbvh": rl,
                     "refitted_lbvh+%d" % k: rl.optimized(k, stream), "fresh_lbvh": fresh, "fresh_lbvh+%d" % k: fresh.optimized(k, stream)}
            row["repair"]["%g" % a] = measure(trees, "fresh_lbvh", p)
        print(json.dumps(row), flush=True)
        results.append(row)
        nt.lbvh_release_workspace()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
