#!/usr/bin/env python3
"""The on-device refit (ntr_bvh_refit) against rebuilding: refit times, and trace rates through a refitted tree as the mesh leaves
the shape the tree was built for.

For each scene, with the deformation pos' = pos + a * d * sin(k * pos.yzx + phase) (d the scene diagonal, k = 9 / d):
  * at a = --refit-amplitude (2 %): the refit time of the host SAH tree, of the LBVH tree and of the binned SAH tree -- the GPU time
    the blocking call reports (its own stream events: both launches, the counters and their read-back memset) and the span of two
    stream events around the asynchronous form (result = NULL, what a frame loop pays) -- beside ntr_lbvh_build of the deformed mesh
    in the same process (the yardstick: the refit does a strict subset of that build's memory work) and the host SAH build it
    replaces; each a median of --reps calls after --warmup calls;
  * at every a of --amplitudes (2 %, 10 %, 30 %): ntr_trace_bvh Mrays/s, with freshly validated flags, through (a) the SAH tree built
    over the undeformed mesh and refitted, (b) a fresh LBVH of the deformed mesh, (c) a fresh host SAH tree of the deformed mesh, on
    a 1920x1080 primary batch and the 8 x AO batch made from (b)'s primary hits (ntr_raygen_ao, radius 5 as bench.py).  A rate is the
    rays over the sum of the kernel times of --reps launches after --warmup launches.
Prints one JSON line per scene.  One scene per process keeps a run short; on a shared GPU box give every process its own time limit
and chain them, e.g. through scripts/gpu_job.sh:

    timeout -k 10 600 python scripts/bvh_refit_bench.py --scenes atrium --out a.json && \\
    timeout -k 10 600 python scripts/bvh_refit_bench.py --scenes conference_room --out c.json && \\
    timeout -k 10 900 python scripts/bvh_refit_bench.py --scenes hairball --out h.json
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
        return Tree([b.clone() for b in self.bufs], self.nb, self.wb, self.ib)

    def refit(self, n_tri, d_tri, n_vert, d_pos, eps, stream, blocking=True):
        return nt.bvh_refit(self.bufs[0].data_ptr(), self.nb, self.bufs[1].data_ptr(), self.wb, self.bufs[2].data_ptr(), self.ib, n_tri,
                            d_tri.data_ptr(), n_vert, d_pos.data_ptr(), eps, 0, stream, blocking)


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
    ap.add_argument("--refit-amplitude", type=float, default=0.02)
    ap.add_argument("--amplitudes", type=float, nargs="+", default=[0.02, 0.1, 0.3])
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
            else:
                r = nt.persistent_bvh_build(n_tri, d_tri.data_ptr(), n_vert, d_pos.data_ptr(), mn, mx, *ptrs, None, stream)
            return Tree(bufs, r.nodesBytes, r.triWoopBytes, r.triIndexBytes), float(r.seconds) * 1e3

        # the trees of the undeformed mesh
        d_pos0 = up(pos)
        sah0, host_ms = Tree.host_sah(tri, pos)
        lbvh0, _ = device_build("lbvh", d_pos0, pos)
        binned0, _ = device_build("binned", d_pos0, pos)
        row["host_sah_build_ms"] = host_ms

        # refit times at the refit amplitude, and the LBVH build of the same mesh in the same process
        p = deform(pos, args.refit_amplitude)
        d_pos = up(p)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {}
        for key, tree, eps in (("host_sah", sah0, 0.0), ("lbvh", lbvh0, 0.001), ("binned_sah", binned0, 0.0)):
            t = tree.clone()

            def blocking():
                blocking.last = t.refit(n_tri, d_tri, n_vert, d_pos, eps, stream)
                return blocking.last.seconds * 1e3

            def asynchronous():
                ev0.record()
                t.refit(n_tri, d_tri, n_vert, d_pos, eps, stream, blocking=False)
                ev1.record()
                ev1.synchronize()
                return ev0.elapsed_time(ev1)

            times[key] = {"blocking_ms_median": median_of(blocking, args.reps, args.warmup),
                          "async_ms_median": median_of(asynchronous, args.reps, args.warmup),
                          "numNodes": blocking.last.numNodes, "numLeaves": blocking.last.numLeaves}
        row["refit"] = times
        row["lbvh_build_ms_median"] = median_of(lambda: device_build("lbvh", d_pos, p)[1], args.reps, args.warmup)
        row["refit_scratch_bytes"] = nt.bvh_refit_scratch_bytes()

        # trace rates through the refitted SAH tree, a fresh LBVH and a fresh host SAH tree as the deformation grows
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        ns = args.samples
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        d_ao_res = torch.zeros(n * ns * 16, dtype=torch.uint8, device="cuda:0")
        row["mrays_s"] = {}
        for a in args.amplitudes:
            p = deform(pos, a)
            d_pos = up(p)
            refitted = sah0.clone()
            refitted.refit(n_tri, d_tri, n_vert, d_pos, 0.0, stream)
            fresh_lbvh, _ = device_build("lbvh", d_pos, p)
            fresh_sah, fresh_ms = Tree.host_sah(tri, p)
            trees = {"refitted_sah": refitted, "fresh_lbvh": fresh_lbvh, "fresh_host_sah": fresh_sah}
            flags = {k: nt.bvh_validate(t.bufs[0].data_ptr(), t.nb, stream) for k, t in trees.items()}

            def trace(key, count, any_hit, d_r, d_out):
                t = trees[key]
                return nt.trace_bvh(args.kernel, count, any_hit, d_r.data_ptr(), d_out.data_ptr(), t.bufs[0].data_ptr(), t.nb,
                                    t.bufs[1].data_ptr(), t.wb, t.bufs[2].data_ptr(), bvh_flags=flags[key], stream=stream)

            trace("fresh_lbvh", n, False, d_rays, d_res)
            d_nrm = up(scenes.tri_normals(tri, p))
            nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                         5.0, 0xFFF2D5E4, stream)
            torch.cuda.synchronize()
            m = {"fresh_host_sah_build_ms": fresh_ms}
            for key in trees:
                m[key + "_primary"] = rate(lambda: trace(key, n, False, d_rays, d_res), n, args.reps, args.warmup)
                m[key + "_ao"] = rate(lambda: trace(key, n * ns, True, d_ao, d_ao_res), n * ns, args.reps, args.warmup)
            row["mrays_s"]["%g" % a] = m
        print(json.dumps(row), flush=True)
        results.append(row)
        nt.lbvh_release_workspace()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
