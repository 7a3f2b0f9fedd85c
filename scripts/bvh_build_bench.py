#!/usr/bin/env python3
"""The on-device SAH BVH builds -- binned (ntr_persistent_bvh_build) and full sweep (ntr_sah_device_build, the host SAH builder's
tree) -- against the other BVH builders: build times, tree statistics and trace rates.

For each scene: the build's time (the call's wall clock, the span of its GPU events and their phases, median of --reps builds after
--warmup builds) beside the GPU times the LBVH (ntr_lbvh_build, leafSize 8, epsilon 0.001) and the HLBVH (hlbvhBits 4) report and
the host SAH build (one build, wall clock); and the
ntr_trace_bvh Mrays/s of the device SAH trees, the LBVH and the host SAH tree on the same rays -- a 1920x1080 primary batch and the
8 x AO batch made from the LBVH's primary hits (ntr_raygen_ao, radius 5 as bench.py).  A rate is the rays over the sum of the kernel
times of --reps launches after --warmup launches; the host tree is measured a second time at the end ("host_sah_again_*": its
run-to-run spread in this process), and the ntr_trace_bvh_stats counters of the host tree and the full-sweep device tree -- the
same nodes in another numbering -- are reported for the primary batch.
Reordered columns ("*_reordered"): the full-sweep, binned and LBVH trees copied into the host builder's node and row order by
ntr_bvh_reorder and traced on the same rays; "reorder" holds the pass's GPU time on the full-sweep and the LBVH tree (median of
--reps calls after --warmup calls) beside ntr_bvh_refit of the same tree with unmoved vertices, and whether the reordered
full-sweep tree's node buffer equals the host tree's as values.  Prints one JSON line per scene.

    python scripts/bvh_build_bench.py [--scenes atrium conference_room hairball] [--reps 5] [--warmup 2] [--out f.json]
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


def slab(sizes):
    """Buffers of `sizes` bytes as 256-byte aligned slices of ONE allocation: the trace's flat fetch needs a tree's node and row
    buffers inside one 4 GiB window (csrc/trace_plan.h), which must not depend on where the allocator puts three late allocations."""
    offs = np.concatenate([[0], np.cumsum([(int(c) + 255) & ~255 for c in sizes])])
    t = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda:0")
    return [t[int(o):int(o) + int(c)] for o, c in zip(offs, sizes)]


def median_build(build, reps, warmup):
    for _ in range(warmup):
        build()
    return [build() for _ in range(reps)]


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
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for name in args.scenes:
        tri, pos, cam = SCENES[name]()
        n_tri = tri.shape[0]
        d_tri, d_pos = up(tri), up(pos)
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        capn, capw, capi = nt.lbvh_capacity(n_tri)
        trees = {}
        row = {"scene": name, "tris": int(n_tri)}

        def buffers():
            return [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]

        # the device SAH build
        pb = buffers()

        def persistent():
            r = nt.persistent_bvh_build(n_tri, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, pb[0].data_ptr(), capn,
                                        pb[1].data_ptr(), capw, pb[2].data_ptr(), capi, None, stream)
            persistent.last = r
            return r.seconds, r.prepMs, r.levelsMs, r.emitMs

        runs = np.array(median_build(persistent, args.reps, args.warmup))
        r = persistent.last
        # gpu_event_ms: the span of the build's stream events (prep + levels + emit), the figure the LBVH / HLBVH results report for
        # theirs; here it still holds the idle gaps of the per-level read-backs
        row["persistent_bvh"] = {"wall_ms_median": float(np.median(runs[:, 0]) * 1e3),
                                 "gpu_event_ms_median": float(np.median(runs[:, 1] + runs[:, 2] + runs[:, 3])),
                                 "prep_ms": float(np.median(runs[:, 1])),
                                 "levels_ms": float(np.median(runs[:, 2])), "emit_ms": float(np.median(runs[:, 3])),
                                 **{k: getattr(r, k) for k in ("numNodes", "numLeaves", "numLevels", "maxDepth", "medianFallbacks")}}
        trees["persistent"] = (pb, r.nodesBytes, r.triWoopBytes, r.triIndexBytes)
        # the full-sweep device SAH build: the host SAH builder's tree
        sb = buffers()

        def sweep():
            r = nt.sah_device_build(n_tri, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), sb[0].data_ptr(), capn, sb[1].data_ptr(), capw,
                                    sb[2].data_ptr(), capi, 1, 1, stream)
            sweep.last = r
            return r.seconds, r.prepMs, r.sortMs, r.levelsMs, r.emitMs

        runs = np.array(median_build(sweep, args.reps, args.warmup))
        r = sweep.last
        row["sah_device"] = {"wall_ms_median": float(np.median(runs[:, 0]) * 1e3),
                             "gpu_event_ms_median": float(np.median(runs[:, 1:].sum(axis=1))),
                             "prep_ms": float(np.median(runs[:, 1])), "sort_ms": float(np.median(runs[:, 2])),
                             "levels_ms": float(np.median(runs[:, 3])), "emit_ms": float(np.median(runs[:, 4])),
                             "scratch_bytes_per_tri": nt.sah_device_scratch_bytes() / n_tri,
                             **{k: getattr(r, k) for k in ("numNodes", "numLeaves", "numLevels", "maxDepth", "numDropped")}}
        trees["sah_device"] = (sb, r.nodesBytes, r.triWoopBytes, r.triIndexBytes)
        # LBVH and HLBVH (bits 4): the builds' own GPU times
        lb = buffers()

        def lbvh():
            res = nt.lbvh_build(n_tri, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, lb[0].data_ptr(), capn,
                                lb[1].data_ptr(), capw, lb[2].data_ptr(), capi, stream)
            lbvh.last = res
            return (res.seconds,)

        runs = np.array(median_build(lbvh, args.reps, args.warmup))
        row["lbvh"] = {"ms_median": float(np.median(runs[:, 0]) * 1e3), "numNodes": lbvh.last.numNodes}
        trees["lbvh"] = (lb, lbvh.last.nodesBytes, lbvh.last.triWoopBytes, lbvh.last.triIndexBytes)
        hb = buffers()

        def hlbvh():
            res = nt.hlbvh_build(n_tri, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, 4, hb[0].data_ptr(), capn,
                                 hb[1].data_ptr(), capw, hb[2].data_ptr(), capi, stream)
            return (res.lbvh.seconds,)

        runs = np.array(median_build(hlbvh, args.reps, args.warmup))
        row["hlbvh4"] = {"ms_median": float(np.median(runs[:, 0]) * 1e3)}
        torch.cuda.synchronize()
        if not args.no_host:
            t0 = time.time()
            host = nt.sah_build(tri, pos)
            row["host_sah"] = {"build_ms": (time.time() - t0) * 1e3}
            trees["host_sah"] = ([up(host.nodes), up(host.woop), up(host.tri_index)], host.nodes.nbytes, host.woop.nbytes,
                                 host.tri_index.nbytes)
        # the same trees in the host builder's order (ntr_bvh_reorder), and what the pass costs beside a refit of the same tree
        row["reorder"] = {}
        for key in ("sah_device", "persistent", "lbvh"):
            b, nb, wb, ib = trees[key]
            ob = slab((nb, wb, ib))

            def reorder():
                reorder.last = nt.bvh_reorder(b[0].data_ptr(), nb, b[1].data_ptr(), wb, b[2].data_ptr(), ib, ob[0].data_ptr(), nb,
                                              ob[1].data_ptr(), wb, ob[2].data_ptr(), ib, stream)
                return (reorder.last.seconds,)

            runs = np.array(median_build(reorder, args.reps, args.warmup))
            ro = reorder.last
            trees[key + "_reordered"] = (ob, ro.nodesBytes, ro.triWoopBytes, ro.triIndexBytes)
            cb = [t.clone() for t in b]                  # the refit of the same tree, vertices unmoved, on a copy

            def refit():
                return (nt.bvh_refit(cb[0].data_ptr(), nb, cb[1].data_ptr(), wb, cb[2].data_ptr(), ib, n_tri, d_tri.data_ptr(), pos.shape[0],
                                     d_pos.data_ptr(), 0.0 if key == "sah_device" else 0.001, 0, stream, True).seconds,)

            row["reorder"][key] = {"ms_median": float(np.median(runs[:, 0]) * 1e3),
                                   "refit_ms_median": float(np.median(np.array(median_build(refit, args.reps, args.warmup))[:, 0]) * 1e3),
                                   "scratch_bytes_per_slot": nt.bvh_reorder_scratch_bytes() / (nb // 64), **ro.as_dict()}
            del cb
        if "host_sah" in trees:
            got = trees["sah_device_reordered"][0][0].cpu().numpy().view(np.float32).reshape(-1, 16)
            ref = host.nodes.view(np.float32).reshape(-1, 16)
            row["reorder"]["sah_device"]["nodes_equal_host_as_values"] = bool(
                got.shape == ref.shape and np.array_equal(got[:, :12], ref[:, :12])
                and np.array_equal(got[:, 12:].view(np.int32), ref[:, 12:].view(np.int32)))
        # rays: primary, then 8 x AO from the LBVH's primary hits
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n = rays.shape[0]
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")

        flags = {key: nt.bvh_validate(b[0].data_ptr(), nb, stream) for key, (b, nb, _, _) in trees.items()}

        def trace(key, count, any_hit, d_r, d_out):
            b, nb, wb, _ = trees[key]
            return nt.trace_bvh(args.kernel, count, any_hit, d_r.data_ptr(), d_out.data_ptr(), b[0].data_ptr(), nb, b[1].data_ptr(), wb,
                                b[2].data_ptr(), bvh_flags=flags[key], stream=stream)

        trace("lbvh", n, False, d_rays, d_res)
        ns = args.samples
        d_nrm = up(scenes.tri_normals(tri, pos))
        d_ao = torch.zeros(n * ns * 32, dtype=torch.uint8, device="cuda:0")
        d_map = torch.zeros(n * ns * 4, dtype=torch.uint8, device="cuda:0")
        nt.raygen_ao(d_ao.data_ptr(), d_map.data_ptr(), d_map.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                     5.0, 0xFFF2D5E4, stream)
        torch.cuda.synchronize()
        n_ao = n * ns
        d_ao_res = torch.zeros(n_ao * 16, dtype=torch.uint8, device="cuda:0")
        m = {}
        for key in trees:
            m[key + "_primary"] = rate(lambda: trace(key, n, False, d_rays, d_res), n, args.reps, args.warmup)
            m[key + "_ao"] = rate(lambda: trace(key, n_ao, True, d_ao, d_ao_res), n_ao, args.reps, args.warmup)
        if "host_sah" in trees:
            m["host_sah_again_primary"] = rate(lambda: trace("host_sah", n, False, d_rays, d_res), n, args.reps, args.warmup)
            m["host_sah_again_ao"] = rate(lambda: trace("host_sah", n_ao, True, d_ao, d_ao_res), n_ao, args.reps, args.warmup)
            st = {}
            for key in ("host_sah", "sah_device", "sah_device_reordered"):
                b, nb, wb, _ = trees[key]
                st[key] = nt.trace_bvh_stats(args.kernel, n, False, d_rays.data_ptr(), d_res.data_ptr(), b[0].data_ptr(), nb, b[1].data_ptr(), wb,
                                             b[2].data_ptr(), bvh_flags=flags[key], stream=stream).as_dict()
            row["primary_trace_stats"] = st
        row["mrays_s"] = m
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
