#!/usr/bin/env python3
"""What the in-place refit of 4-wide trees (ntr_pool_wide_refit, ntr_tlas_wide_refit) costs beside the only other way to
bring wide trees to a moved, deformed frame: widening again (ntr_pool_widen, ntr_tlas_widen).  Recorded, not gated.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  Every figure is the median of --reps runs after --warmup runs, with the minimum and
maximum beside it, taken by stream events around the call (the blocking widenings: events around the call, and the call's own wall
clock):
  * forest   scripts/instanced_bench.py's 4 096-instance forest (one BLAS of 1 000 triangles, a 16 x 16 x 16 grid, spacing 30), the
             vertices deformed by np_bvh_refit's 2 % wave and every instance translated by a seeded 10 % of the spacing: the update by
             ntr_bvh_refit_batch + ntr_pool_wide_refit (rewriteRows 0) + ntr_tlas_refit + ntr_tlas_wide_refit, the all-wide update by
             ntr_pool_wide_refit (rewriteRows 1) + ntr_tlas_wide_refit, the same all-wide update replayed as one HIP graph, and the update
             by ntr_bvh_refit_batch + ntr_tlas_refit + ntr_pool_widen + ntr_tlas_widen; then the 1920x1080 primary batch through the
             refitted wide trees and through the re-widened ones, and the records in which the two differ
  * pool     a pool of 1 024 BLASes of 1 000 triangles each (ntr_ploc_build_batch): ntr_pool_wide_refit with and without the rows,
             ntr_bvh_refit_batch, and ntr_pool_widen's loop
Prints one JSON line per row.

    timeout -k 10 600 python scripts/studies/wide_refit_timing.py --out wide_refit_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

import np_bvh_refit as rf  # noqa: E402
from instanced_bench import Blas, Tlas, rotations, step, transforms, up  # noqa: E402
from tlas_refit_bench import event_ms, refit as tlas_refit, set_transforms, stats  # noqa: E402

F = np.float32
SPACING = 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["forest", "pool"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blases", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def measure(fn):
        return stats([event_ms(fn) for _ in range(args.warmup + args.reps)][args.warmup:])

    def walled(fn):
        """-> (event ms, wall ms) of a blocking call"""
        ev, wall = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            ev.append(event_ms(fn))
            wall.append((time.perf_counter() - t0) * 1e3)
        return stats(ev[args.warmup:]), stats(wall[args.warmup:])

    if "forest" in args.parts:
        def forest():
            tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
            soup = Blas(tri, pos, stream)
            rng = np.random.default_rng(4096)
            g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
            rot, home = rotations(4096, rng), (g - 7.5) * SPACING
            t = Tlas(soup, transforms(rot, home), stream)
            t.widen()
            built = [b.clone() for b in (soup.bufs[0], soup.bufs[1], t.d_wpool, t.d_wtlas, t.d_wrec, t.d_nodes, t.d_rec)]
            d_pos = up(rf.moved(soup.pos, 0.02))
            set_transforms(t, transforms(rot, home + np.random.default_rng(100).uniform(-1.0, 1.0, (4096, 3)) * 0.1 * SPACING))
            n_tris, n_verts = soup.tri.shape[0], soup.pos.shape[0]
            binary_entry = [(soup.ranges[0], 0, n_tris, 0.0)]
            w = t.wide_ranges[0]
            wide_entry = [(w[0], w[1], 0, soup.wb, 0, n_tris, 0.0)]

            def restore():
                for dst, src in zip((soup.bufs[0], soup.bufs[1], t.d_wpool, t.d_wtlas, t.d_wrec, t.d_nodes, t.d_rec), built):
                    dst.copy_(src)

            def binary_pool():
                nt.bvh_refit_batch(binary_entry, soup.bufs[0].data_ptr(), soup.nb, soup.bufs[1].data_ptr(), soup.wb, soup.bufs[2].data_ptr(), n_tris,
                                   soup.d_tri.data_ptr(), n_verts, d_pos.data_ptr(), stream=stream, blocking=False)

            def wide_pool(rewrite, s=stream):
                nt.pool_wide_refit(wide_entry, t.d_wpool.data_ptr(), t.wpool_res.nodesBytes, soup.bufs[1].data_ptr(), soup.wb, soup.bufs[2].data_ptr(),
                                   n_tris, soup.d_tri.data_ptr(), n_verts, d_pos.data_ptr(), rewrite, stream=s, blocking=False)

            def wide_tlas(s=stream):
                nt.tlas_wide_refit(t.n, t.d_inst.data_ptr(), soup.ranges, t.wide_ranges, t.d_wpool.data_ptr(), t.wpool_res.nodesBytes, t.d_wtlas.data_ptr(),
                                   t.wtlas_res.nodesBytes, t.res.rootLink, t.d_wrec.data_ptr(), 64 * t.n, stream=s, blocking=False)

            def both_paths():
                binary_pool()
                wide_pool(0)
                tlas_refit(t)
                wide_tlas()

            def all_wide():
                wide_pool(1)
                wide_tlas()

            def rewiden():
                binary_pool()
                tlas_refit(t)
                t.widen()

            row = {"part": "forest", "instances": t.n, "triangles": n_tris, "wide_pool_bytes": int(t.wpool_res.nodesBytes),
                   "wide_tlas_bytes": int(t.wtlas_res.nodesBytes)}
            row["pool_wide_refit_rows0_ms"] = measure(lambda: wide_pool(0))
            row["pool_wide_refit_rows1_ms"] = measure(lambda: wide_pool(1))
            row["tlas_wide_refit_ms"] = measure(wide_tlas)
            row["bvh_refit_batch_ms"] = measure(binary_pool)
            row["tlas_refit_ms"] = measure(lambda: tlas_refit(t))
            row["update_both_paths_ms"] = measure(both_paths)
            row["update_all_wide_ms"] = measure(all_wide)
            side = torch.cuda.Stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                cs = torch.cuda.current_stream().cuda_stream
                wide_pool(1, cs)
                wide_tlas(cs)
            row["update_all_wide_graph_ms"] = measure(graph.replay)
            del graph
            # the primary batch through the refitted wide trees ...
            cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
            rays, _ = scenes.primary_rays(cam, args.width, args.height)
            n = rays.shape[0]
            d_rays = up(rays)
            d_res, d_ids, d_res2, d_ids2 = (torch.zeros(n * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4, 16, 4))
            restore()
            both_paths()
            torch.cuda.synchronize()
            row["primary_refitted_ms"] = stats([t.trace_wide(n, False, d_rays, d_res, d_ids) * 1e3 for _ in range(args.warmup + args.reps)][args.warmup:])
            # ... and through the re-widened ones (the blocking update timed on the way)
            restore()
            row["update_rewiden_ms"], row["update_rewiden_wall_ms"] = walled(rewiden)
            row["primary_rewidened_ms"] = stats([t.trace_wide(n, False, d_rays, d_res2, d_ids2) * 1e3 for _ in range(args.warmup + args.reps)][args.warmup:])
            a, b = d_res.cpu().numpy().view(np.uint32).reshape(-1, 4), d_res2.cpu().numpy().view(np.uint32).reshape(-1, 4)
            row["primary_rays"] = n
            row["records_that_differ"] = int((a != b).any(axis=1).sum())
            row["scratch_bytes"] = [nt.pool_wide_refit_scratch_bytes(), nt.tlas_wide_refit_scratch_bytes()]
            return row
        emit(step("forest", args.limit, forest))

    if "pool" in args.parts:
        def pool():
            num = args.blases
            tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
            tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
            all_tri = np.concatenate([tri + k * pos.shape[0] for k in range(num)])
            all_pos = np.concatenate([pos + F(0.001 * k) for k in range(num)])
            meshes = [(k * tri.shape[0], tri.shape[0], all_pos[k * pos.shape[0]:(k + 1) * pos.shape[0]].min(axis=0),
                       all_pos[k * pos.shape[0]:(k + 1) * pos.shape[0]].max(axis=0)) for k in range(num)]
            d_tri, d_pos = up(all_tri), up(all_pos)
            cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
            bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (cn, cw, ci)]
            _, ranges, _ = nt.ploc_build_batch(meshes, all_tri.shape[0], d_tri.data_ptr(), all_pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), cn,
                                               bufs[1].data_ptr(), cw, bufs[2].data_ptr(), ci)
            ranges = [tuple(r) for r in ranges]
            cap = nt.pool_widen_capacity(ranges)
            d_wide = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            state = {}

            def widen():
                state["wide"], state["res"] = nt.pool_widen(ranges, bufs[0].data_ptr(), cn, d_wide.data_ptr(), cap, stream)
            widen_ms, widen_wall = walled(widen)
            wide, res = state["wide"], state["res"]
            d_moved = up(rf.moved(all_pos, 0.02))
            entries = [(w[0], w[1], r[2], r[3], m[0], m[1], 0.0) for w, r, m in zip(wide, ranges, meshes)]
            binary = [(r, m[0], m[1], 0.0) for r, m in zip(ranges, meshes)]

            def wide_refit(rewrite):
                nt.pool_wide_refit(entries, d_wide.data_ptr(), res.nodesBytes, bufs[1].data_ptr(), cw, bufs[2].data_ptr(), all_tri.shape[0], d_tri.data_ptr(),
                                   all_pos.shape[0], d_moved.data_ptr(), rewrite, stream=stream, blocking=False)

            def binary_refit():
                nt.bvh_refit_batch(binary, bufs[0].data_ptr(), cn, bufs[1].data_ptr(), cw, bufs[2].data_ptr(), all_tri.shape[0], d_tri.data_ptr(),
                                   all_pos.shape[0], d_moved.data_ptr(), stream=stream, blocking=False)
            blocking = nt.pool_wide_refit(entries, d_wide.data_ptr(), res.nodesBytes, bufs[1].data_ptr(), cw, bufs[2].data_ptr(), all_tri.shape[0],
                                          d_tri.data_ptr(), all_pos.shape[0], d_moved.data_ptr(), 1, stream=stream)
            return {"part": "pool", "blases": num, "triangles": int(all_tri.shape[0]), "wide_pool_bytes": int(res.nodesBytes),
                    "wide_nodes": int(blocking.numNodes), "lanes_per_leaf": int(blocking.lanesPerLeaf), "blocking_gpu_ms": blocking.seconds * 1e3,
                    "pool_wide_refit_rows1_ms": measure(lambda: wide_refit(1)), "pool_wide_refit_rows0_ms": measure(lambda: wide_refit(0)),
                    "bvh_refit_batch_ms": measure(binary_refit), "pool_widen_ms": widen_ms, "pool_widen_wall_ms": widen_wall,
                    "scratch_bytes": nt.pool_wide_refit_scratch_bytes()}
        emit(step("pool", args.limit, pool))

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
