#!/usr/bin/env python3
"""Batched BLAS refits (ntr_bvh_refit_batch) against the only other way to refit a pool: one ntr_bvh_refit call per BLAS at pool + offset.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  Every figure is the median of --reps runs after --warmup runs, with the minimum and
maximum beside it, taken by stream events around the work:
  * batch_ms   ntr_bvh_refit_batch with result = NULL (asynchronous: two launches)
  * loop_ms    the loop of asynchronous ntr_bvh_refit calls (result = NULL), one per BLAS, and one synchronisation at the end.  The calls
               go straight through ctypes with arguments marshalled beforehand, so that the loop is the library's and the launches' cost
               as far as Python allows; the events see the stream idle while the host prepares the next call, which is the point
  * build_ms   ntr_ploc_build_batch of the same pool (its own host wall clock, as scripts/ploc_batch_bench.py reports it): refitting
               should be cheaper than rebuilding
The pools are those of scripts/ploc_batch_bench.py: consecutive triangle ranges of one mesh of 2^20 triangles (atrium(2^20), whose
consecutive triangles lie together, and random_soup(2^20), whose ranges each span the scene), 1024 x 1000, 64 x 16 384, 16 384 x 64 and
1 x 2^20, built by ntr_ploc_build_batch; the vertices are then moved by np_bvh_refit's deformation of 2 %.  The batch's pool and the
loop's are compared byte for byte.  Prints one JSON line per row.

    timeout -k 10 900 python scripts/refit_batch_bench.py --out refit_batch.json
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

import np_bvh_refit as rf  # noqa: E402

F = np.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("refit_batch_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
        sys.stderr.flush()
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


def ranges_of(tri, pos, count, size):
    """`count` meshes of `size` consecutive triangles, each over its own bounding box."""
    assert count * size <= tri.shape[0]
    v = pos[tri[:count * size]].reshape(count, size * 3, 3)
    lo, hi = v.min(axis=1), v.max(axis=1)
    return [(k * size, size, lo[k], hi[k]) for k in range(count)]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", nargs="+", default=["atrium", "soup"])
    ap.add_argument("--shapes", nargs="+", default=["1024x1000", "64x16384", "16384x64", "1x1048576"], help="meshes x triangles")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    L = nt.lib()
    vp = C.c_void_p
    rows = []

    for source in args.sources:
        tri, pos = (scenes.atrium(1 << 20) if source == "atrium" else scenes.random_soup(1 << 20, seed=20, walls=False))[:2]
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        d_tri, d_pos, d_moved = up(tri), up(pos), up(rf.deform(pos, 0.02))
        nv = pos.shape[0]
        for shape in args.shapes:
            count, size = (int(x) for x in shape.split("x"))
            name = "%s %s" % (source, shape)
            meshes = ranges_of(tri, pos, count, size)
            marr = (nt.PlocBatchMesh * count)(*[nt.PlocBatchMesh(*m) for m in meshes])
            caps = nt.ploc_batch_capacity(marr)
            built = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps[:3]]

            def build():
                return nt.ploc_build_batch(marr, tri.shape[0], d_tri.data_ptr(), nv, d_pos.data_ptr(), built[0].data_ptr(), caps[0],
                                           built[1].data_ptr(), caps[1], built[2].data_ptr(), caps[2], 8, stream)

            nt.lbvh_release_workspace()
            runs = step(name + " build", args.limit, lambda: [build() for _ in range(args.warmup + args.reps)][args.warmup:])
            ranges = runs[-1][1]
            build_ms = [r[0].seconds * 1e3 for r in runs]
            batch, loop = [b.clone() for b in built], [b.clone() for b in built]

            earr = (nt.RefitBatchEntry * count)(*[nt.RefitBatchEntry(r, m[0], m[1], 0.0) for r, m in zip(ranges, meshes)])
            batch_args = (count, C.cast(earr, vp), vp(batch[0].data_ptr()), caps[0], vp(batch[1].data_ptr()), caps[1], vp(batch[2].data_ptr()),
                          tri.shape[0], vp(d_tri.data_ptr()), nv, vp(d_moved.data_ptr()), None, None, vp(stream))
            loop_args = [(vp(loop[0].data_ptr() + no), nb, vp(loop[1].data_ptr() + wo), wb, vp(loop[2].data_ptr() + wo // 4), wb // 4, m[1],
                          vp(d_tri.data_ptr() + 12 * m[0]), nv, vp(d_moved.data_ptr()), C.c_float(0.0), None, None, vp(stream))
                         for (no, nb, wo, wb), m in zip(ranges, meshes)]

            def run_batch():
                if L.ntr_bvh_refit_batch(*batch_args) != 0:
                    raise RuntimeError(L.ntr_last_error())

            def run_loop():
                refit = L.ntr_bvh_refit
                for a in loop_args:
                    if refit(*a) != 0:
                        raise RuntimeError(L.ntr_last_error())

            def measure(fn):
                return [event_ms(fn) for _ in range(args.warmup + args.reps)][args.warmup:]

            batch_ms = step(name + " batch", args.limit, lambda: measure(run_batch))
            res = step(name + " batch, blocking", args.limit, lambda: nt.bvh_refit_batch(
                earr, batch[0].data_ptr(), caps[0], batch[1].data_ptr(), caps[1], batch[2].data_ptr(), tri.shape[0], d_tri.data_ptr(), nv,
                d_moved.data_ptr(), 0, stream))
            scratch = nt.bvh_refit_batch_scratch_bytes()
            loop_ms = step(name + " loop", args.limit, lambda: measure(run_loop))
            equal = all(bool(torch.equal(a, b)) for a, b in zip(batch, loop))
            changed = not bool(torch.equal(batch[0], built[0]))
            row = {"source": source, "meshes": count, "tris_per_mesh": size, "tris": count * size, "batch_ms": stats(batch_ms),
                   "loop_ms": stats(loop_ms), "build_ms": stats(build_ms), "ratio_loop_over_batch": float(np.median(loop_ms) / np.median(batch_ms)),
                   "ratio_build_over_batch": float(np.median(build_ms) / np.median(batch_ms)), "pools_equal": equal, "pool_changed": changed,
                   "lanesPerLeaf": res.lanesPerLeaf, "numNodes": res.numNodes, "blocking_gpu_ms": res.seconds * 1e3,
                   "scratch_bytes_per_tri": scratch / (count * size), "mtris_per_s_batch": count * size / float(np.median(batch_ms)) / 1e3}
            print(json.dumps(row), flush=True)
            rows.append(row)
            if not (equal and changed):
                sys.stderr.write("refit_batch_bench: %s: the batch's pool differs from the loop's, or nothing was refitted; stopping\n" % name)
                sys.exit(1)
            del batch, loop, built

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
