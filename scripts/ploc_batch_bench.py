#!/usr/bin/env python3
"""Batched BLAS builds (ntr_ploc_build_batch) against the only other way to fill a pool: one ntr_ploc_build call per BLAS.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  Every figure is the median of --reps runs after --warmup runs.  batch_call_ms and
loop_calls_ms are the calls' own host wall clock (the result's `seconds`; the loop's is the sum over its calls) and give the ratio;
batch_ms and loop_ms are the wall clock around this script's Python as well (the ctypes marshalling of up to 16 384 meshes or calls);
the batch's phase times are stream events.  The meshes are consecutive triangle ranges of one mesh of 2^20 triangles -- atrium(2^20),
whose consecutive triangles lie together, and random_soup(2^20), whose ranges each span the scene -- every range over its own box:
  * many      1024 x 1000, 64 x 16 384 and 16 384 x 64 triangles: the batch, and the loop of ntr_ploc_build calls into the same pool at
              the batch's offsets; the two pools are compared byte for byte.  ratio_loop_over_batch = loop_calls_ms / batch_call_ms
  * one       one mesh of 2^20 triangles: the batch against ntr_ploc_build of it.  That ratio is the price of segmentation
  * the phase times and the scratch bytes per triangle come with every row
Prints one JSON line per row.

    timeout -k 10 900 python scripts/ploc_batch_bench.py --out ploc_batch.json
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

F = np.float32
PHASES = ("checkMs", "sortMs", "emitMs", "roundsMs")
SLACK = 4096   # ntr_ploc_build asks for ntr_lbvh_capacity bytes, a few rows more than it writes: room behind the last BLAS


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("ploc_batch_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
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


class Pool:
    def __init__(self, meshes):
        self.meshes = meshes
        self.caps = nt.ploc_batch_capacity(meshes)
        self.bufs = [torch.zeros(c + SLACK, dtype=torch.uint8, device="cuda:0") for c in self.caps[:3]]

    def equal(self, other):
        return all(bool(torch.equal(a[:c], b[:c])) for a, b, c in zip(self.bufs, other.bufs, self.caps[:3]))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", nargs="+", default=["atrium", "soup"])
    ap.add_argument("--shapes", nargs="+", default=["1024x1000", "64x16384", "16384x64", "1x1048576"], help="meshes x triangles")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--limit", type=int, default=180, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    for source in args.sources:
        tri, pos = (scenes.atrium(1 << 20) if source == "atrium" else scenes.random_soup(1 << 20, seed=20, walls=False))[:2]
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        d_tri, d_pos = up(tri), up(pos)
        nv = pos.shape[0]
        for shape in args.shapes:
            count, size = (int(x) for x in shape.split("x"))
            meshes = ranges_of(tri, pos, count, size)
            marr = (nt.PlocBatchMesh * count)(*[nt.PlocBatchMesh(*m) for m in meshes])   # (made once: not part of the build)
            batch, loop = Pool(marr), Pool(marr)
            ranges = batch.caps[3]

            def run_batch():
                b = batch.bufs
                return nt.ploc_build_batch(marr, tri.shape[0], d_tri.data_ptr(), nv, d_pos.data_ptr(), b[0].data_ptr(), batch.caps[0],
                                           b[1].data_ptr(), batch.caps[1], b[2].data_ptr(), batch.caps[2], args.radius, stream)[0]

            def run_loop():
                b, tp = loop.bufs, d_tri.data_ptr()
                ends = [x.numel() for x in b]
                last, inside = None, 0.0
                for (first, n, mn, mx), (no, _, wo, _) in zip(meshes, ranges):
                    last = nt.ploc_build(n, tp + 12 * first, nv, d_pos.data_ptr(), mn, mx, b[0].data_ptr() + no, ends[0] - no, b[1].data_ptr() + wo,
                                         ends[1] - wo, b[2].data_ptr() + wo // 4, ends[2] - wo // 4, args.radius, stream)
                    inside += last.seconds
                last.seconds = inside   # the calls' own wall clocks, summed: the loop without this script's Python
                return last

            def measure(fn):
                runs = [wall(fn) for _ in range(args.warmup + args.reps)][args.warmup:]
                return float(np.median([s for s, _ in runs])) * 1e3, [r for _, r in runs]

            name = "%s %s" % (source, shape)
            nt.lbvh_release_workspace()
            batch_ms, results = step(name + " batch", args.limit, lambda: measure(run_batch))
            scratch = nt.ploc_batch_scratch_bytes()
            loop_ms, singles = step(name + " loop", args.limit, lambda: measure(run_loop))
            batch_call_ms = float(np.median([r.seconds for r in results])) * 1e3
            loop_calls_ms = float(np.median([r.seconds for r in singles])) * 1e3
            row = {"source": source, "meshes": count, "tris_per_mesh": size, "tris": count * size, "batch_ms": batch_ms, "loop_ms": loop_ms,
                   "batch_call_ms": batch_call_ms, "loop_calls_ms": loop_calls_ms, "ratio_loop_over_batch": loop_calls_ms / batch_call_ms,
                   "ratio_with_python": loop_ms / batch_ms, "pools_equal": batch.equal(loop), "numRounds": results[-1].numRounds,
                   "maxHeight": results[-1].maxHeight, "scratch_bytes_per_tri": scratch / (count * size),
                   "mtris_per_s_batch": count * size / batch_call_ms / 1e3}
            row.update({p: float(np.median([getattr(r, p) for r in results])) for p in PHASES})
            if count == 1:
                s = singles[-1]
                row.update(single_numRounds=s.numRounds, single_tailClusters=s.tailClusters,
                           single_phases={p: getattr(s, p) for p in ("mortonMs", "sortMs", "emitMs", "roundsMs", "tailMs")})
            print(json.dumps(row), flush=True)
            rows.append(row)
            if not row["pools_equal"]:
                sys.stderr.write("ploc_batch_bench: %s: the batch's pool differs from the loop's; stopping\n" % name)
                sys.exit(1)
            del batch, loop

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
