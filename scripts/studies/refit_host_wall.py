#!/usr/bin/env python3
"""What an asynchronous in-place refit call costs the HOST when the device already holds its table -- the call a frame loop makes once
per frame -- for ntr_tlas_refit and ntr_pool_wide_refit (refit_launch.h).  Recorded, not gated.

Run once per build of the library, the builds interleaved on one machine in one session (NTR_LIB_OVERRIDE=<library> python3
scripts/studies/refit_host_wall.py); a build compares with another only through the spread the same build shows against itself.
The calls go straight through ctypes with arguments marshalled beforehand; each is timed by the host's clock around the call alone, and
the stream is drained, untimed, after every 16 calls so that no call waits for a full queue.  Every GPU step runs under its own time
limit (an alarm that ends the process).
  * tlas_refit        1 025 instances of one BLAS of 1 000 triangles (scripts/tlas_refit_bench.py's small set): a table of one range
  * pool_wide_refit   a wide pool of --blases BLASes of 1 000 triangles each (scripts/studies/wide_refit_timing.py's pool): a table of
                      that many entries, built and compared with the held one on every call
Prints one JSON line: the median, the quartiles and the minimum of --calls calls after --warmup, in microseconds.
"""
import argparse
import ctypes as C
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

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--blases", type=int, default=64)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    L, vp = nt.lib(), C.c_void_p

    def walled(fn, call_args):
        us = []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter_ns()
            rc = fn(*call_args)
            us.append((time.perf_counter_ns() - t0) * 1e-3)
            if rc != 0:
                raise RuntimeError(L.ntr_last_error())
            if k % 16 == 15:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        q = np.percentile(us[args.warmup:], [25, 50, 75])
        return {"median_us": float(q[1]), "q25_us": float(q[0]), "q75_us": float(q[2]), "min_us": float(np.min(us[args.warmup:]))}

    tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]

    def tlas():
        soup = Blas(tri, pos, stream)
        rng = np.random.default_rng(1025)
        t = Tlas(soup, transforms(rotations(1025, rng), rng.uniform(-25.0, 25.0, (1025, 3))), stream)
        ranges = (nt.BlasRange * 1)(nt.BlasRange(*[int(x) for x in soup.ranges[0]]))
        return walled(L.ntr_tlas_refit, (t.n, vp(t.d_inst.data_ptr()), 1, C.cast(ranges, vp), vp(soup.bufs[0].data_ptr()), soup.nb,
                                         vp(t.d_nodes.data_ptr()), t.res.nodesBytes, t.res.rootLink, vp(t.d_rec.data_ptr()), t.caps[1], None,
                                         None, vp(stream)))

    def wide_pool():
        num = args.blases
        t32, p32 = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        all_tri = np.concatenate([t32 + k * p32.shape[0] for k in range(num)])
        all_pos = np.concatenate([p32 + F(0.001 * k) for k in range(num)])
        nv = p32.shape[0]
        meshes = [(k * t32.shape[0], t32.shape[0], all_pos[k * nv:(k + 1) * nv].min(axis=0), all_pos[k * nv:(k + 1) * nv].max(axis=0))
                  for k in range(num)]
        d_tri, d_pos = up(all_tri), up(all_pos)
        cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
        bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (cn, cw, ci)]
        _, ranges, _ = nt.ploc_build_batch(meshes, all_tri.shape[0], d_tri.data_ptr(), all_pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), cn,
                                           bufs[1].data_ptr(), cw, bufs[2].data_ptr(), ci)
        ranges = [tuple(r) for r in ranges]
        cap = nt.pool_widen_capacity(ranges)
        d_wide = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        wide, res = nt.pool_widen(ranges, bufs[0].data_ptr(), cn, d_wide.data_ptr(), cap, stream)
        d_moved = up(rf.moved(all_pos, 0.02))
        entries = (nt.WideRefitEntry * num)(*[nt.WideRefitEntry(w[0], w[1], r[2], r[3], m[0], m[1], 0.0) for w, r, m in zip(wide, ranges, meshes)])
        return walled(L.ntr_pool_wide_refit, (num, C.cast(entries, vp), vp(d_wide.data_ptr()), int(res.nodesBytes), vp(bufs[1].data_ptr()), cw,
                                              vp(bufs[2].data_ptr()), all_tri.shape[0], vp(d_tri.data_ptr()), all_pos.shape[0],
                                              vp(d_moved.data_ptr()), 1, None, None, vp(stream)))

    row = {"lib": os.environ.get("NTR_LIB_OVERRIDE", "product"), "calls": args.calls,
           "tlas_refit": step("tlas_refit", args.limit, tlas), "pool_wide_refit": step("pool_wide_refit", args.limit, wide_pool)}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
