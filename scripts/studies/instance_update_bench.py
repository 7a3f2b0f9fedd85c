#!/usr/bin/env python3
"""The instance update on the device (ntr_instances_update) against what CudaInstancedBVH::setInstances does: the rule on one host
thread (ntr_instances_update_host) and the upload of the 112-byte records.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  Every figure is the median of --reps runs after --warmup runs, with the minimum and
maximum beside it.  For 1 025 and 65 536 instances of soup1000 (the sizes of the TLAS tables in DESIGN.md 6k / 6o) and three shapes --
flat (one root node per instance), depth 3 (one root, N / 64 groups, one node per instance) and the limit depth 16 (one root, fourteen
levels of N / 64 nodes, one node per instance):
  * host      wall clock of ntr_instances_update_host, of the blocking upload of 112 B x N behind it, and of both
  * device    ntr_instances_update with result = NULL (the reset and the kernel), by stream events; its bytes are compared with the
              host's once
  * update    ntr_instances_update -> ntr_tlas_refit on one stream, by stream events, beside ntr_tlas_refit alone
Prints one JSON line per row.

    timeout -k 10 600 python scripts/studies/instance_update_bench.py --out instance_update.json
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

from instanced_bench import Blas, Tlas, rotations, transforms, up  # noqa: E402

F = np.float32


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("instance_update_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
        sys.stderr.flush()
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


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


def hierarchy(n, depth, seed):
    """-> (local (numNodes, 12), parent or None): the instances' nodes first (instance i uses node i), then the levels above them down to
    the root, which comes last.  The upper levels are rigid and small, so that a chain of 16 keeps the scene's extent."""
    rng = np.random.default_rng(seed)
    spread = 25.0 * (n / 1025.0) ** (1.0 / 3.0)
    leaves = transforms(rotations(n, rng), rng.uniform(-spread, spread, (n, 3)))
    if depth == 1:
        return leaves, None
    widths = [n] + [max(1, n // 64)] * (depth - 2) + [1]
    local, parent, first = [leaves], [], 0
    for lv in range(1, depth):
        w = widths[lv]
        local.append(transforms(rotations(w, rng), rng.uniform(-1.0, 1.0, (w, 3))))
        parent.append(first + widths[lv - 1] + rng.integers(0, w, widths[lv - 1]))
        first += widths[lv - 1]
    parent.append(np.array([-1]))
    return np.concatenate(local), np.concatenate(parent).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1025, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    L = nt.lib()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def measure(fn):
        return [fn() for _ in range(args.warmup + args.reps)][args.warmup:]

    tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
    soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))

    for n in args.sizes:
        for shape, depth in (("flat", 1), ("depth3", 3), ("depth16", 16)):
            def run():
                local, parent = hierarchy(n, depth, 7 * n + depth)
                num_nodes = local.shape[0]
                blas = np.zeros(n, np.int32)
                out = np.zeros(n, nt.INSTANCE_DTYPE)
                st = (C.c_uint32 * 4)()
                p_parent = None if parent is None else parent.ctypes.data

                def host():
                    t0 = time.perf_counter()
                    rc = L.ntr_instances_update_host(num_nodes, local.ctypes.data, p_parent, n, None, blas.ctypes.data, out.ctypes.data, C.byref(st))
                    t1 = time.perf_counter()
                    assert rc == 0, L.ntr_last_error()
                    assert L.ntr_memcpy_h2d(t.d_inst.data_ptr(), out.ctypes.data, out.nbytes, None) == 0 and L.ntr_stream_synchronize(None) == 0
                    t2 = time.perf_counter()
                    return (t1 - t0) * 1e3, (t2 - t1) * 1e3

                # the tree to refit: built over the instances the rule gives
                assert L.ntr_instances_update_host(num_nodes, local.ctypes.data, p_parent, n, None, blas.ctypes.data, out.ctypes.data, C.byref(st)) == 0
                t = Tlas(soup, out["objectToWorld"].copy(), stream)
                d_local, d_blas, d_status = up(local), up(blas), torch.zeros(16, dtype=torch.uint8, device="cuda:0")
                d_parent = None if parent is None else up(parent)

                def device():
                    nt.instances_update(num_nodes, d_local.data_ptr(), 0 if d_parent is None else d_parent.data_ptr(), n, 0, d_blas.data_ptr(),
                                        t.d_inst.data_ptr(), d_status.data_ptr(), stream=stream, blocking=False)

                def refit():
                    b = t.blas
                    nt.tlas_refit(n, t.d_inst.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb, t.d_nodes.data_ptr(), t.res.nodesBytes, t.res.rootLink,
                                  t.d_rec.data_ptr(), t.caps[1], 0, stream, False)

                host_ms = measure(host)
                t.d_inst.zero_()
                dev_ms = measure(lambda: event_ms(device))
                same = t.d_inst.cpu().numpy().tobytes() == out.tobytes()
                status = nt.instances_status_read(d_status.data_ptr(), stream)
                refit()                                  # (an uncaptured call first: the refit's range table)
                refit_ms = measure(lambda: event_ms(refit))
                both_ms = measure(lambda: event_ms(lambda: (device(), refit())))
                comp, upl = [h[0] for h in host_ms], [h[1] for h in host_ms]
                return {"instances": n, "shape": shape, "nodes": int(num_nodes), "host_compute_ms": stats(comp), "host_upload_ms": stats(upl),
                        "host_ms": stats([a + b for a, b in host_ms]), "device_ms": stats(dev_ms),
                        "host_over_device": float(np.median([a + b for a, b in host_ms]) / np.median(dev_ms)), "device_equals_host": bool(same),
                        "status": status, "tlas_refit_ms": stats(refit_ms), "update_then_refit_ms": stats(both_ms)}
            emit(step("%d %s" % (n, shape), args.limit, run))

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
