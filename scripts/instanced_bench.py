#!/usr/bin/env python3
"""Instanced scenes (ntr_tlas_build, ntr_trace_instanced): what the top-level build costs and what the second level costs a frame.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung).  Every figure is the median of --reps runs after --warmup runs, timed by stream events (the calls' own seconds / phases):
  * tlas       ntr_tlas_build over 1 025 and 65 536 instances of soup1000, split by phases (boxes, sort, clusters, rounds, tail)
  * identity   a 1920x1080 primary batch and one 2^20-ray AO batch (made on the host from the primary hits: uniform directions, length 5)
               through ONE identity instance of atrium(), beside ntr_trace_bvh (fermi_speculative_while_while, validated flags) on the
               same tree and rays: the price of the second level and of GENERIC arithmetic
  * forest     the same kind of frame through 4 096 instances of soup1000 (a 16 x 16 x 16 grid, seeded rotations)
Each frame part also makes its AO batch on the device, beside the host-made one: ntr_instanced_hit_attributes over the primary hits, then
ntr_raygen_ao_normals with --ao-samples rays per primary ray (length 5), timed together and apart by stream events (attr_aogen_ms,
attr_ms, aogen_ms), and traced (ao_device_instanced).  The identity part times ntr_raygen_ao over the single-level records of the same
frame beside it (raygen_ao_single_ms).  The keys of earlier runs stay as they were.
  * masks      (not in the default parts) instance visibility and the counters of the two-level trace over the identity and the forest
               frame: per batch (primary closest hit, host-made AO any hit) the counters of ntr_trace_instanced_stats, the algorithmic
               bytes and their fraction of 8 TB/s at the measured time, and three launches timed: the unmasked launch, the masked
               launch with everything visible (an instance mask array of all ones) and, for the AO batch, the masked launch with
               every second instance hidden from it (odd instances carry mask 1, even ones 3; the AO rays carry 2)
  * wide       (not in the default parts) the two-level trace over 4-wide trees (ntr_pool_widen, ntr_tlas_widen,
               ntr_trace_instanced_wide) beside the binary one, over the identity and the forest frame: per batch (primary
               closest hit, host-made AO any hit) the binary launch and the wide launch ALTERNATED in this process, each timed by its own
               stream events (median, min, max); per ray the counters of both stats calls (top-level nodes, entries, bottom-level nodes,
               triangle tests), the algorithmic bytes over the median as a fraction of 8 TB/s, and how many records differ between the
               two paths (the spec's known limit, reported and not asserted).  Then what widening costs: the frame's own pool and TLAS,
               and ntr_pool_widen's loop over a pool of 1 024 BLASes of 1 000 triangles each (built by ntr_ploc_build_batch)
  * widen_batch (not in the default parts) ntr_pool_widen_batch beside ntr_pool_widen's loop, ALTERNATED in this process, over
               pools of 1 024 BLASes of 1 000 triangles (6r's pool), 16 384 of 64, 64 of 16 384 and one of 2^20 (the pool shapes of 6m and
               6n), each BLAS a copy of one soup built by ntr_ploc_build_batch: GPU time (the calls' own seconds) and wall time (around the
               entry point itself, on range arrays made once), median, min and max, and the kernel launches and read-backs each call takes -- derived from the trees' heights by the rule of
               the two host loops (widen_counts below; every BLAS of a pool is the same tree, so the pool's height is each BLAS's).  The
               two wide pools, the ranges and the result fields are asserted equal before anything is timed
  * optimize_batch (not in the default parts) ntr_bvh_optimize_batch beside the loop of ntr_bvh_optimize calls, ALTERNATED in this
               process, each on a fresh copy of one pool, over widen_batch's four pool shapes at 2 passes: GPU time (the calls' own
               seconds, summed for the loop) and wall time around the entry points, median, min and max, launches and read-backs; then
               ntr_bvh_sah_cost_batch beside the loop of ntr_bvh_sah_cost calls the same way.  The pools and the costs are asserted equal
  * optimize_forest (not in the default parts) the forest after its mesh has moved by 0.02, 0.1 and 0.3 of its diagonal: the primary batch
               and an AO batch through the refitted BLAS, through the same after 1, 2 and 4 treelet passes and through a rebuilt BLAS --
               time, node fetches per ray (ntr_trace_instanced_stats), the BLAS's SAH cost and the update's own GPU time
  * wide_sweep (not in the default parts) the primary batch of `wide` over k x k x k grids of soup1000 for k = 1, 2, 4, 8, 16 (the last is
               the forest), the camera moved back with the grid: where in instance count the wide path starts to pay
  * fast       (not in the default parts) the FAST slab test in the two-level trace (ntr_instanced_validate, ntr_trace_instanced_fast;
               DESIGN.md 6w) over the identity and the forest frame: per batch (primary closest hit, host-made AO any hit)
               ntr_trace_instanced_masked -- the kernel as it was: the yardstick -- and the fast launch ALTERNATED in this process,
               each timed by its own stream events (median, min, max); the FAST share (fastWaveSteps / waveSteps, niceEntries /
               numInstanceEntries) from ntr_trace_instanced_fast_stats; ntr_instanced_validate's own time and the flags it grants.  The
               records, the instance ids and the eight counters of both paths are asserted equal before anything is timed
  * wide_fast  (not in the default parts) the FAST slab test in the two-level trace over 4-wide trees (ntr_instanced_wide_validate,
               ntr_trace_instanced_wide_fast) over the identity and the forest frame: per batch (primary closest hit,
               host-made AO any hit) ntr_trace_instanced_wide with a vis that shows everything -- the kernel as it was: the yardstick --
               and the wide fast launch ALTERNATED in this process, each timed by its own stream events (median, min, max), and for
               context the binary fast launch of `fast` on the same frame; the FAST share from ntr_trace_instanced_wide_fast_stats;
               ntr_instanced_wide_validate's own time and the flags it grants.  The records, the instance ids and the counters of both
               wide paths are asserted equal before anything is timed
Prints one JSON line per part.

    timeout -k 10 600 python scripts/instanced_bench.py --out instanced.json
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
PHASES = ("boxesMs", "sortMs", "clustersMs", "roundsMs", "tailMs")
KERNEL = "fermi_speculative_while_while"
PEAK_BYTES_PER_S = 8e12   # the HBM figure the roofline fractions are taken of


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def step(name, limit, fn):
    """fn() under a time limit of its own: a step that does not come back ends the process."""
    def expired(*_):
        sys.stderr.write("instanced_bench: step '%s' exceeded %d s; stopping\n" % (name, limit))
        sys.stderr.flush()
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        return fn()
    finally:
        signal.alarm(0)


def rotations(n, rng):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def transforms(rot, translation):
    m = np.zeros((rot.shape[0], 3, 4))
    m[:, :, :3] = rot
    m[:, :, 3] = translation
    return m.astype(F).reshape(-1, 12)


class Blas:
    """One mesh built by ntr_ploc_build at the start of pool buffers of its own."""

    def __init__(self, tri, pos, stream):
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        self.tri, self.pos = tri, pos
        caps = nt.lbvh_capacity(tri.shape[0])
        self.bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps]
        d_tri, d_pos = up(tri), up(pos)
        self.d_tri, self.d_pos, self.d_blas_tris = d_tri, d_pos, up(np.array([(0, tri.shape[0])], np.int32))
        r = nt.ploc_build(tri.shape[0], d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), pos.min(axis=0), pos.max(axis=0), self.bufs[0].data_ptr(),
                          caps[0], self.bufs[1].data_ptr(), caps[1], self.bufs[2].data_ptr(), caps[2], 8, stream)
        self.nb, self.wb = r.nodesBytes, r.triWoopBytes
        self.ranges = [(0, self.nb, 0, self.wb)]
        self.flags = nt.bvh_validate(self.bufs[0].data_ptr(), self.nb, stream)


class Tlas:
    def __init__(self, blas, tf, stream):
        self.blas, self.n, self.stream = blas, tf.shape[0], stream
        self.d_inst = up(nt.make_instances(tf, np.zeros(tf.shape[0], np.int32)))
        self.caps = nt.tlas_capacity(self.n)
        self.d_nodes = torch.zeros(self.caps[0], dtype=torch.uint8, device="cuda:0")
        self.d_rec = torch.zeros(self.caps[1], dtype=torch.uint8, device="cuda:0")
        self.res = self.build()

    def build(self):
        b = self.blas
        return nt.tlas_build(self.n, self.d_inst.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb, self.d_nodes.data_ptr(), self.caps[0],
                             self.d_rec.data_ptr(), self.caps[1], 8, self.stream)

    def geometry(self):
        b = self.blas
        return nt.InstancedGeometry(self.n, 1, b.tri.shape[0], b.pos.shape[0], self.d_inst.data_ptr(), b.d_blas_tris.data_ptr(),
                                    b.d_tri.data_ptr(), b.d_pos.data_ptr())

    def args(self, count, any_hit, d_rays, d_res, d_ids):
        b, r = self.blas, self.res
        return (count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), self.d_nodes.data_ptr(), r.nodesBytes, r.rootLink,
                self.d_rec.data_ptr(), self.n, b.bufs[0].data_ptr(), b.nb, b.bufs[1].data_ptr(), b.wb, b.bufs[2].data_ptr())

    def trace_masked(self, count, any_hit, d_rays, d_res, d_ids, vis):
        return nt.trace_instanced_masked(*self.args(count, any_hit, d_rays, d_res, d_ids), vis=vis, stream=self.stream)

    def stats(self, count, any_hit, d_rays, d_res, d_ids, vis):
        return nt.trace_instanced_stats(*self.args(count, any_hit, d_rays, d_res, d_ids), vis=vis, stream=self.stream)

    def widen(self, reps=1):
        """The wide pool, TLAS and records of this scene; -> (the pool's BvhWideResult runs, the TLAS's TlasWideResult runs)."""
        b, r = self.blas, self.res
        cap = nt.pool_widen_capacity(b.ranges)
        self.d_wpool = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        tcap = nt.bvh_widen_capacity(r.nodesBytes) if r.rootLink == 0 else 0
        self.d_wtlas = torch.zeros(max(tcap, 128), dtype=torch.uint8, device="cuda:0")
        self.d_wrec = torch.zeros(64 * self.n, dtype=torch.uint8, device="cuda:0")
        pools, tops = [], []
        for _ in range(reps):
            self.wide_ranges, p = nt.pool_widen(b.ranges, b.bufs[0].data_ptr(), b.nb, self.d_wpool.data_ptr(), cap, self.stream)
            pools.append(p)
            tops.append(nt.tlas_widen(self.n, self.d_inst.data_ptr(), self.d_nodes.data_ptr(), r.nodesBytes, r.rootLink, b.ranges, self.wide_ranges,
                                      self.d_wtlas.data_ptr(), tcap, self.d_wrec.data_ptr(), 64 * self.n, self.stream))
        self.wpool_res, self.wtlas_res = pools[-1], tops[-1]
        return pools, tops

    def wide_args(self, count, any_hit, d_rays, d_res, d_ids):
        b, r = self.blas, self.res
        return (count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), self.d_wtlas.data_ptr(), self.wtlas_res.nodesBytes, r.rootLink,
                self.d_wrec.data_ptr(), self.n, self.d_wpool.data_ptr(), self.wpool_res.nodesBytes, b.bufs[1].data_ptr(), b.wb, b.bufs[2].data_ptr())

    def trace_wide(self, count, any_hit, d_rays, d_res, d_ids):
        return nt.trace_instanced_wide(*self.wide_args(count, any_hit, d_rays, d_res, d_ids), stream=self.stream)

    def stats_wide(self, count, any_hit, d_rays, d_res, d_ids):
        return nt.trace_instanced_wide_stats(*self.wide_args(count, any_hit, d_rays, d_res, d_ids), stream=self.stream)

    def trace(self, count, any_hit, d_rays, d_res, d_ids):
        b, r = self.blas, self.res
        return nt.trace_instanced(count, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), self.d_nodes.data_ptr(), r.nodesBytes,
                                  r.rootLink, self.d_rec.data_ptr(), self.n, b.bufs[0].data_ptr(), b.nb, b.bufs[1].data_ptr(), b.wb,
                                  b.bufs[2].data_ptr(), self.stream)


def median_rate(fn, count, reps, warmup):
    """fn() -> the launch's GPU seconds; -> dict(ms_median, mrays_per_s)."""
    secs = [fn() for _ in range(warmup + reps)][warmup:]
    ms = float(np.median(secs)) * 1e3
    return {"ms_median": ms, "mrays_per_s": count / ms / 1e3, "ms_min": float(min(secs)) * 1e3, "ms_max": float(max(secs)) * 1e3}


def median_event_ms(fn, reps, warmup):
    """fn() launches on the current stream; -> the median GPU milliseconds between two events around it."""
    ms = []
    for _ in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[warmup:]))


def widen_counts(height, slots, batch_entries=0):
    """(kernel launches, read-backs) of one ntr_bvh_widen of a tree of `slots` slots and `height` wide levels -- or, with batch_entries,
    of one ntr_pool_widen_batch whose tallest BLAS that tree is.  Both host loops launch mark + close per level, four levels at a time,
    and read the next level's extent back after each four until it is empty.  Around that: the seed launch, the two scan launches and
    the emit launch (the batch: the entry-table launch on top), and the read-back of the report (the batch's carries the entry table)."""
    level, readbacks = 0, 0
    while True:
        level = min(level + 4, slots)
        readbacks += 1
        if level >= height or level >= slots:
            break
    return 1 + 2 * level + (4 if batch_entries else 3), readbacks + 1


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
    ap.add_argument("--parts", nargs="+", default=["tlas", "identity", "forest"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-rays", type=int, default=1 << 20)
    ap.add_argument("--ao-samples", type=int, default=8, help="rays per primary ray of the device-made AO batch")
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    soup = None
    if any(p in args.parts for p in ("tlas", "forest", "masks", "wide", "wide_sweep", "optimize_forest", "fast", "wide_fast")):
        tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
        soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))

    if "tlas" in args.parts:
        for n in (1025, 65536):
            rng = np.random.default_rng(n)
            tf = transforms(rotations(n, rng), rng.uniform(-25.0, 25.0, (n, 3)) * (n / 1025.0) ** (1.0 / 3.0))

            def run():
                t = Tlas(soup, tf, stream)
                runs = [t.build() for _ in range(args.warmup + args.reps)][args.warmup:]
                row = {"part": "tlas", "instances": n, "ms_median": float(np.median([r.seconds for r in runs])) * 1e3}
                row.update({p: float(np.median([getattr(r, p) for r in runs])) for p in PHASES})
                row.update(numRounds=runs[-1].numRounds, height=runs[-1].height, tailClusters=runs[-1].tailClusters,
                           scratch_bytes=nt.tlas_scratch_bytes())
                return row
            emit(step("tlas %d" % n, args.limit, run))

    def frame(part, t, cam, single=None):
        """Primary batch and AO batch through Tlas t; single: the Blas to trace beside it with ntr_trace_bvh (same rays)."""
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res, d_ids = (torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4))
        row = {"part": part, "instances": t.n, "primary_rays": n, "ao_rays": na}

        def bvh(count, any_hit, d_r):
            return nt.trace_bvh(KERNEL, count, any_hit, d_r.data_ptr(), d_res.data_ptr(), single.bufs[0].data_ptr(), single.nb,
                                single.bufs[1].data_ptr(), single.wb, single.bufs[2].data_ptr(), bvh_flags=single.flags, stream=stream)
        row["primary_instanced"] = step(part + " primary", args.limit, lambda: median_rate(lambda: t.trace(n, False, d_rays, d_res, d_ids), n, args.reps, args.warmup))
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        row["primary_hits"] = int((res["id"] >= 0).sum())
        if single is not None:
            row["primary_single_level"] = step(part + " primary single", args.limit, lambda: median_rate(lambda: bvh(n, False, d_rays), n, args.reps, args.warmup))
            torch.cuda.synchronize()
            same = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE)
            row["primary_records_equal"] = bool(same.tobytes() == res.tobytes())
        d_ao = up(host_ao_rays(rays, res, na, 7))
        row["ao_instanced"] = step(part + " ao", args.limit, lambda: median_rate(lambda: t.trace(na, True, d_ao, d_res, d_ids), na, args.reps, args.warmup))
        if single is not None:
            row["ao_single_level"] = step(part + " ao single", args.limit, lambda: median_rate(lambda: bvh(na, True, d_ao), na, args.reps, args.warmup))
        # the device-made AO batch: attributes of the two-level primary hits, then the generator over their normals
        ns, nd = args.ao_samples, n * args.ao_samples
        row.update(ao_samples=ns, ao_device_rays=nd)
        t.trace(n, False, d_rays, d_res, d_ids)
        geom = t.geometry()
        d_out, d_nrm = (torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        d_drays = torch.zeros(nd * 32, dtype=torch.uint8, device="cuda:0")
        d_i2s, d_s2i, d_dids = (torch.zeros(nd * 4, dtype=torch.uint8, device="cuda:0") for _ in range(3))
        d_dres = torch.zeros(nd * 16, dtype=torch.uint8, device="cuda:0")

        def attr():
            nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), geom, d_out.data_ptr(), d_nrm.data_ptr(), stream)

        def aogen():
            nt.raygen_ao_normals(d_drays.data_ptr(), d_i2s.data_ptr(), d_s2i.data_ptr(), d_rays.data_ptr(), d_out.data_ptr(), d_nrm.data_ptr(), 0, n,
                                 ns, 5.0, 0x2545f491, stream)
        row["attr_aogen_ms"] = step(part + " attributes + ao generation", args.limit, lambda: median_event_ms(lambda: (attr(), aogen()), args.reps, args.warmup))
        row["attr_ms"] = step(part + " attributes", args.limit, lambda: median_event_ms(attr, args.reps, args.warmup))
        row["aogen_ms"] = step(part + " ao generation", args.limit, lambda: median_event_ms(aogen, args.reps, args.warmup))
        row["ao_device_instanced"] = step(part + " device ao", args.limit, lambda: median_rate(lambda: t.trace(nd, True, d_drays, d_dres, d_dids), nd, args.reps, args.warmup))
        row["resolved_hits"] = nt.count_hits(d_out.data_ptr(), n, stream)
        if single is not None:
            # ntr_raygen_ao over the single-level records of the same frame: the table of triangle normals the two-level hits cannot use
            d_tn = up(scenes.tri_normals(single.tri, single.pos))
            bvh(n, False, d_rays)

            def single_gen():
                nt.raygen_ao(d_drays.data_ptr(), d_i2s.data_ptr(), d_s2i.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_tn.data_ptr(), 0, n, ns,
                             5.0, 0x2545f491, stream)
            row["raygen_ao_single_ms"] = step(part + " single-level ao generation", args.limit, lambda: median_event_ms(single_gen, args.reps, args.warmup))
        assert nt.trace_status() == 0, "traversal stack overflow"
        return row

    def masks_frame(frame_name, t, cam):
        """The counters, the algorithmic bytes and the three timed launches of the part `masks` over one frame."""
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res, d_ids = (torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4))
        row = {"part": "masks", "frame": frame_name, "instances": t.n, "primary_rays": n, "ao_rays": na, "peak_bytes_per_s": PEAK_BYTES_PER_S}
        t.trace(n, False, d_rays, d_res, d_ids)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        d_ao = up(host_ao_rays(rays, res, na, 7))
        d_ones = up(np.full(t.n, 0xFFFFFFFF, np.uint32))
        d_half = up(np.where(np.arange(t.n) % 2 == 0, 3, 1).astype(np.uint32))
        visible = nt.InstanceVisibility(d_ones.data_ptr(), 0, 0xFFFFFFFF)
        half = nt.InstanceVisibility(d_half.data_ptr(), 0, 2)
        row["instances_hidden_from_ao"] = int(t.n // 2)

        def launch(name, count, any_hit, d_r, vis):
            """One launch kind of one batch: its counters, then its time, then the bytes over the time."""
            st = step("%s %s counters" % (frame_name, name), args.limit, lambda: t.stats(count, any_hit, d_r, d_res, d_ids, vis))
            if vis is None:
                fn = lambda: t.trace(count, any_hit, d_r, d_res, d_ids)   # noqa: E731
            else:
                fn = lambda: t.trace_masked(count, any_hit, d_r, d_res, d_ids, vis)   # noqa: E731
            out = step("%s %s" % (frame_name, name), args.limit, lambda: median_rate(fn, count, args.reps, args.warmup))
            out["counters"] = st.as_dict()
            out["algorithmic_bytes"] = int(st.algorithmic_bytes(instance_masks=vis is not None))
            out["fraction_of_peak"] = out["algorithmic_bytes"] / (out["ms_median"] * 1e-3) / PEAK_BYTES_PER_S
            return out
        row["primary_unmasked"] = launch("primary unmasked", n, False, d_rays, None)
        row["primary_masked_all_visible"] = launch("primary masked, all visible", n, False, d_rays, visible)
        row["ao_unmasked"] = launch("ao unmasked", na, True, d_ao, None)
        row["ao_masked_all_visible"] = launch("ao masked, all visible", na, True, d_ao, visible)
        row["ao_masked_half_hidden"] = launch("ao masked, every second instance hidden", na, True, d_ao, half)
        for k in ("primary", "ao"):
            row[k + "_masked_over_unmasked"] = row[k + "_masked_all_visible"]["ms_median"] / row[k + "_unmasked"]["ms_median"]
        assert nt.trace_status() == 0, "traversal stack overflow"
        return row

    def rate(secs, count):
        ms = float(np.median(secs)) * 1e3
        return {"ms_median": ms, "mrays_per_s": count / ms / 1e3, "ms_min": float(min(secs)) * 1e3, "ms_max": float(max(secs)) * 1e3}

    def wide_frame(frame_name, t, cam):
        """The part `wide` over one frame: binary and wide launches alternated, their counters, bytes and differing records."""
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays, d_res, d_ids, d_wres, d_wids = step(frame_name + " buffers", args.limit, lambda: [up(rays)] + [
            torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4, 16, 4)])
        row = {"part": "wide", "frame": frame_name, "instances": t.n, "primary_rays": n, "ao_rays": na, "peak_bytes_per_s": PEAK_BYTES_PER_S}
        pools, tops = step(frame_name + " widening", args.limit, lambda: t.widen(args.warmup + args.reps))
        row["pool_widen_ms"] = float(np.median([p.seconds for p in pools[args.warmup:]])) * 1e3
        row["tlas_widen_ms"] = float(np.median([w.seconds for w in tops[args.warmup:]])) * 1e3
        row.update(wide_pool_bytes=int(t.wpool_res.nodesBytes), binary_pool_bytes=int(t.blas.nb), wide_tlas_bytes=int(t.wtlas_res.nodesBytes),
                   binary_tlas_bytes=int(t.res.nodesBytes), stack_bound=int(t.wtlas_res.stackBound), wide_tlas_counts=list(t.wtlas_res.counts),
                   wide_pool_counts=list(t.wpool_res.counts))
        def first_primary():
            t.trace(n, False, d_rays, d_res, d_ids)
            torch.cuda.synchronize()
            return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        res = step(frame_name + " primary for the ao rays", args.limit, first_primary)
        d_ao = step(frame_name + " ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

        def batch(name, count, any_hit, d_r):
            def run():
                b_secs, w_secs = [], []
                for _ in range(args.warmup + args.reps):      # alternated: binary, wide, binary, wide, ...
                    b_secs.append(t.trace(count, any_hit, d_r, d_res, d_ids))
                    w_secs.append(t.trace_wide(count, any_hit, d_r, d_wres, d_wids))
                torch.cuda.synchronize()                      # (the read-backs of both paths' last records: under the step's limit too)
                back = (d_res.cpu().numpy()[:16 * count].reshape(-1, 16), d_wres.cpu().numpy()[:16 * count].reshape(-1, 16),
                        d_ids.cpu().numpy()[:4 * count].reshape(-1, 4), d_wids.cpu().numpy()[:4 * count].reshape(-1, 4))
                return b_secs[args.warmup:], w_secs[args.warmup:], back
            b_secs, w_secs, (rb, rw, ib, iw) = step("%s %s" % (frame_name, name), args.limit, run)
            out = {"binary": rate(b_secs, count), "wide": rate(w_secs, count),
                   "records_differ": int(((rb != rw).any(axis=1) | (ib != iw).any(axis=1)).sum()),
                   "hit_status_differs": int(((rb[:, :4].view(np.int32)[:, 0] >= 0) != (rw[:, :4].view(np.int32)[:, 0] >= 0)).sum())}
            for key, st in (("binary", step("%s %s binary counters" % (frame_name, name), args.limit, lambda: t.stats(count, any_hit, d_r, d_res, d_ids, None))),
                            ("wide", step("%s %s wide counters" % (frame_name, name), args.limit, lambda: t.stats_wide(count, any_hit, d_r, d_wres, d_wids)))):
                c = st.as_dict()
                out[key]["counters"] = c
                out[key]["per_ray"] = {"top_nodes": c["numTopInnerVisits"] / count, "entries": c["numInstanceEntries"] / count,
                                       "bottom_nodes": c["numInnerVisits"] / count, "tri_tests": c["numTriTests"] / count}
                out[key]["algorithmic_bytes"] = int(st.algorithmic_bytes())
                out[key]["fraction_of_peak"] = out[key]["algorithmic_bytes"] / (out[key]["ms_median"] * 1e-3) / PEAK_BYTES_PER_S
            out["wide_over_binary"] = out["wide"]["ms_median"] / out["binary"]["ms_median"]
            return out
        row["primary"] = batch("primary", n, False, d_rays)
        row["ao"] = batch("ao", na, True, d_ao)
        assert nt.trace_status() == 0, "traversal stack overflow"
        return row

    def fast_frame(frame_name, t, cam):
        """The part `fast` over one frame: masked and fast launches alternated, the FAST share, the validate pass's own time."""
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays, d_res, d_ids, d_fres, d_fids = step(frame_name + " buffers", args.limit, lambda: [up(rays)] + [
            torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4, 16, 4)])
        d_flags = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        b, r = t.blas, t.res
        row = {"part": "fast", "frame": frame_name, "instances": t.n, "primary_rays": n, "ao_rays": na}

        def validate():
            nt.instanced_validate(t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, b.bufs[0].data_ptr(), b.nb, d_flags.data_ptr(), stream)
        row["validate_ms"] = step(frame_name + " validate", args.limit, lambda: median_event_ms(validate, args.reps, args.warmup))
        row["validated_bytes"] = int(r.nodesBytes + b.nb)
        row["granted_tlas_flags"], row["granted_pool_flags"] = nt.instanced_flags_read(d_flags.data_ptr(), stream)

        def first_primary():
            t.trace(n, False, d_rays, d_res, d_ids)
            torch.cuda.synchronize()
            return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        res = step(frame_name + " primary for the ao rays", args.limit, first_primary)
        d_ao = step(frame_name + " ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

        def batch(name, count, any_hit, d_r):
            def check():                                      # records and counters equal, before anything is timed
                st = t.stats(count, any_hit, d_r, d_res, d_ids, None)
                fst, ff = nt.trace_instanced_fast_stats(*t.args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), stream=stream)
                t.trace_masked(count, any_hit, d_r, d_res, d_ids, None)
                nt.trace_instanced_fast(*t.args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                assert torch.equal(d_res[:16 * count], d_fres[:16 * count]) and torch.equal(d_ids[:4 * count], d_fids[:4 * count]), \
                    "%s %s: the fast launch's records differ from the masked launch's" % (frame_name, name)
                assert st.as_dict() == fst.as_dict(), (st.as_dict(), fst.as_dict())
                return st, ff
            st, ff = step("%s %s records and counters" % (frame_name, name), args.limit, check)

            def run():
                m_secs, f_secs = [], []
                for _ in range(args.warmup + args.reps):      # alternated: masked, fast, masked, fast, ...
                    m_secs.append(t.trace_masked(count, any_hit, d_r, d_res, d_ids, None))
                    f_secs.append(nt.trace_instanced_fast(*t.args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), stream=stream))
                return m_secs[args.warmup:], f_secs[args.warmup:]
            m_secs, f_secs = step("%s %s" % (frame_name, name), args.limit, run)
            c, f = st.as_dict(), ff.as_dict()
            out = {"masked": rate(m_secs, count), "fast": rate(f_secs, count), "counters": c, "fast_counters": f,
                   "fast_wave_share": f["fastWaveSteps"] / max(f["waveSteps"], 1), "nice_entry_share": f["niceEntries"] / max(c["numInstanceEntries"], 1),
                   "nice_start_share": f["niceStarts"] / count}
            out["fast_over_masked"] = out["fast"]["ms_median"] / out["masked"]["ms_median"]
            return out
        row["primary"] = batch("primary", n, False, d_rays)
        row["ao"] = batch("ao", na, True, d_ao)
        assert nt.trace_status() == 0, "traversal stack overflow"
        return row

    def wide_fast_frame(frame_name, t, cam):
        """The part `wide_fast` over one frame: wide and wide fast launches alternated, the FAST share, the wide validate pass's own time."""
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays, d_res, d_ids, d_fres, d_fids = step(frame_name + " buffers", args.limit, lambda: [up(rays)] + [
            torch.zeros(max(n, na) * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4, 16, 4)])
        d_flags = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        d_bflags = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        b, r = t.blas, t.res
        row = {"part": "wide_fast", "frame": frame_name, "instances": t.n, "primary_rays": n, "ao_rays": na}
        step(frame_name + " widening", args.limit, lambda: t.widen())
        wt, wp = int(t.wtlas_res.nodesBytes), int(t.wpool_res.nodesBytes)
        everything = nt.InstanceVisibility(0, 0)

        def validate():
            nt.instanced_wide_validate(t.d_wtlas.data_ptr() if wt else 0, wt, t.d_wpool.data_ptr(), wp, d_flags.data_ptr(), stream)
        row["wide_validate_ms"] = step(frame_name + " wide validate", args.limit, lambda: median_event_ms(validate, args.reps, args.warmup))
        row["validated_bytes"] = wt + wp
        row["granted_wide_tlas_flags"], row["granted_wide_pool_flags"] = nt.instanced_flags_read(d_flags.data_ptr(), stream)
        nt.instanced_validate(t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, b.bufs[0].data_ptr(), b.nb, d_bflags.data_ptr(), stream)

        def first_primary():
            t.trace(n, False, d_rays, d_res, d_ids)
            torch.cuda.synchronize()
            return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        res = step(frame_name + " primary for the ao rays", args.limit, first_primary)
        d_ao = step(frame_name + " ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

        def batch(name, count, any_hit, d_r):
            def check():                                      # records and counters equal, before anything is timed
                st = nt.trace_instanced_wide_stats(*t.wide_args(count, any_hit, d_r, d_res, d_ids), vis=everything, stream=stream)
                fst, ff = nt.trace_instanced_wide_fast_stats(*t.wide_args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), vis=everything,
                                                             stream=stream)
                nt.trace_instanced_wide(*t.wide_args(count, any_hit, d_r, d_res, d_ids), vis=everything, stream=stream)
                nt.trace_instanced_wide_fast(*t.wide_args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), vis=everything, stream=stream)
                torch.cuda.synchronize()
                assert torch.equal(d_res[:16 * count], d_fres[:16 * count]) and torch.equal(d_ids[:4 * count], d_fids[:4 * count]), \
                    "%s %s: the wide fast launch's records differ from the wide launch's" % (frame_name, name)
                assert st.as_dict() == fst.as_dict(), (st.as_dict(), fst.as_dict())
                return st, ff
            st, ff = step("%s %s records and counters" % (frame_name, name), args.limit, check)

            def run():
                w_secs, f_secs = [], []
                for _ in range(args.warmup + args.reps):      # alternated: wide, wide fast, wide, wide fast, ...
                    w_secs.append(nt.trace_instanced_wide(*t.wide_args(count, any_hit, d_r, d_res, d_ids), vis=everything, stream=stream))
                    f_secs.append(nt.trace_instanced_wide_fast(*t.wide_args(count, any_hit, d_r, d_fres, d_fids), d_flags.data_ptr(), vis=everything,
                                                               stream=stream))
                return w_secs[args.warmup:], f_secs[args.warmup:]
            w_secs, f_secs = step("%s %s" % (frame_name, name), args.limit, run)
            bf_secs = step("%s %s binary fast" % (frame_name, name), args.limit, lambda: [
                nt.trace_instanced_fast(*t.args(count, any_hit, d_r, d_fres, d_fids), d_bflags.data_ptr(), stream=stream)
                for _ in range(args.warmup + args.reps)][args.warmup:])
            c, f = st.as_dict(), ff.as_dict()
            out = {"wide": rate(w_secs, count), "wide_fast": rate(f_secs, count), "binary_fast": rate(bf_secs, count), "counters": c,
                   "fast_counters": f, "fast_wave_share": f["fastWaveSteps"] / max(f["waveSteps"], 1),
                   "nice_entry_share": f["niceEntries"] / max(c["numInstanceEntries"], 1), "nice_start_share": f["niceStarts"] / count}
            out["wide_fast_over_wide"] = out["wide_fast"]["ms_median"] / out["wide"]["ms_median"]
            return out
        row["primary"] = batch("primary", n, False, d_rays)
        row["ao"] = batch("ao", na, True, d_ao)
        assert nt.trace_status() == 0, "traversal stack overflow"
        return row

    def wide_pool_loop(num_blas=1024):
        """ntr_pool_widen over a pool of num_blas BLASes of soup1000's triangles each: what the unbatched loop costs."""
        tri, pos = soup.tri, soup.pos
        nt_, nv = tri.shape[0], pos.shape[0]
        k = np.arange(num_blas)
        all_tri = (tri[None, :, :] + (k * nv)[:, None, None]).reshape(-1, 3).astype(np.int32)
        all_pos = np.tile(pos, (num_blas, 1)).astype(F)
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        meshes = [(int(i * nt_), int(nt_), mn, mx) for i in k]
        cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
        d_tri, d_pos = up(all_tri), up(all_pos)
        bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (cn, cw, ci)]
        out = nt.ploc_build_batch(meshes, all_tri.shape[0], d_tri.data_ptr(), all_pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), cn,
                                  bufs[1].data_ptr(), cw, bufs[2].data_ptr(), ci, 8, stream)
        ranges = out[1]
        cap = nt.pool_widen_capacity(ranges)
        d_wide = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        gpu, wall = [], []
        for _ in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, r = nt.pool_widen(ranges, bufs[0].data_ptr(), cn, d_wide.data_ptr(), cap, stream)
            wall.append(time.perf_counter() - t0)
            gpu.append(r.seconds)
        gpu, wall = gpu[args.warmup:], wall[args.warmup:]
        return {"part": "wide", "frame": "pool_widen_loop", "blases": num_blas, "tris_per_blas": int(nt_), "binary_pool_bytes": int(cn),
                "wide_pool_bytes": int(r.nodesBytes), "gpu_ms_median": float(np.median(gpu)) * 1e3, "gpu_ms_min": float(min(gpu)) * 1e3,
                "gpu_ms_max": float(max(gpu)) * 1e3, "wall_ms_median": float(np.median(wall)) * 1e3, "wall_ms_min": float(min(wall)) * 1e3,
                "wall_ms_max": float(max(wall)) * 1e3, "wall_us_per_blas": float(np.median(wall)) * 1e6 / num_blas}

    def widen_batch_row(num_blas, tris_per_blas):
        """ntr_pool_widen's loop and ntr_pool_widen_batch, alternated, over num_blas copies of one soup of tris_per_blas triangles."""
        tri, pos = scenes.random_soup(tris_per_blas, seed=1100 + tris_per_blas, walls=False)[:2]
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        nt_, nv = tri.shape[0], pos.shape[0]
        k = np.arange(num_blas)
        all_tri = (tri[None, :, :] + (k * nv)[:, None, None]).reshape(-1, 3).astype(np.int32)
        all_pos = np.tile(pos, (num_blas, 1)).astype(F)
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        meshes = [(int(i * nt_), int(nt_), mn, mx) for i in k]
        cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
        d_tri, d_pos = up(all_tri), up(all_pos)
        bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (cn, cw, ci)]
        out = nt.ploc_build_batch(meshes, all_tri.shape[0], d_tri.data_ptr(), all_pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), cn,
                                  bufs[1].data_ptr(), cw, bufs[2].data_ptr(), ci, 8, stream)
        ranges = out[1]
        cap = nt.pool_widen_capacity(ranges)
        d_loop, d_batch = (torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        calls = {"loop": lambda: nt.pool_widen(ranges, bufs[0].data_ptr(), cn, d_loop.data_ptr(), cap, stream),
                 "batch": lambda: nt.pool_widen_batch(ranges, bufs[0].data_ptr(), cn, d_batch.data_ptr(), cap, stream)}
        (lr, l), (br, b) = calls["loop"](), calls["batch"]()
        torch.cuda.synchronize()
        fields = lambda r: (r.nodesBytes, r.numNodes, list(r.counts), r.numLeafLinks, r.height, r.stackBound)   # noqa: E731
        assert lr == br and fields(l) == fields(b), "the batch's ranges or result differ from the loop's"
        assert torch.equal(d_loop, d_batch), "the batch's wide pool differs from the loop's"
        # timed: the entry points themselves, on range arrays made once (the binding's list conversions are 16 384 Python objects a call)
        import ctypes as C
        arr = (nt.BlasRange * num_blas)(*[nt.BlasRange(*[int(x) for x in r]) for r in ranges])
        w_out, r = (nt.WideBlasRange * num_blas)(), nt.BvhWideResult()
        raw = {"loop": (nt.lib().ntr_pool_widen, d_loop), "batch": (nt.lib().ntr_pool_widen_batch, d_batch)}
        gpu, wall = {"loop": [], "batch": []}, {"loop": [], "batch": []}
        for _ in range(args.warmup + args.reps):          # alternated
            for name in ("loop", "batch"):
                fn, d_out = raw[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = fn(num_blas, C.cast(arr, C.c_void_p), bufs[0].data_ptr(), cn, d_out.data_ptr(), cap, C.cast(w_out, C.c_void_p), C.byref(r),
                        C.c_void_p(stream))
                wall[name].append(time.perf_counter() - t0)
                assert rc == 0, nt.lib().ntr_last_error()
                gpu[name].append(r.seconds)
        slots = ranges[0][1] // 64
        one = widen_counts(b.height, slots)
        row = {"part": "widen_batch", "blases": num_blas, "tris_per_blas": int(nt_), "slots_per_blas": int(slots), "height": int(b.height),
               "binary_pool_bytes": int(cn), "wide_pool_bytes": int(b.nodesBytes), "bytes_equal": True,
               "batch_scratch_bytes": nt.pool_widen_batch_scratch_bytes()}
        for name, (launches, readbacks) in (("loop", (num_blas * one[0], num_blas * one[1])), ("batch", widen_counts(b.height, slots, num_blas))):
            g, w = gpu[name][args.warmup:], wall[name][args.warmup:]
            row[name] = {"gpu_ms_median": float(np.median(g)) * 1e3, "gpu_ms_min": float(min(g)) * 1e3, "gpu_ms_max": float(max(g)) * 1e3,
                         "wall_ms_median": float(np.median(w)) * 1e3, "wall_ms_min": float(min(w)) * 1e3, "wall_ms_max": float(max(w)) * 1e3,
                         "launches": int(launches), "readbacks": int(readbacks)}
        row["single_widen_launches"], row["single_widen_readbacks"] = one
        row["wall_loop_over_batch"] = row["loop"]["wall_ms_median"] / row["batch"]["wall_ms_median"]
        return row

    if "widen_batch" in args.parts:
        for num_blas, tris_per_blas in ((1024, 1000), (16384, 64), (64, 16384), (1, 1 << 20)):
            emit(step("widen_batch %d x %d" % (num_blas, tris_per_blas), args.limit, lambda: widen_batch_row(num_blas, tris_per_blas)))
            nt.lbvh_release_workspace()

    def optimize_batch_row(num_blas, tris_per_blas, passes=2):
        """The loop of ntr_bvh_optimize calls and ntr_bvh_optimize_batch, alternated, each on a fresh copy of one pool of num_blas copies
        of one soup; then the loop of ntr_bvh_sah_cost calls and ntr_bvh_sah_cost_batch over the optimised pool, alternated."""
        import ctypes as C
        tri, pos = scenes.random_soup(tris_per_blas, seed=1100 + tris_per_blas, walls=False)[:2]
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        nt_, nv = tri.shape[0], pos.shape[0]
        k = np.arange(num_blas)
        all_tri = (tri[None, :, :] + (k * nv)[:, None, None]).reshape(-1, 3).astype(np.int32)
        all_pos = np.tile(pos, (num_blas, 1)).astype(F)
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        meshes = [(int(i * nt_), int(nt_), mn, mx) for i in k]
        cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
        d_tri, d_pos = up(all_tri), up(all_pos)
        bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (cn, cw, ci)]
        ranges = nt.ploc_build_batch(meshes, all_tri.shape[0], d_tri.data_ptr(), all_pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), cn,
                                     bufs[1].data_ptr(), cw, bufs[2].data_ptr(), ci, 8, stream)[1]
        L = nt.lib()
        arr = (nt.BlasRange * num_blas)(*[nt.BlasRange(*[int(x) for x in r]) for r in ranges])
        d_work = {"loop": bufs[0].clone(), "batch": bufs[0].clone()}
        one, res = nt.BvhOptimizeResult(), nt.BvhOptimizeBatchResult()

        def loop(d):
            secs = 0.0
            for no, nb, _, _ in ranges:
                rc = L.ntr_bvh_optimize(d.data_ptr() + no, nb, passes, C.byref(one), C.c_void_p(stream))
                assert rc == 0, L.ntr_last_error()
                secs += one.seconds
            return secs

        def batch(d):
            rc = L.ntr_bvh_optimize_batch(num_blas, C.cast(arr, C.c_void_p), d.data_ptr(), cn, passes, None, C.byref(res), C.c_void_p(stream))
            assert rc == 0, L.ntr_last_error()
            return res.seconds
        calls = {"loop": loop, "batch": batch}
        gpu, wall = {"loop": [], "batch": []}, {"loop": [], "batch": []}
        for _ in range(args.warmup + args.reps):          # alternated, each on the pool as built
            for name in ("loop", "batch"):
                d_work[name].copy_(bufs[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                secs = calls[name](d_work[name])
                wall[name].append(time.perf_counter() - t0)
                gpu[name].append(secs)
        torch.cuda.synchronize()
        assert torch.equal(d_work["loop"], d_work["batch"]), "the batch's pool differs from the loop's"
        slots = ranges[0][1] // 64
        # what the loop issues: per BLAS and pass five launches and one per height with roots, one read-back; two launches and two
        # read-backs at the end.  Every BLAS is the same tree, so the batch's launches are one BLAS's
        row = {"part": "optimize_batch", "blases": num_blas, "tris_per_blas": int(nt_), "slots_per_blas": int(slots), "passes": passes,
               "pool_bytes": int(cn), "bytes_equal": True, "height_before": int(res.maxHeightBefore), "height_after": int(res.maxHeightAfter),
               "formed": list(res.formed)[:passes], "rewritten": list(res.rewritten)[:passes],
               "batch_scratch_bytes": nt.bvh_optimize_batch_scratch_bytes()}
        counts = {"loop": (num_blas * int(res.launches), num_blas * (passes + 2)), "batch": (int(res.launches), int(res.readBacks))}

        def summary(name, g, w, launches, readbacks):
            g, w = g[args.warmup:], w[args.warmup:]
            return {"gpu_ms_median": float(np.median(g)) * 1e3, "gpu_ms_min": float(min(g)) * 1e3, "gpu_ms_max": float(max(g)) * 1e3,
                    "wall_ms_median": float(np.median(w)) * 1e3, "wall_ms_min": float(min(w)) * 1e3, "wall_ms_max": float(max(w)) * 1e3,
                    "launches": int(launches), "readbacks": int(readbacks)}
        for name in ("loop", "batch"):
            row[name] = summary(name, gpu[name], wall[name], *counts[name])
        row["wall_loop_over_batch"] = row["loop"]["wall_ms_median"] / row["batch"]["wall_ms_median"]

        # the cost of every BLAS of the optimised pool
        d_opt = d_work["batch"]
        sah_one, sah_res, per = nt.BvhSahResult(), nt.BvhSahBatchResult(), (nt.BvhSahResult * num_blas)()

        def sah_loop():
            secs, costs = 0.0, []
            for no, nb, wo, wb in ranges:
                rc = L.ntr_bvh_sah_cost(d_opt.data_ptr() + no, nb, bufs[1].data_ptr() + wo, wb, C.byref(sah_one), C.c_void_p(stream))
                assert rc == 0, L.ntr_last_error()
                secs += sah_one.seconds
                costs.append(sah_one.sahCost)
            return secs, costs

        def sah_batch():
            rc = L.ntr_bvh_sah_cost_batch(num_blas, C.cast(arr, C.c_void_p), d_opt.data_ptr(), cn, bufs[1].data_ptr(), cw, C.cast(per, C.c_void_p),
                                          C.byref(sah_res), C.c_void_p(stream))
            assert rc == 0, L.ntr_last_error()
            return sah_res.seconds, [p.sahCost for p in per]
        sgpu, swall = {"loop": [], "batch": []}, {"loop": [], "batch": []}
        costs = {}
        for _ in range(args.warmup + args.reps):
            for name, fn in (("loop", sah_loop), ("batch", sah_batch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                secs, costs[name] = fn()
                swall[name].append(time.perf_counter() - t0)
                sgpu[name].append(secs)
        assert np.array_equal(np.asarray(costs["loop"], F).view(np.uint32), np.asarray(costs["batch"], F).view(np.uint32)), "costs differ"
        row["sah_cost"] = float(costs["batch"][0])
        row["sah_loop"] = summary("loop", sgpu["loop"], swall["loop"], 2 * num_blas, num_blas)
        row["sah_batch"] = summary("batch", sgpu["batch"], swall["batch"], 2, 1)
        row["sah_wall_loop_over_batch"] = row["sah_loop"]["wall_ms_median"] / row["sah_batch"]["wall_ms_median"]
        return row

    if "optimize_batch" in args.parts:
        for num_blas, tris_per_blas in ((1024, 1000), (16384, 64), (64, 16384), (1, 1 << 20)):
            emit(step("optimize_batch %d x %d" % (num_blas, tris_per_blas), args.limit, lambda: optimize_batch_row(num_blas, tris_per_blas)))
            nt.lbvh_release_workspace()

    def optimize_forest_rows(t, cam):
        """The forest after its one mesh has moved: the refitted BLAS, the same after 1, 2 and 4 treelet passes, and a rebuilt BLAS, each
        under a TLAS brought to it, traced by the primary batch and an AO batch; time and node fetches per ray, and what each update costs."""
        b = t.blas
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res, d_ids = (torch.zeros(max(n, na) * w, dtype=torch.uint8, device="cuda:0") for w in (16, 4))
        built = [x.clone() for x in b.bufs]
        fetches = lambda c, count: (c["numTopInnerVisits"] + c["numInstanceEntries"] + c["numInnerVisits"]) / count   # noqa: E731
        out = []
        for amp in (0.02, 0.1, 0.3):
            d = float(np.linalg.norm(b.pos.max(axis=0) - b.pos.min(axis=0)))
            moved = (b.pos + F(amp * d) * np.sin(F(7.0 / d) * b.pos[:, (1, 2, 0)] + F(0.5))).astype(F)
            d_moved = up(moved)

            def refit():
                for x, src in zip(b.bufs, built):
                    x.copy_(src)
                r = nt.bvh_refit_batch([(b.ranges[0], 0, b.tri.shape[0], 0.0)], b.bufs[0].data_ptr(), b.nb, b.bufs[1].data_ptr(), b.wb,
                                       b.bufs[2].data_ptr(), b.tri.shape[0], b.d_tri.data_ptr(), b.pos.shape[0], d_moved.data_ptr(), stream=stream)
                tr = nt.tlas_refit(t.n, t.d_inst.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb, t.d_nodes.data_ptr(), t.res.nodesBytes,
                                   t.res.rootLink, t.d_rec.data_ptr(), t.caps[1], stream=stream)
                return (r.seconds + tr.seconds) * 1e3

            def measure(variant, update_ms):
                prim = median_rate(lambda: t.trace(n, False, d_rays, d_res, d_ids), n, args.reps, args.warmup)
                res = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE)
                d_ao = up(host_ao_rays(rays, res, na, 7))
                sp = t.stats(n, False, d_rays, d_res, d_ids, None).as_dict()
                ao = median_rate(lambda: t.trace(na, True, d_ao, d_res, d_ids), na, args.reps, args.warmup)
                sa = t.stats(na, True, d_ao, d_res, d_ids, None).as_dict()
                cost = nt.bvh_sah_cost_batch(b.ranges, b.bufs[0].data_ptr(), b.nb, b.bufs[1].data_ptr(), b.wb, stream)[0][0].sahCost
                out.append({"part": "optimize_forest", "amplitude": amp, "variant": variant, "update_ms": update_ms, "sah_cost": float(cost),
                            "primary": prim, "primary_fetches_per_ray": fetches(sp, n), "ao": ao, "ao_fetches_per_ray": fetches(sa, na),
                            "primary_hits": int(sp["numHits"])})
            ms = step("forest refit %g" % amp, args.limit, refit)
            step("forest refitted %g" % amp, args.limit, lambda: measure("refitted", ms))
            for passes in (1, 2, 4):
                ms = step("forest refit %g" % amp, args.limit, refit)
                o = step("forest optimise %g %d" % (amp, passes), args.limit,
                         lambda: nt.bvh_optimize_batch(b.ranges, b.bufs[0].data_ptr(), b.nb, passes, stream, entry_results=False)[0])
                step("forest optimised %g %d" % (amp, passes), args.limit, lambda: measure("refit + %d passes" % passes, ms + o.seconds * 1e3))

            def rebuild():
                caps = nt.lbvh_capacity(b.tri.shape[0])
                r = nt.ploc_build(b.tri.shape[0], b.d_tri.data_ptr(), b.pos.shape[0], d_moved.data_ptr(), moved.min(axis=0), moved.max(axis=0),
                                  b.bufs[0].data_ptr(), caps[0], b.bufs[1].data_ptr(), caps[1], b.bufs[2].data_ptr(), caps[2], 8, stream)
                assert (r.nodesBytes, r.triWoopBytes) == (b.nb, b.wb)
                t.res = t.build()
                return (r.seconds + t.res.seconds) * 1e3
            ms = step("forest rebuild %g" % amp, args.limit, rebuild)
            step("forest rebuilt %g" % amp, args.limit, lambda: measure("rebuilt", ms))
            assert nt.trace_status() == 0, "traversal stack overflow"
        for x, src in zip(b.bufs, built):
            x.copy_(src)
        t.res = t.build()
        return out

    if any(p in args.parts for p in ("identity", "masks", "wide", "fast", "wide_fast")):
        tri, pos, cam = scenes.atrium()
        atrium = step("atrium BLAS", args.limit, lambda: Blas(tri, pos, stream))
        t = step("identity tlas", args.limit, lambda: Tlas(atrium, np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F), stream))
        if "identity" in args.parts:
            row = frame("identity", t, cam, atrium)
            row["tris"] = int(tri.shape[0])
            emit(row)
        if "masks" in args.parts:
            emit(masks_frame("identity", t, cam))
        if "wide" in args.parts:
            emit(wide_frame("identity", t, cam))
        if "fast" in args.parts:
            emit(fast_frame("identity", t, cam))
        if "wide_fast" in args.parts:
            emit(wide_fast_frame("identity", t, cam))

    if any(p in args.parts for p in ("forest", "masks", "wide", "optimize_forest", "fast", "wide_fast")):
        rng = np.random.default_rng(4096)
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        t = step("forest tlas", args.limit, lambda: Tlas(soup, transforms(rotations(4096, rng), (g - 7.5) * 30.0), stream))
        cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
        if "forest" in args.parts:
            row = frame("forest", t, cam)
            row.update(tlas_height=t.res.height, tlas_ms=t.res.seconds * 1e3)
            emit(row)
        if "masks" in args.parts:
            emit(masks_frame("forest", t, cam))
        if "wide" in args.parts:
            emit(wide_frame("forest", t, cam))
            emit(step("pool widen loop", args.limit, wide_pool_loop))
        if "fast" in args.parts:
            emit(fast_frame("forest", t, cam))
        if "wide_fast" in args.parts:
            emit(wide_fast_frame("forest", t, cam))
        if "optimize_forest" in args.parts:
            for row in optimize_forest_rows(t, cam):
                emit(row)

    if "wide_sweep" in args.parts:
        for k in (1, 2, 4, 8, 16):
            rng = np.random.default_rng(4096)
            g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
            t = step("sweep tlas %d" % k, args.limit, lambda: Tlas(soup, transforms(rotations(k ** 3, rng), (g - (k - 1) / 2.0) * 30.0), stream))
            f = (30.0 * k + 40.0) / 520.0                     # the forest's camera, moved back with the grid's extent
            cam = dict(eye=(40.0 * f, 60.0 * f, -420.0 * f), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
            rays, _ = scenes.primary_rays(cam, args.width, args.height)
            n = rays.shape[0]
            d_rays, d_res, d_ids, d_wres, d_wids = step("sweep buffers %d" % k, args.limit, lambda: [up(rays)] + [
                torch.zeros(n * b, dtype=torch.uint8, device="cuda:0") for b in (16, 4, 16, 4)])
            step("sweep widening %d" % k, args.limit, lambda: t.widen())

            def run():
                b_secs, w_secs = [], []
                for _ in range(args.warmup + args.reps):      # alternated
                    b_secs.append(t.trace(n, False, d_rays, d_res, d_ids))
                    w_secs.append(t.trace_wide(n, False, d_rays, d_wres, d_wids))
                return b_secs[args.warmup:], w_secs[args.warmup:]
            b_secs, w_secs = step("sweep %d" % k, args.limit, run)
            sb = step("sweep %d binary counters" % k, args.limit, lambda: t.stats(n, False, d_rays, d_res, d_ids, None)).as_dict()
            sw = step("sweep %d wide counters" % k, args.limit, lambda: t.stats_wide(n, False, d_rays, d_wres, d_wids)).as_dict()
            fetches = lambda c: (c["numTopInnerVisits"] + c["numInstanceEntries"] + c["numInnerVisits"]) / n   # noqa: E731
            row = {"part": "wide_sweep", "instances": k ** 3, "primary_rays": n, "hits": sb["numHits"], "binary": rate(b_secs, n), "wide": rate(w_secs, n),
                   "binary_fetches_per_ray": fetches(sb), "wide_fetches_per_ray": fetches(sw)}
            row["wide_over_binary"] = row["wide"]["ms_median"] / row["binary"]["ms_median"]
            assert nt.trace_status() == 0, "traversal stack overflow"
            emit(row)

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
