#!/usr/bin/env python
"""What deforming BLASes cost in the motion-blurred two-level trace (ntr_trace_instanced_deform, ntr_tlas_deform_refit), over
the two frames of scripts/instanced_motion_bench.py: the 1920 x 1080 primary batch (closest hit) and 2^20 host-made AO rays (any hit)
through ONE identity instance of atrium() and through the forest of 4 096 instances of soup1000, whose instances all move.
  * none      no BLAS is flagged, per-ray times: the deform launch against the motion launch over the same buffers -- the price of the
              new kernel on scenes that do not use it.  The records must be equal.
  * time0     every BLAS deforms (np_bvh_refit.deform at 0.05), every ray at time 0: the deform launch against the motion launch over
              the same buffers, whose Woop rows are key 0's.  The records must be equal: this is the kernel's own cost
  * hashed    every BLAS deforms, random times in [0, 1): against the motion launch over the same buffers (the meshes frozen at key 0
              inside the swept boxes), with the counters and the algorithmic bytes
  * refit     ntr_tlas_deform_refit against ntr_tlas_motion_refit, both asynchronous (two launches each), by stream events
  * blas      ntr_bvh_motion_refit_batch against the per-BLAS loop of ntr_bvh_motion_refit that it replaces and against
              ntr_bvh_refit_batch, over a pool of 1 and of --blases copies of soup1000 (a Compact tree's links are relative to its own
              start, so a copy at another offset is a BLAS), all asynchronous and alternated in one run; and over --many-blases copies
              the two batch calls alone.  --parts blas runs this part only
  * frame     frames over deforming BLASes (ntr_instanced_hit_attributes_deform), on the two primary batches with every BLAS
              deforming and one hashed time per pixel: the new attributes launch against ntr_instanced_hit_attributes_motion on the same
              records, and a whole --frame-samples-sample AO frame through the six calls (primary times, trace, attributes,
              ntr_raygen_ao_normals, secondary times, any-hit trace) with the blur's deform path against the motion path, all
              asynchronous on one stream, by stream events.  --parts frame runs this part only
Both launches get the same visibility, a ray mask of 0x7FFFFFFF that refuses nothing.  Launches are alternated, five runs after two
warm-ups; every figure is the median with its minimum and maximum.  One JSON line per row; --out writes them as a list.  Every GPU step
runs under a time limit of its own.

    timeout -k 10 600 python scripts/instanced_deform_bench.py --out instanced_deform.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from instanced_bench import Blas, Tlas, host_ao_rays, rotations, step, transforms, up  # noqa: E402
from instanced_motion_bench import key1, spread  # noqa: E402
from np_bvh_refit import deform  # noqa: E402

F = np.float32


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-rays", type=int, default=1 << 20)
    ap.add_argument("--blases", type=int, default=256)
    ap.add_argument("--many-blases", type=int, default=1024, help="copies for the two batch calls alone")
    ap.add_argument("--frame-samples", type=int, default=8, help="AO samples per primary hit of the frame part")
    ap.add_argument("--frame-radius", type=float, default=5.0)
    ap.add_argument("--parts", default="frames,blas", help="comma-separated: frames (none, time0, hashed, refit), blas, frame")
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def pose(b, d_nodes, d_nodes1, d_woop, d_v0, d_v1, d_pos1, k=0, blocking=False):
        """ntr_bvh_motion_refit of copy k of BLAS b inside pool buffers"""
        nt.bvh_motion_refit(d_nodes.data_ptr() + k * b.nb, b.nb, d_nodes1.data_ptr() + k * b.nb, d_woop.data_ptr() + k * b.wb, b.wb,
                            b.bufs[2].data_ptr(), b.wb // 4, d_v0.data_ptr() + k * b.wb, d_v1.data_ptr() + k * b.wb, b.tri.shape[0], b.d_tri.data_ptr(),
                            b.pos.shape[0], b.d_pos.data_ptr(), d_pos1.data_ptr(), 0.0, stream=stream, blocking=blocking)

    def frame(name, t, tf, cam):
        b, r = t.blas, t.res
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays, d_res, d_ids, d_mres, d_mids = step(name + " buffers", args.limit, lambda: [up(rays)] + [
            torch.zeros(max(n, na) * w, dtype=torch.uint8, device="cuda:0") for w in (16, 4, 16, 4)])
        hashed = np.random.default_rng(11).random(max(n, na)).astype(F)
        d_times = up(hashed)
        d_keys = torch.zeros(128 * t.n, dtype=torch.uint8, device="cuda:0")
        d_inst1 = up(nt.make_instances(key1(tf), np.zeros(t.n, np.int32)))
        d_nodes1, d_v0, d_v1 = (torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (b.nb, b.wb, b.wb))
        d_pos1, d_flags = up(deform(b.pos, 0.05)), up(np.zeros(1, np.uint32))
        motion = nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, d_times.data_ptr(), 0.0)
        dfm = nt.InstanceDeform(d_nodes1.data_ptr(), d_v0.data_ptr(), d_v1.data_ptr())
        vis = nt.InstanceVisibility(0, 0, 0x7FFFFFFF)         # refuses nothing, and selects the masked loop

        def tail():
            return (t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, r.rootLink, t.d_rec.data_ptr(), 64 * t.n, d_keys.data_ptr(), 128 * t.n,
                    0, stream)

        def deform_refit(blocking):
            return nt.tlas_deform_refit(t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), b.ranges, b.bufs[0].data_ptr(), d_nodes1.data_ptr(), b.nb,
                                        d_flags.data_ptr(), *tail(), blocking)

        def motion_refit(blocking):
            return nt.tlas_motion_refit(t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.nb, *tail(), blocking)

        # key 0 of the pool is refitted in place before anything is traced, so every part runs over the same key-0 bytes
        step(name + " BLAS motion refit", args.limit, lambda: pose(b, b.bufs[0], d_nodes1, b.bufs[1], d_v0, d_v1, d_pos1, blocking=True))

        def first_primary():
            motion_refit(True)
            nt.trace_instanced_motion(*t.args(n, False, d_rays, d_res, d_ids), vis=vis, motion=nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, 0, 0.0),
                                      stream=stream)
            torch.cuda.synchronize()
            return d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        res = step(name + " primary for the ao rays", args.limit, first_primary)
        d_ao = step(name + " ao upload", args.limit, lambda: up(host_ao_rays(rays, res, na, 7)))

        def batch(what, count, any_hit, d_r, equal):
            def check():                                      # records (where they must be equal) and counters, before anything is timed
                mst, mm = nt.trace_instanced_motion_stats(*t.args(count, any_hit, d_r, d_res, d_ids), vis=vis, motion=motion, stream=stream)
                dst, dm, dd = nt.trace_instanced_deform_stats(*t.args(count, any_hit, d_r, d_mres, d_mids), vis=vis, motion=motion, deform=dfm,
                                                              stream=stream)
                torch.cuda.synchronize()
                if equal:
                    assert torch.equal(d_res[:16 * count], d_mres[:16 * count]) and torch.equal(d_ids[:4 * count], d_mids[:4 * count]), \
                        "%s %s: the deform launch's records differ from the motion launch's" % (name, what)
                    assert mst.as_dict() == dst.as_dict() and mm.as_dict() == dm.as_dict()
                return dst, dm, dd
            dst, dm, dd = step("%s %s records and counters" % (name, what), args.limit, check)

            def run():
                a, m = [], []
                for _ in range(args.warmup + args.reps):      # alternated: motion, deform, motion, deform, ...
                    a.append(nt.trace_instanced_motion(*t.args(count, any_hit, d_r, d_res, d_ids), vis=vis, motion=motion, stream=stream))
                    m.append(nt.trace_instanced_deform(*t.args(count, any_hit, d_r, d_mres, d_mids), vis=vis, motion=motion, deform=dfm, stream=stream))
                return a[args.warmup:], m[args.warmup:]
            a, m = step("%s %s" % (name, what), args.limit, run)
            out = {"rays": count, "motion_ms": spread(a, 1e3), "deform_ms": spread(m, 1e3),
                   "deform_counters": dict(dst.as_dict(), **dm.as_dict(), **dd.as_dict()),
                   "deform_algorithmic_bytes": int(dd.algorithmic_bytes(dst, dm, ray_times=True))}
            out["deform_over_motion"] = out["deform_ms"]["median"] / out["motion_ms"]["median"]
            out["deform_inner_visits_per_ray"] = dd.numDeformInnerVisits / count
            out["deform_tri_tests_per_ray"] = dd.numDeformTriTests / count
            return out

        for part, flag, times in (("none", 0, hashed), ("time0", 1, np.zeros_like(hashed)), ("hashed", 1, hashed)):
            d_flags.copy_(up(np.full(1, flag, np.uint32)))
            d_times.copy_(up(times))
            rr = step("%s %s deform refit" % (name, part), args.limit, lambda: deform_refit(True))
            row = {"part": part, "frame": name, "instances": t.n, "moving": int(rr.motion.numMoving), "deforming": int(rr.numDeforming)}
            row["primary"] = batch(part + " primary", n, False, d_rays, part != "hashed")
            row["ao"] = batch(part + " ao", na, True, d_ao, part != "hashed")
            emit(row)

        def refits():
            p, m = [], []
            for _ in range(args.warmup + args.reps):          # alternated: motion, deform, motion, deform, ...
                p.append(timed(lambda: motion_refit(False)))
                m.append(timed(lambda: deform_refit(False)))
            return p[args.warmup:], m[args.warmup:]
        p, m = step(name + " refits", args.limit, refits)
        row = {"part": "refit", "frame": name, "instances": t.n, "tlas_motion_refit_ms": spread(p), "tlas_deform_refit_ms": spread(m),
               "scratch_bytes": nt.tlas_deform_refit_scratch_bytes()}
        row["deform_over_motion"] = row["tlas_deform_refit_ms"]["median"] / row["tlas_motion_refit_ms"]["median"]
        emit(row)
        assert nt.trace_status() == 0, "traversal stack overflow"

    def shaded_frame(name, t, tf, cam):
        """The attributes launch and the whole AO frame over scene t with its one BLAS deforming: the deform path against the motion path"""
        b, r = t.blas, t.res
        rays, s2i = scenes.primary_rays(cam, args.width, args.height)
        n, ns = rays.shape[0], args.frame_samples
        m = n * ns
        d_rays, d_s2i = step(name + " frame rays", args.limit, lambda: (up(rays), up(s2i.astype(np.int32))))
        z = lambda c: torch.zeros(c, dtype=torch.uint8, device="cuda:0")      # noqa: E731
        d_times, d_res, d_ids, d_out, d_nrm, d_out0, d_nrm0 = z(4 * n), z(16 * n), z(4 * n), z(16 * n), z(16 * n), z(16 * n), z(16 * n)
        d_srays, d_si2s, d_ss2i, d_stimes, d_sres, d_sids = step(name + " frame buffers", args.limit,
                                                                 lambda: (z(32 * m), z(4 * m), z(4 * m), z(4 * m), z(16 * m), z(4 * m)))
        d_keys = z(128 * t.n)
        d_inst1 = up(nt.make_instances(key1(tf), np.zeros(t.n, np.int32)))
        d_nodes1, d_v0, d_v1 = z(b.nb), z(b.wb), z(b.wb)
        d_pos1, d_flags = up(deform(b.pos, 0.05)), up(np.ones(1, np.uint32))
        dfm = nt.InstanceDeform(d_nodes1.data_ptr(), d_v0.data_ptr(), d_v1.data_ptr())
        geom = nt.InstancedGeometry(t.n, 1, b.tri.shape[0], b.pos.shape[0], t.d_inst.data_ptr(), b.d_blas_tris.data_ptr(), b.d_tri.data_ptr(),
                                    b.d_pos.data_ptr())
        dgeom = nt.InstancedDeformGeometry(d_pos1.data_ptr(), d_flags.data_ptr())
        vis = nt.InstanceVisibility(0, 0, 0x7FFFFFFF)
        pm = nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, d_times.data_ptr(), 0.0)
        sm = nt.InstanceMotion(d_keys.data_ptr(), 128 * t.n, d_stimes.data_ptr(), 0.0)
        step(name + " BLAS motion refit", args.limit, lambda: pose(b, b.bufs[0], d_nodes1, b.bufs[1], d_v0, d_v1, d_pos1, blocking=True))
        rr = step(name + " deform refit", args.limit, lambda: nt.tlas_deform_refit(
            t.n, t.d_inst.data_ptr(), d_inst1.data_ptr(), b.ranges, b.bufs[0].data_ptr(), d_nodes1.data_ptr(), b.nb, d_flags.data_ptr(),
            t.d_nodes.data_ptr() if r.nodesBytes else 0, r.nodesBytes, r.rootLink, t.d_rec.data_ptr(), 64 * t.n, d_keys.data_ptr(), 128 * t.n, 0, stream,
            True))

        def six(deforming):
            """The six calls of one AO frame, asynchronous on the stream"""
            trace = (lambda *a, **k: nt.trace_instanced_deform(*a, deform=dfm, **k)) if deforming else nt.trace_instanced_motion
            nt.ray_times_primary(n, d_s2i.data_ptr(), 0, 0.0, 1.0, d_times.data_ptr(), stream)
            trace(*t.args(n, False, d_rays, d_res, d_ids), vis=vis, motion=pm, stream=stream, timed=False)
            nt.instanced_hit_attributes_deform(n, d_res.data_ptr(), d_ids.data_ptr(), geom, pm, dgeom if deforming else None, d_out.data_ptr(),
                                               d_nrm.data_ptr(), stream)
            nt.raygen_ao_normals(d_srays.data_ptr(), d_si2s.data_ptr(), d_ss2i.data_ptr(), d_rays.data_ptr(), d_out.data_ptr(), d_nrm.data_ptr(), 0, n, ns,
                                 args.frame_radius, 7, stream)
            nt.ray_times_secondary(d_times.data_ptr(), 0, n, ns, d_stimes.data_ptr(), stream)
            trace(*t.args(m, True, d_srays, d_sres, d_sids), vis=vis, motion=sm, stream=stream, timed=False)

        def counts():
            six(True)
            torch.cuda.synchronize()
            hits = int((d_out.view(torch.int32)[::4] >= 0).sum())
            return hits, int((d_sres.view(torch.int32)[::4] >= 0).sum())
        hits, occluded = step(name + " frame once", args.limit, counts)          # (it leaves the deform trace's records for the launches below)

        def launches():
            a, q = [], []
            for _ in range(args.warmup + args.reps):          # alternated: motion, deform, motion, deform, ...
                a.append(timed(lambda: nt.instanced_hit_attributes_motion(n, d_res.data_ptr(), d_ids.data_ptr(), geom, pm, d_out0.data_ptr(),
                                                                            d_nrm0.data_ptr(), stream)))
                q.append(timed(lambda: nt.instanced_hit_attributes_deform(n, d_res.data_ptr(), d_ids.data_ptr(), geom, pm, dgeom, d_out.data_ptr(),
                                                                            d_nrm.data_ptr(), stream)))
            assert torch.equal(d_out, d_out0), "the two attribute calls resolve different ids"
            return a[args.warmup:], q[args.warmup:], int((d_nrm.view(torch.int32).view(-1, 4) != d_nrm0.view(torch.int32).view(-1, 4)).any(dim=1).sum())
        a, q, differ = step(name + " attribute launches", args.limit, launches)

        def frames():
            f0, f1 = [], []
            for _ in range(args.warmup + args.reps):          # alternated: motion path, deform path, ...
                f0.append(timed(lambda: six(False)))
                f1.append(timed(lambda: six(True)))
            return f0[args.warmup:], f1[args.warmup:]
        f0, f1 = step(name + " frames", args.limit, frames)
        row = {"part": "frame", "frame": name, "instances": t.n, "moving": int(rr.motion.numMoving), "deforming": int(rr.numDeforming), "rays": n,
               "samples": ns, "primary_hits": hits, "ao_rays_occluded": occluded, "normals_that_differ": differ,
               "attributes_motion_ms": spread(a), "attributes_deform_ms": spread(q), "frame_motion_ms": spread(f0), "frame_deform_ms": spread(f1)}
        row["attributes_deform_over_motion"] = row["attributes_deform_ms"]["median"] / row["attributes_motion_ms"]["median"]
        row["frame_deform_over_motion"] = row["frame_deform_ms"]["median"] / row["frame_motion_ms"]["median"]
        emit(row)
        assert nt.trace_status() == 0, "traversal stack overflow"

    def blas_loop(b, copies, with_loop=True):
        """ntr_bvh_motion_refit_batch against the per-BLAS loop of ntr_bvh_motion_refit and against ntr_bvh_refit_batch over `copies`
        copies of BLAS b in one pool"""
        d_nodes, d_woop = b.bufs[0][:b.nb].repeat(copies), b.bufs[1][:b.wb].repeat(copies)
        d_idx = b.bufs[2][:b.wb // 4].repeat(copies)
        d_nodes1, d_v0, d_v1 = torch.zeros_like(d_nodes), torch.zeros_like(d_woop), torch.zeros_like(d_woop)
        d_pos1 = up(deform(b.pos, 0.05))
        entries = [((k * b.nb, b.nb, k * b.wb, b.wb), 0, b.tri.shape[0]) for k in range(copies)]

        def batch(blocking):
            return nt.bvh_refit_batch(entries, d_nodes.data_ptr(), d_nodes.numel(), d_woop.data_ptr(), d_woop.numel(), d_idx.data_ptr(), b.tri.shape[0],
                                      b.d_tri.data_ptr(), b.pos.shape[0], b.d_pos.data_ptr(), 0, stream, blocking)

        def motion_batch(blocking):
            return nt.bvh_motion_refit_batch(entries, d_nodes.data_ptr(), d_nodes.numel(), d_nodes1.data_ptr(), d_woop.data_ptr(), d_woop.numel(),
                                             d_idx.data_ptr(), d_v0.data_ptr(), d_v1.data_ptr(), b.tri.shape[0], b.d_tri.data_ptr(), b.pos.shape[0],
                                             b.d_pos.data_ptr(), d_pos1.data_ptr(), 0, stream, blocking)

        def loop(blocking=False):
            for k in range(copies):
                nt.bvh_motion_refit(d_nodes.data_ptr() + k * b.nb, b.nb, d_nodes1.data_ptr() + k * b.nb, d_woop.data_ptr() + k * b.wb, b.wb,
                                    d_idx.data_ptr() + k * (b.wb // 4), b.wb // 4, d_v0.data_ptr() + k * b.wb, d_v1.data_ptr() + k * b.wb,
                                    b.tri.shape[0], b.d_tri.data_ptr(), b.pos.shape[0], b.d_pos.data_ptr(), d_pos1.data_ptr(), 0.0, stream=stream,
                                    blocking=blocking)

        def run():
            batch(True)                                       # once blocking: the scratch and the held tables
            res = motion_batch(True)
            nt.bvh_motion_refit(d_nodes.data_ptr(), b.nb, d_nodes1.data_ptr(), d_woop.data_ptr(), b.wb, d_idx.data_ptr(), b.wb // 4, d_v0.data_ptr(),
                                d_v1.data_ptr(), b.tri.shape[0], b.d_tri.data_ptr(), b.pos.shape[0], b.d_pos.data_ptr(), d_pos1.data_ptr(), 0.0,
                                stream=stream)
            if with_loop:                                     # the batch call's bytes are the loop's, before anything is timed
                mine = [x.clone() for x in (d_nodes, d_nodes1, d_woop, d_v0, d_v1)]
                loop()
                torch.cuda.synchronize()
                for name, x, y in zip(("nodes0", "nodes1", "triWoop", "vertRows0", "vertRows1"), mine, (d_nodes, d_nodes1, d_woop, d_v0, d_v1)):
                    fx, fy = x.view(torch.float32), y.view(torch.float32)    # Woop words that are NaN on both sides compare equal
                    same = torch.equal(x, y) or (name == "triWoop" and bool(((x.view(torch.int32) == y.view(torch.int32)) |
                                                                           (fx.isnan() & fy.isnan())).all()))
                    assert same, "ntr_bvh_motion_refit_batch differs from the loop in " + name
            p, q, m = [], [], []
            for _ in range(args.warmup + args.reps):          # alternated: batch, motion batch, loop, batch, ...
                p.append(timed(lambda: batch(False)))
                q.append(timed(lambda: motion_batch(False)))
                if with_loop:
                    m.append(timed(loop))
            return p[args.warmup:], q[args.warmup:], m[args.warmup:], res
        p, q, m, res = step("blas refits, %d copies" % copies, args.limit, run)
        row = {"part": "blas", "blases": copies, "triangles_per_blas": int(b.tri.shape[0]), "lanes_per_leaf": int(res.lanesPerLeaf),
               "refit_batch_ms": spread(p), "motion_refit_batch_ms": spread(q),
               "scratch_bytes": nt.bvh_motion_refit_batch_scratch_bytes()}
        row["motion_batch_over_batch"] = row["motion_refit_batch_ms"]["median"] / row["refit_batch_ms"]["median"]
        if with_loop:
            row["motion_refit_loop_ms"] = spread(m)
            row["loop_over_motion_batch"] = row["motion_refit_loop_ms"]["median"] / row["motion_refit_batch_ms"]["median"]
            row["loop_over_batch"] = row["motion_refit_loop_ms"]["median"] / row["refit_batch_ms"]["median"]
        emit(row)

    parts = set(args.parts.split(","))
    assert parts and parts <= {"frames", "blas", "frame"}, "--parts takes frames, blas and frame"
    if parts & {"frames", "frame"}:
        tri, pos, cam = scenes.atrium()
        atrium = step("atrium BLAS", args.limit, lambda: Blas(tri, pos, stream))
        tf = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
        if "frames" in parts:
            frame("identity", step("identity tlas", args.limit, lambda: Tlas(atrium, tf, stream)), tf, cam)
        if "frame" in parts:
            shaded_frame("identity", step("identity tlas", args.limit, lambda: Tlas(atrium, tf, stream)), tf, cam)

    tri, pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]
    soup = step("soup1000 BLAS", args.limit, lambda: Blas(tri, pos, stream))
    if parts & {"frames", "frame"}:
        rng = np.random.default_rng(4096)
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        tf = transforms(rotations(4096, rng), (g - 7.5) * 30.0)
        cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
        if "frames" in parts:
            frame("forest", step("forest tlas", args.limit, lambda: Tlas(soup, tf, stream)), tf, cam)
        if "frame" in parts:
            shaded_frame("forest", step("forest tlas", args.limit, lambda: Tlas(soup, tf, stream)), tf, cam)
    if "blas" in parts:
        for copies in (1, args.blases):
            blas_loop(soup, copies)
        blas_loop(soup, args.many_blases, with_loop=False)

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
