#!/usr/bin/env python3
"""A static world beside moving instances: what the seeded two-level trace buys over the world as one more identity
instance.  Recorded as measured, not tuned, and not gated.

One process; every GPU step runs under its own time limit (an alarm that ends the process, so that nothing more is started on a device
that hung); the script stops at the first failure.  The world is atrium() (262 k triangles), the instances are K copies of
instanced_bench's 1 000-triangle soup (K = 64, 1 024, 4 096), each scaled to --size units, rotated and placed inside the atrium's box by a
seeded draw; world and soup are two BLASes of one pool (ntr_ploc_build_batch).  Per K, over the 1920x1080 primary batch (closest hit)
and a 2^20-ray AO batch (any hit; host-made from the primary hits, length --ao-radius), binary and 4-wide, two paths ALTERNATED in this
process, each launch timed by the call's own stream events:
  (a) world_as_instance   K + 1 instances, the world being identity instance K: ntr_trace_instanced_masked (vis NULL: the kernel
                          CudaInstancedBVH::traceBatch launches) / ntr_trace_instanced_wide
  (b) seeded              ntr_trace_bvh on the world BLAS's range of the pool, then ntr_trace_instanced_seeded /
                          ntr_trace_instanced_wide_seeded over the K instances in place: the SUM of both kernel times (world_ms and
                          seeded_ms are given apart as well)
--reps runs after --warmup, reported as median and min - max; then the counters of both (the _stats calls and ntr_trace_bvh_stats), the
records in which the two paths differ, and hit or miss.
  * forest   the cost of the seed read: instanced_bench's 4 096-instance forest, its primary and AO batch, the seeded kernel with an
             all-miss seed beside ntr_trace_instanced_masked -- both forced onto the masked loop by a ray mask that refuses nothing
             (0x7FFFFFFF), so that the seed is the only difference -- and the unmasked kernel for reference.
Prints one JSON line per row.

    timeout -k 10 900 python scripts/studies/seeded_world_study.py --out seeded_world_study.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402

from instanced_bench import KERNEL, Blas, Tlas, host_ao_rays, rotations, step, up  # noqa: E402

F = np.float32
IDENTITY = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)


def spread(secs, count):
    ms = np.asarray(secs, np.float64) * 1e3
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "mrays_per_s": count / float(np.median(ms)) / 1e3}


def zeros(nbytes):
    return torch.zeros(max(int(nbytes), 128), dtype=torch.uint8, device="cuda:0")


class Pool:
    """The world and the soup as BLAS 0 and BLAS 1 of one pool, binary and wide."""

    def __init__(self, world, soup, stream):
        (wt, wp), (st, sp) = world, soup
        self.tri = np.concatenate([wt, st + wp.shape[0]]).astype(np.int32)
        self.pos = np.concatenate([wp, sp]).astype(F)
        meshes = [(0, wt.shape[0], wp.min(axis=0), wp.max(axis=0)), (wt.shape[0], st.shape[0], sp.min(axis=0), sp.max(axis=0))]
        cn, cw, ci, _ = nt.ploc_batch_capacity(meshes)
        self.d_tri, self.d_pos = up(self.tri), up(self.pos)
        self.bufs = [zeros(c) for c in (cn, cw, ci)]
        _, ranges, _ = nt.ploc_build_batch(meshes, self.tri.shape[0], self.d_tri.data_ptr(), self.pos.shape[0], self.d_pos.data_ptr(),
                                           self.bufs[0].data_ptr(), cn, self.bufs[1].data_ptr(), cw, self.bufs[2].data_ptr(), ci, 8, stream)
        self.ranges = [tuple(int(x) for x in r) for r in ranges]
        self.nb, self.wb = cn, cw
        cap = nt.pool_widen_capacity(self.ranges)
        self.d_wide = zeros(cap)
        self.wide_ranges, self.wide_res = nt.pool_widen(self.ranges, self.bufs[0].data_ptr(), cn, self.d_wide.data_ptr(), cap, stream)
        n_off, n_bytes, w_off, w_bytes = self.ranges[0]
        self.world_args = (self.bufs[0].data_ptr() + n_off, n_bytes, self.bufs[1].data_ptr() + w_off, w_bytes, self.bufs[2].data_ptr() + 4 * (w_off // 16))
        self.world_flags = nt.bvh_validate(self.world_args[0], n_bytes, stream)


class Top:
    """A top-level tree over instances of a Pool, binary and wide, and the argument tails of the trace calls."""

    def __init__(self, pool, tf, blas, stream):
        self.pool, self.n = pool, tf.shape[0]
        self.d_inst = up(nt.make_instances(tf, blas))
        caps = nt.tlas_capacity(self.n)
        self.d_nodes, self.d_rec = zeros(caps[0]), zeros(caps[1])
        self.res = nt.tlas_build(self.n, self.d_inst.data_ptr(), pool.ranges, pool.bufs[0].data_ptr(), pool.nb, self.d_nodes.data_ptr(), caps[0],
                                 self.d_rec.data_ptr(), caps[1], 8, stream)
        tcap = nt.bvh_widen_capacity(self.res.nodesBytes) if self.res.rootLink == 0 else 0
        self.d_wtlas, self.d_wrec = zeros(tcap), zeros(64 * self.n)
        self.wres = nt.tlas_widen(self.n, self.d_inst.data_ptr(), self.d_nodes.data_ptr(), self.res.nodesBytes, self.res.rootLink, pool.ranges,
                                  pool.wide_ranges, self.d_wtlas.data_ptr(), tcap, self.d_wrec.data_ptr(), 64 * self.n, stream)

    def tail(self, wide):
        p = self.pool
        if wide:
            return (self.d_wtlas.data_ptr(), self.wres.nodesBytes, self.res.rootLink, self.d_wrec.data_ptr(), self.n, p.d_wide.data_ptr(),
                    p.wide_res.nodesBytes, p.bufs[1].data_ptr(), p.wb, p.bufs[2].data_ptr())
        return (self.d_nodes.data_ptr(), self.res.nodesBytes, self.res.rootLink, self.d_rec.data_ptr(), self.n, p.bufs[0].data_ptr(), p.nb,
                p.bufs[1].data_ptr(), p.wb, p.bufs[2].data_ptr())


def per_ray(c, count):
    return {"top_nodes": c["numTopInnerVisits"] / count, "entries": c["numInstanceEntries"] / count, "bottom_nodes": c["numInnerVisits"] / count,
            "tri_tests": c["numTriTests"] / count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["world", "forest"])
    ap.add_argument("--instances", nargs="+", type=int, default=[64, 1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ao-rays", type=int, default=1 << 20)
    ap.add_argument("--ao-radius", type=float, default=100.0)
    ap.add_argument("--size", type=float, default=60.0, help="the largest extent of one placed soup")
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    soup_tri, soup_pos = scenes.random_soup(1000, seed=1100, walls=False)[:2]

    if "world" in args.parts:
        a_tri, a_pos, cam = scenes.atrium()
        pool = step("pool", args.limit, lambda: Pool((np.asarray(a_tri, np.int32), np.asarray(a_pos, F)), (np.asarray(soup_tri, np.int32), np.asarray(soup_pos, F)), stream))
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res_a, d_res_b = zeros(16 * max(n, na)), zeros(16 * max(n, na))
        d_ids_a, d_ids_b = zeros(4 * max(n, na)), zeros(4 * max(n, na))
        lo, hi = a_pos.min(axis=0), a_pos.max(axis=0)
        centre, half = (lo + hi) / 2, (hi - lo) / 2 * 0.9
        scale = args.size / float((soup_pos.max(axis=0) - soup_pos.min(axis=0)).max())
        for k in args.instances:
            rng = np.random.default_rng(k)
            tf = np.zeros((k, 3, 4))
            tf[:, :, :3] = rotations(k, rng) * scale
            tf[:, :, 3] = centre + rng.uniform(-1.0, 1.0, (k, 3)) * half
            tf = tf.astype(F).reshape(-1, 12)
            inst = step("tlas %d" % k, args.limit, lambda: Top(pool, tf, np.ones(k, np.int32), stream))
            both = step("tlas %d + world" % k, args.limit, lambda: Top(pool, np.concatenate([tf, IDENTITY]), np.concatenate([np.ones(k, np.int32), [0]]), stream))
            row = {"part": "world", "instances": k, "world_tris": int(a_tri.shape[0]), "soup_tris": int(soup_tri.shape[0]), "soup_size": args.size,
                   "primary_rays": n, "ao_rays": na, "ao_radius": args.ao_radius, "reps": args.reps, "warmup": args.warmup}

            def batch(name, count, any_hit, d_r):
                out = {}
                head_a = (count, any_hit, d_r.data_ptr(), d_res_a.data_ptr(), d_ids_a.data_ptr())
                head_b = (count, any_hit, d_r.data_ptr(), d_res_b.data_ptr(), k, d_res_b.data_ptr(), d_ids_b.data_ptr())
                for wide in (False, True):
                    fa = nt.trace_instanced_wide if wide else nt.trace_instanced_masked
                    fb = nt.trace_instanced_wide_seeded if wide else nt.trace_instanced_seeded

                    def run():
                        sa, sw, ss = [], [], []
                        for _ in range(args.warmup + args.reps):      # alternated: (a), (b), (a), (b), ...
                            sa.append(fa(*head_a, *both.tail(wide), stream=stream))
                            sw.append(nt.trace_bvh(KERNEL, count, any_hit, d_r.data_ptr(), d_res_b.data_ptr(), *pool.world_args, bvh_flags=pool.world_flags,
                                                   stream=stream))
                            ss.append(fb(*head_b, *inst.tail(wide), stream=stream))
                        torch.cuda.synchronize()
                        ra, rb = d_res_a.cpu().numpy()[:16 * count].view(np.int32).reshape(-1, 4), d_res_b.cpu().numpy()[:16 * count].view(np.int32).reshape(-1, 4)
                        ia, ib = d_ids_a.cpu().numpy()[:4 * count].view(np.int32), d_ids_b.cpu().numpy()[:4 * count].view(np.int32)
                        return sa[args.warmup:], sw[args.warmup:], ss[args.warmup:], (ra, rb, ia, ib)
                    form = "wide" if wide else "binary"
                    sa, sw, ss, (ra, rb, ia, ib) = step("%d %s %s" % (k, name, form), args.limit, run)
                    o = {"world_as_instance": spread(sa, count), "seeded_sum": spread(np.asarray(sw) + np.asarray(ss), count), "world_ms": spread(sw, count),
                         "seeded_ms": spread(ss, count)}
                    o["seeded_over_world_as_instance"] = o["seeded_sum"]["ms_median"] / o["world_as_instance"]["ms_median"]
                    o["records_differ_id_t_instance"] = int(((ra[:, :2] != rb[:, :2]).any(axis=1) | (ia != ib)).sum())
                    o["hit_status_differs"] = int(((ra[:, 0] != -1) != (rb[:, 0] != -1)).sum())
                    o["hits"] = int((rb[:, 0] != -1).sum())
                    o["hits_in_instances"] = int(((ib >= 0) & (ib < k)).sum())
                    stats_a = (nt.trace_instanced_wide_stats if wide else nt.trace_instanced_stats)
                    stats_b = (nt.trace_instanced_wide_seeded_stats if wide else nt.trace_instanced_seeded_stats)
                    ca = step("%d %s %s counters (a)" % (k, name, form), args.limit, lambda: stats_a(*head_a, *both.tail(wide), stream=stream)).as_dict()

                    def seeded_counters():
                        w = nt.trace_bvh_stats(KERNEL, count, any_hit, d_r.data_ptr(), d_res_b.data_ptr(), *pool.world_args, bvh_flags=pool.world_flags,
                                               stream=stream)
                        nt.trace_bvh(KERNEL, count, any_hit, d_r.data_ptr(), d_res_b.data_ptr(), *pool.world_args, bvh_flags=pool.world_flags, stream=stream)
                        return w, stats_b(*head_b, *inst.tail(wide), stream=stream)
                    cw, cb = step("%d %s %s counters (b)" % (k, name, form), args.limit, seeded_counters)
                    cb = cb.as_dict()
                    o["counters_world_as_instance"], o["counters_seeded"] = ca, cb
                    o["counters_world_single_level"] = {f: int(getattr(cw, f)) for f, _ in cw._fields_}
                    o["per_ray_world_as_instance"], o["per_ray_seeded"] = per_ray(ca, count), per_ray(cb, count)
                    out[form] = o
                return out
            row["primary"] = batch("primary", n, False, d_rays)
            res = d_res_a.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()     # (the wide path (a)'s primary records: the AO rays' origins)
            d_ao = step("%d ao upload" % k, args.limit, lambda: up(host_ao_rays(rays, res, na, 7, radius=args.ao_radius)))
            row["ao"] = batch("ao", na, True, d_ao)
            assert nt.trace_status() == 0, "traversal stack overflow"
            emit(row)

    if "forest" in args.parts:
        soup = step("soup1000 BLAS", args.limit, lambda: Blas(soup_tri, soup_pos, stream))
        rng = np.random.default_rng(4096)
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        from instanced_bench import transforms
        t = step("forest tlas", args.limit, lambda: Tlas(soup, transforms(rotations(4096, rng), (g - 7.5) * 30.0), stream))
        cam = dict(eye=(40.0, 60.0, -420.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, far=2000.0)
        rays, _ = scenes.primary_rays(cam, args.width, args.height)
        n, na = rays.shape[0], args.ao_rays
        d_rays = up(rays)
        d_res, d_ids, d_res2, d_ids2 = zeros(16 * max(n, na)), zeros(4 * max(n, na)), zeros(16 * max(n, na)), zeros(4 * max(n, na))
        t.trace(n, False, d_rays, d_res, d_ids)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()[:16 * n].view(nt.RESULT_DTYPE).copy()
        ao = host_ao_rays(rays, res, na, 7)
        d_ao = up(ao)
        vis = nt.InstanceVisibility(0, 0, 0x7FFFFFFF)       # refuses nothing, and puts ntr_trace_instanced_masked onto the masked loop
        row = {"part": "forest", "instances": t.n, "primary_rays": n, "ao_rays": na, "reps": args.reps, "warmup": args.warmup}
        for name, count, any_hit, d_r, host in (("primary", n, False, d_rays, rays), ("ao", na, True, d_ao, ao)):
            seed = np.zeros(count, nt.RESULT_DTYPE)
            seed["id"], seed["t"] = -1, host["tmax"]
            d_seed = up(seed)

            def run():
                sm, ss, su = [], [], []
                for _ in range(args.warmup + args.reps):              # alternated
                    sm.append(t.trace_masked(count, any_hit, d_r, d_res, d_ids, vis))
                    ss.append(nt.trace_instanced_seeded(count, any_hit, d_r.data_ptr(), d_seed.data_ptr(), 0, d_res2.data_ptr(), d_ids2.data_ptr(),
                                                        *t.args(count, any_hit, d_r, d_res2, d_ids2)[5:], vis=vis, stream=stream))
                    su.append(t.trace(count, any_hit, d_r, d_res, d_ids))
                torch.cuda.synchronize()
                same = bool(torch.equal(d_res[:16 * count], d_res2[:16 * count]) and torch.equal(d_ids[:4 * count], d_ids2[:4 * count]))
                return sm[args.warmup:], ss[args.warmup:], su[args.warmup:], same
            sm, ss, su, same = step("forest " + name, args.limit, run)
            row[name] = {"masked": spread(sm, count), "seeded_all_miss": spread(ss, count), "unmasked": spread(su, count), "bytes_equal": same}
            row[name]["seeded_over_masked"] = row[name]["seeded_all_miss"]["ms_median"] / row[name]["masked"]["ms_median"]
        assert nt.trace_status() == 0, "traversal stack overflow"
        emit(row)

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
