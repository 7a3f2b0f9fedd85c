#!/usr/bin/env python3
"""Decision gate of the certain-step prologue (trace_kernels.hip uniform_prologue<.., CERTAIN>): how many wave-uniform prologue steps
does a wave of the bench frame take, and in what share of them is EVERY live lane certain -- its origin inside one child box, the
sibling out of its reach -- so that the step needs no quotient?  CPU replay: atrium-262k SAH tree (leaf prefs 1, 1), the 1080p primary
batch in PixelTable order traced by the oracle, the AO batches restated from its records (tests/np_raygen.py, eight samples of length
5 per pixel: a wave is eight neighbouring pixels), rays grouped into waves of 64 in buffer order.  The prologue is replayed as the
kernel runs it: while every live lane holds the same inner node; the exact step is the float32 slab test, the rule is
tests/np_certain_step.py (the restatement the CPU test checks against the exact test).  Break-even is a certain share of about 35 %
(about 25 VALU of test against about 63 saved).  One JSON line per batch group; no GPU needed.
  AO_BATCHES=all|<n>   how many of the 16 AO batches to replay (default all)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from oracle import oracle  # noqa: E402
import np_raygen  # noqa: E402
import np_certain_step as cs  # noqa: E402

F = np.float32
SENT = 0x76543210
DEPTH = 48
GIVE_UP_AFTER = 2   # kCertainGiveUpAfter of the kernel


def replay(nodes, rays):
    """Per wave of 64 rays in buffer order: prologue steps, steps in which every live lane is certain, and the same under the kernel's
    give-up policy (steps that take the certain path / steps that pay the test for nothing)."""
    nodes_f = np.frombuffer(np.ascontiguousarray(nodes).tobytes(), dtype=F)
    nodes_i = nodes_f.view(np.int32)
    n = rays.shape[0]
    W = (n + 63) // 64
    pad = W * 64 - n

    def col(k, fill):
        return np.concatenate([rays[k].astype(F), np.full(pad, fill, dtype=F)]).reshape(W, 64)
    o = [col(k, 1.0) for k in ("ox", "oy", "oz")]
    d = [col(k, 1.0) for k in ("dx", "dy", "dz")]
    tmin, tmax = col("tmin", 0.0), col("tmax", -1.0)
    node = np.where(tmin < tmax, 0, SENT).astype(np.int64)
    stack = np.zeros((W, 64, DEPTH), dtype=np.int32)
    sp = np.zeros((W, 64), dtype=np.int64)
    seg_lo, seg_hi = cs.segment(o, d, tmax)
    eligible = ((tmin == 0) | (node == SENT)).all(1)      # the wave-uniform precondition (tmin == 0 on every live lane)
    steps = np.zeros(W, dtype=np.int64)
    cert = np.zeros(W, dtype=np.int64)
    lane_steps = lane_cert = 0
    taken = np.zeros(W, dtype=np.int64)       # under the give-up policy: steps on the certain path
    wasted = np.zeros(W, dtype=np.int64)      # ... steps that paid the test and then ran the exact step
    trying = eligible.copy()
    misses = np.zeros(W, dtype=np.int64)
    active = np.ones(W, dtype=bool)
    with np.errstate(all="ignore"):
        while True:
            live = node != SENT
            first = np.argmax(live, axis=1)
            unode = node[np.arange(W), first]
            ok = live.any(1) & ((node == unode[:, None]) | ~live).all(1) & (unode >= 0) & (unode < SENT)
            active &= ok
            ws = np.nonzero(active)[0]
            if ws.size == 0:
                break
            b = (unode[ws] // 4)[:, None]
            pl = [nodes_f[b + k] for k in range(12)]     # planes, broadcast over the wave's lanes
            lv = live[ws]
            oo = [a[ws] for a in o]
            dd = [a[ws] for a in d]
            box0 = (pl[0], pl[1], pl[2], pl[3], pl[8], pl[9])
            box1 = (pl[4], pl[5], pl[6], pl[7], pl[10], pl[11])
            i0, mn0 = cs.exact_accept(box0, oo, dd, tmin[ws], tmax[ws])
            i1, mn1 = cs.exact_accept(box1, oo, dd, tmin[ws], tmax[ws])
            certain, take0 = cs.certain(box0, box1, oo, [a[ws] for a in seg_lo], [a[ws] for a in seg_hi])
            assert not (certain & lv & ((i0 != take0) | (i1 == take0))).any(), "the rule disagrees with the exact test"
            wave_cert = (certain | ~lv).all(1) & eligible[ws]
            steps[ws] += 1
            cert[ws] += wave_cert
            lane_steps += int(lv.sum())
            lane_cert += int((certain & lv).sum())
            tr = trying[ws]
            taken[ws] += tr & wave_cert
            wasted[ws] += tr & ~wave_cert
            misses[ws] = np.where(tr & ~wave_cert, misses[ws] + 1, 0)
            trying[ws] = tr & (misses[ws] < GIVE_UP_AFTER)
            # the exact step (inner_advance)
            c0 = nodes_i[b + 12].astype(np.int64) + np.zeros((1, 64), dtype=np.int64)
            c1 = nodes_i[b + 13].astype(np.int64) + np.zeros((1, 64), dtype=np.int64)
            swp = i1 & (~i0 | (mn0 > mn1))
            near, far = np.where(swp, c1, c0), np.where(swp, c0, c1)
            both = i0 & i1 & lv
            nd, s_, st_ = node[ws], sp[ws], stack[ws]
            assert int(s_.max()) < DEPTH - 1
            wi, li = np.nonzero(both)
            st_[wi, li, s_[wi, li]] = far[wi, li]
            s_[wi, li] += 1
            none = ~(i0 | i1) & lv
            nd = np.where((i0 | i1) & lv, near, nd)
            wi, li = np.nonzero(none)
            has = s_[wi, li] > 0
            s_[wi[has], li[has]] -= 1
            nd[wi, li] = np.where(has, st_[wi, li, s_[wi, li]], SENT)
            node[ws], sp[ws], stack[ws] = nd, s_, st_
    return dict(steps=steps, cert=cert, taken=taken, wasted=wasted, eligible=eligible, lane_steps=lane_steps, lane_cert=lane_cert,
                live_waves=(col("tmax", -1.0) > tmin).any(1))


def summarise(name, parts):
    cat = lambda k: np.concatenate([p[k] for p in parts])
    lw = cat("live_waves")
    steps, cert, taken, wasted = cat("steps")[lw], cat("cert")[lw], cat("taken")[lw], cat("wasted")[lw]
    tot = int(steps.sum())
    ls, lc = sum(p["lane_steps"] for p in parts), sum(p["lane_cert"] for p in parts)
    return dict(batch=name, waves=int(lw.sum()), eligible_waves=float(cat("eligible")[lw].mean()), prologue_steps=tot,
                steps_per_wave_mean=float(steps.mean()), steps_per_wave_p10_p50_p90=[int(x) for x in np.percentile(steps, (10, 50, 90))],
                certain_step_share=float(cert.sum() / max(tot, 1)), lane_certain_share=float(lc / max(ls, 1)),
                policy_give_up_after=GIVE_UP_AFTER, policy_certain_path_share=float(taken.sum() / max(tot, 1)),
                policy_wasted_test_share=float(wasted.sum() / max(tot, 1)))


def main():
    tri, pos, cam = scenes.atrium()
    bvh = nt.sah_build(tri, pos, 1, 1)
    w, h, ns, radius, batch_rays = 1920, 1080, 8, 5.0, 1 << 20
    prim, _ = scenes.primary_rays(cam, w, h)
    print(json.dumps(summarise("primary", [replay(bvh.nodes, prim)])), flush=True)
    res, _ = oracle.trace(bvh.nodes, bvh.woop, bvh.tri_index, prim, any_hit=False, threads=os.cpu_count() or 1)
    normals = scenes.tri_normals(tri, pos)
    per = batch_rays // ns
    firsts = list(range(0, w * h, per))
    want = os.environ.get("AO_BATCHES", "all")
    if want != "all":
        firsts = firsts[:: max(1, len(firsts) // int(want))][: int(want)]
    parts = []
    for first in firsts:
        cnt = min(per, w * h - first)
        o, d, tmax = np_raygen.ao_rays(prim, res, normals, ns, radius, 0xFFF2D5E4, first, cnt)
        rays = np.zeros(cnt * ns, dtype=prim.dtype)
        for i, k in enumerate(("ox", "oy", "oz")):
            rays[k] = o[:, i].astype(F)
        for i, k in enumerate(("dx", "dy", "dz")):
            rays[k] = d[:, i].astype(F)
        rays["tmin"], rays["tmax"] = 0.0, tmax.astype(F)
        parts.append(replay(bvh.nodes, rays))
        print(json.dumps(dict(summarise("ao batch at pixel %d" % first, parts[-1:]))), flush=True)
    print(json.dumps(summarise("ao (%d of %d batches)" % (len(firsts), (w * h + per - 1) // per), parts)), flush=True)


if __name__ == "__main__":
    main()
