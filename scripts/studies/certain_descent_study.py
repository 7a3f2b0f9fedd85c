#!/usr/bin/env python3
"""Decision gate of the carried certain descent (trace_kernels.hip uniform_prologue, NTR_TRACE_CERTAIN_DESCENT): of the certain steps a
wave of the bench frame takes under the give-up policy, how many are CARRIED -- every live lane certain, all of them inside the same
child, that child an inner node -- so that the wave can keep the node in a scalar register and go on to the next record without
writing the child to the lanes and reading it back?  The replay is certain_step_study.py's (same tree, same batches, same waves, the
rule of tests/np_certain_step.py); per wave it adds the carried steps, the runs they form (a run ends where the lanes part, a lane is
uncertain or the child is a leaf) and the runs entered again after an exact step.  The predicted saving is 50 instructions per carried
step (about 75 issued by the per-step path against about 25).  Gate: fewer than 4 carried steps per AO wave and the kernel is not worth
building.  One JSON line per batch group; no GPU needed.
  AO_BATCHES=all|<n>   how many of the 16 AO batches to replay (default all)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import certain_step_study as base  # noqa: E402  (puts the repository and tests/ on the path)
import ntrace_amd as nt  # noqa: E402
from ntrace_amd import scenes  # noqa: E402
from oracle import oracle  # noqa: E402
import np_raygen  # noqa: E402
import np_certain_step as cs  # noqa: E402

F = np.float32
SENT, DEPTH, GIVE_UP_AFTER = base.SENT, base.DEPTH, base.GIVE_UP_AFTER
SAVED_PER_CARRIED_STEP = 50


def replay(nodes, rays):
    """Per wave of 64 rays in buffer order, under the kernel's give-up policy: prologue steps, certain steps taken, carried steps, runs of
    carried steps and the runs that begin after the wave has taken an exact step."""
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
    trying = ((tmin == 0) | (node == SENT)).all(1)
    z = lambda: np.zeros(W, dtype=np.int64)
    steps, taken, carried, runs, reentered, misses, longest, current = z(), z(), z(), z(), z(), z(), z(), z()
    in_run = np.zeros(W, dtype=bool)
    exact_seen = np.zeros(W, dtype=bool)
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
            pl = [nodes_f[b + k] for k in range(12)]
            lv = live[ws]
            oo = [a[ws] for a in o]
            dd = [a[ws] for a in d]
            box0 = (pl[0], pl[1], pl[2], pl[3], pl[8], pl[9])
            box1 = (pl[4], pl[5], pl[6], pl[7], pl[10], pl[11])
            i0, mn0 = cs.exact_accept(box0, oo, dd, tmin[ws], tmax[ws])
            i1, mn1 = cs.exact_accept(box1, oo, dd, tmin[ws], tmax[ws])
            certain, take0 = cs.certain(box0, box1, oo, [a[ws] for a in seg_lo], [a[ws] for a in seg_hi])
            assert not (certain & lv & ((i0 != take0) | (i1 == take0))).any(), "the rule disagrees with the exact test"
            tr = trying[ws]
            wave_cert = (certain | ~lv).all(1) & tr
            c0, c1 = nodes_i[b + 12].astype(np.int64)[:, 0], nodes_i[b + 13].astype(np.int64)[:, 0]
            all0, all1 = (take0 | ~lv).all(1), (~take0 | ~lv).all(1)
            child = np.where(all0, c0, c1)
            carry = wave_cert & (all0 | all1) & (child > 0) & (child < SENT)
            steps[ws] += 1
            taken[ws] += wave_cert
            carried[ws] += carry
            start = carry & ~in_run[ws]
            runs[ws] += start
            reentered[ws] += start & exact_seen[ws]
            current[ws] = np.where(carry, current[ws] + 1, 0)
            longest[ws] = np.maximum(longest[ws], current[ws])
            in_run[ws] = carry
            exact_seen[ws] |= ~wave_cert
            misses[ws] = np.where(tr & ~wave_cert, misses[ws] + 1, 0)
            trying[ws] = tr & (misses[ws] < GIVE_UP_AFTER)
            # the step itself (inner_advance; a certain step's outcome is the same)
            c0l, c1l = c0[:, None] + np.zeros((1, 64), dtype=np.int64), c1[:, None] + np.zeros((1, 64), dtype=np.int64)
            swp = i1 & (~i0 | (mn0 > mn1))
            near, far = np.where(swp, c1l, c0l), np.where(swp, c0l, c1l)
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
    return dict(steps=steps, taken=taken, carried=carried, runs=runs, reentered=reentered, longest=longest,
                live_waves=(col("tmax", -1.0) > tmin).any(1))


def summarise(name, parts):
    cat = lambda k: np.concatenate([p[k] for p in parts])
    lw = cat("live_waves")
    steps, taken, carried, runs, reentered, longest = (cat(k)[lw] for k in ("steps", "taken", "carried", "runs", "reentered", "longest"))
    return dict(batch=name, waves=int(lw.sum()), steps_per_wave=float(steps.mean()), certain_steps_taken_per_wave=float(taken.mean()),
                carried_steps_per_wave=float(carried.mean()), carried_per_wave_p10_p50_p90=[int(x) for x in np.percentile(carried, (10, 50, 90))],
                carried_share_of_taken=float(carried.sum() / max(int(taken.sum()), 1)), runs_per_wave=float(runs.mean()),
                runs_reentered_after_exact_step_per_wave=float(reentered.mean()), waves_with_reentry=float((reentered > 0).mean()),
                longest_run_mean=float(longest.mean()), predicted_instructions_saved_per_wave=float(SAVED_PER_CARRIED_STEP * carried.mean()))


def main():
    tri, pos, cam = scenes.atrium()
    bvh = nt.sah_build(tri, pos, 1, 1)
    w, h, ns, radius, batch_rays = 1920, 1080, 8, 5.0, 1 << 20
    prim, _ = scenes.primary_rays(cam, w, h)
    print(json.dumps(summarise("primary (as with NTR_TRACE_CERTAIN_STEPS=2)", [replay(bvh.nodes, prim)])), flush=True)
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
        print(json.dumps(summarise("ao batch at pixel %d" % first, parts[-1:])), flush=True)
    print(json.dumps(summarise("ao (%d of %d batches)" % (len(firsts), (w * h + per - 1) // per), parts)), flush=True)


if __name__ == "__main__":
    main()
