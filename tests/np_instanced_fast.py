"""numpy spec of the FAST path of the two-level trace: ntr_instanced_validate, ntr_instanced_flags_read, ntr_trace_instanced_fast and
ntr_trace_instanced_fast_stats (test helper; this docstring is the normative text).

EXTENSION: the reference has no instancing.  The device (csrc/instanced_validate_kernels.hip, csrc/trace_instanced_body.h with
NTR_TI_FAST) equals validate() in both words and trace() in all four result words, the instance id, the eight counters of
np_instanced_masked and the four counters below.

validate(tlas_bytes, pool_bytes) -> (withheld_tlas, withheld_pool).  ntr_bvh_validate's rule (tests/np_bvh_validate.py) for FINITE,
FASTDIV, NOTINY and ORDERED, stated as what is WITHHELD, over EVERY 64-byte slot of a buffer -- a pool's slack and gaps too: words
0..11 of a slot are six (lo, hi) pairs; words 12..15 are not looked at.
  FINITE    withheld when some box float is not finite or has |x| >= 2^100
  FASTDIV   withheld when some box float has not |x| < 2^55 (a NaN has not)
  NOTINY    withheld when some box float is neither 0 nor of |x| >= 2^-93 (a NaN is neither)
  ORDERED   withheld when some pair has not lo <= hi
An empty buffer withholds nothing.  granted(w) = ~w & 15 is what ntr_instanced_flags_read returns.

trace(flags, ...): the records and the eight counters are np_instanced_masked.trace's, or with a seed np_instanced_seeded.trace's,
called as they are -- this spec adds nothing to them and uses plain division throughout; that the FAST quotient equals the division is
ntr_selftest_division's business.  The loop is then walked again in lockstep, all rays one step per iteration as a wave's lanes take
them, to carry one more per-ray state:
  nice      the ray's CURRENT form may take FAST on its CURRENT level.  level_nice(form, w) = not (w & FASTDIV) and every direction
            component has 2^-40 <= |d| <= 2^20 and every origin component has 2^-36 <= |o| < 2^55 or, when w does not withhold NOTINY,
            is +-0.
  start     nice = level_nice(world ray, flags[0])
  entering  (a step that enters instance i) after the transform: nice = level_nice(object ray, flags[1])
  leaving   (the exit marker) nice = level_nice(world ray, flags[0])
A step of the lockstep walk is one iteration of the device's loop.  It is the spec's step with one difference that no record and no
counter of the eight can see: a triangle step also looks at word 0 of the row behind the triangle and pops when that is the terminator
(unless an any-hit ray just ended), where np_instanced_masked takes a step of its own for that row.
Wave w is rays [64 w, 64 w + 64).  A ray is live while its node is not the sentinel.
  waveSteps      iterations with at least one live ray in the wave, summed over the waves
  fastWaveSteps  those in which no live ray of the wave has nice == false: the wave runs the FAST form of the step
  niceStarts     rays that start live and nice
  niceEntries    entering steps that entered and leave the ray nice
"""
import numpy as np

import np_instanced_masked as nm
import np_instanced_seeded as nsd
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, TERM, _dot4, _smax, _smin, xform

FOUR = FINITE | FASTDIV | NOTINY | ORDERED
FAST_COUNTERS = ("waveSteps", "fastWaveSteps", "niceStarts", "niceEntries")
WAVE = 64


# ---- validate -------------------------------------------------------------------------------------------------------------------------
def withheld(nodes):
    """The withheld bits of one node buffer (any view of whole 64-byte slots; may be empty)."""
    w = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8).view(np.uint32).reshape(-1, 16)
    box = w[:, :12].view(F).astype(np.float64)         # NaN stays NaN, every float32 is exact
    mag = np.abs(box)
    bits = 0
    with np.errstate(invalid="ignore"):
        if not bool(np.all(np.isfinite(box) & (mag < 2.0 ** 100))):
            bits |= FINITE
        if not bool(np.all(mag < 2.0 ** 55)):
            bits |= FASTDIV
        if not bool(np.all((box == 0.0) | (mag >= 2.0 ** -93))):
            bits |= NOTINY
        if not bool(np.all(box[:, 0::2] <= box[:, 1::2])):
            bits |= ORDERED
    return bits


def validate(tlas_bytes, pool_bytes):
    """-> (withheld_tlas, withheld_pool): d_flags[0] and d_flags[1] after ntr_instanced_validate."""
    return withheld(tlas_bytes), withheld(pool_bytes)


def granted(w):
    return ~int(w) & FOUR


# ---- nice -----------------------------------------------------------------------------------------------------------------------------
def level_nice(form, w):
    """form: six float32 arrays ox, oy, oz, dx, dy, dz; w: the level's withheld bits -> bool array."""
    ok = np.full(form[0].shape, not (int(w) & FASTDIV))
    zero_ok = not (int(w) & NOTINY)
    with np.errstate(invalid="ignore"):
        for o in form[:3]:
            a = np.abs(o.astype(np.float64))
            ok &= ((a >= 2.0 ** -36) & (a < 2.0 ** 55)) | (zero_ok & (o == 0))
        for d in form[3:]:
            a = np.abs(d.astype(np.float64))
            ok &= (a >= 2.0 ** -40) & (a <= 2.0 ** 20)
    return ok


# ---- trace ----------------------------------------------------------------------------------------------------------------------------
def trace(flags, tlas_nodes, root_link, records, pool, rays, any_hit=False, inst_masks=None, ray_masks=None, ray_mask=0xFFFFFFFF, seed=None,
          seed_instance=-1):
    """flags: (withheld_tlas, withheld_pool).  seed: None (unseeded) or one record per ray as np_instanced_seeded takes it.
    -> (id int32, t float32, u float32, v float32, instance int32, counters dict, fast counters dict)"""
    if seed is None:
        out = nm.trace(tlas_nodes, root_link, records, pool, rays, any_hit, inst_masks, ray_masks, ray_mask)
    else:
        out = nsd.trace(seed, seed_instance, tlas_nodes, root_link, records, pool, rays, any_hit, inst_masks, ray_masks, ray_mask)
    words, inst, fast = _walk(flags, tlas_nodes, root_link, records, pool, rays, any_hit, inst_masks, ray_masks, ray_mask, seed, seed_instance)
    want = np.stack([np.ascontiguousarray(x).view(np.uint32) for x in out[:4]], axis=1)
    assert np.array_equal(words, want) and np.array_equal(inst, out[4]), "np_instanced_fast: the lockstep walk left the spec's records"
    return out + (fast,)


def _walk(flags, tlas_nodes, root_link, records, pool, rays, any_hit, inst_masks, ray_masks, ray_mask, seed, seed_instance):
    """The loop in the device's iterations, carrying `nice`.  -> (record words (n, 4) uint32, instance int32, fast counters)"""
    w_tlas, w_pool = int(flags[0]), int(flags[1])
    tl = np.ascontiguousarray(tlas_nodes).view(np.uint8).reshape(-1)
    tl = np.concatenate([tl, np.zeros(64, np.uint8)]).view(F)        # (an empty buffer when N == 1)
    pn = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).view(F)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1)
    pw = np.concatenate([pw, np.zeros(64, np.uint8)]).view(F).reshape(-1, 4)   # zeros behind the extent: what a read beyond it gives
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    M = np.full(num_inst, 0xFFFFFFFF, np.uint32) if inst_masks is None else np.ascontiguousarray(inst_masks).view(np.uint32).reshape(-1)
    m = np.full(n, int(ray_mask) & 0xFFFFFFFF, np.uint32) if ray_masks is None else np.ascontiguousarray(ray_masks).view(np.uint32).reshape(-1)
    W = [rays[k].astype(F) for k in ("ox", "oy", "oz", "dx", "dy", "dz")]
    R = [w.copy() for w in W]
    tmin = rays["tmin"].astype(F)
    tmax = rays["tmax"].astype(F).copy()
    res = np.zeros((n, 4), np.uint32)
    res[:, 0] = 0xFFFFFFFF
    res[:, 1] = tmax.view(np.uint32)
    res_inst = np.full(n, -1, np.int32)
    node = np.full(n, int(root_link), np.int64)
    if seed is not None:
        sw = nsd.seed_words(seed)
        assert sw.shape[0] == n
        res = sw.copy()
        s_hit = sw[:, 0].view(np.int32) != -1
        tmax = np.where(s_hit, sw[:, 1].view(F), tmax).astype(F)
        res_inst = np.where(s_hit, int(np.int32(seed_instance)), -1).astype(np.int32)
        if any_hit:
            node[s_hit] = SENTINEL
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL
    inst = np.full(n, -1, np.int64)
    n_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    nice = level_nice(W, w_tlas)
    fast = dict.fromkeys(FAST_COUNTERS, 0)
    fast["niceStarts"] = int(((node != SENTINEL) & nice).sum())
    waves = -(-n // WAVE)

    def by_wave(x):
        p = np.zeros(waves * WAVE, bool)
        p[:n] = x
        return p.reshape(waves, WAVE).any(axis=1)

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_fast: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

    def inner(idx, buf, base):
        b = (base + node[idx]) // 4
        g = lambda k: buf[b + k]
        rx, ry, rz, ex, ey, ez = (a[idx] for a in R)

        def box(lox, hix, loy, hiy, loz, hiz):
            t0x, t0y, t0z = (lox - rx) / ex, (loy - ry) / ey, (loz - rz) / ez
            t1x, t1y, t1z = (hix - rx) / ex, (hiy - ry) / ey, (hiz - rz) / ez
            mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
            mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
            return mn, mx
        mn0, mx0 = box(g(0), g(1), g(2), g(3), g(8), g(9))
        mn1, mx1 = box(g(4), g(5), g(6), g(7), g(10), g(11))
        c0 = buf.view(np.int32)[b + 12].astype(np.int64)
        c1 = buf.view(np.int32)[b + 13].astype(np.int64)
        i0 = (mn0 <= mx0) & (mx0 >= tmin[idx]) & (mn0 <= tmax[idx])
        i1 = (mn1 <= mx1) & (mx1 >= tmin[idx]) & (mn1 <= tmax[idx])
        swp = i1 & (~i0 | (mn0 > mn1))
        near, far = np.where(swp, c1, c0), np.where(swp, c0, c1)
        both = i0 & i1
        push(idx[both], far[both])
        some = i0 | i1
        node[idx[some]] = near[some]
        pop(idx[~some])

    with np.errstate(all="ignore"):
        while True:
            act = node != SENTINEL
            if not act.any():
                break
            live_w = by_wave(act)
            fast["waveSteps"] += int(live_w.sum())
            fast["fastWaveSteps"] += int((live_w & ~by_wave(act & ~nice)).sum())
            is_exit = act & (node == EXIT_MARKER)
            is_inner = act & (node >= 0) & (node < SENTINEL)
            top = inst < 0
            k_top_inner = np.flatnonzero(is_inner & top)
            k_enter = np.flatnonzero(act & (node < 0) & top)
            k_bot_inner = np.flatnonzero(is_inner & ~top)
            k_tri = np.flatnonzero(act & (node < 0) & ~top)
            k_exit = np.flatnonzero(is_exit)
            k_other = np.flatnonzero(act & (node > SENTINEL) & ~is_exit)      # a positive word that is no link: dropped
            if k_top_inner.size:
                inner(k_top_inner, tl, 0)
            if k_bot_inner.size:
                inner(k_bot_inner, pn, n_off[k_bot_inner])
            if k_other.size:
                pop(k_other)
            if k_enter.size:
                i = ~node[k_enter]
                in_range = (i >= 0) & (i < num_inst)
                pop(k_enter[~in_range])
                k_enter, i = k_enter[in_range], i[in_range]
                seen = nm.visible(M, m, i, k_enter)
                pop(k_enter[~seen])
                k_enter, i = k_enter[seen], i[seen]
            if k_enter.size:
                push(k_enter, EXIT_MARKER)
                m_i = rec_f[i, :12]
                o = xform(m_i, W[0][k_enter], W[1][k_enter], W[2][k_enter], 1)
                d = xform(m_i, W[3][k_enter], W[4][k_enter], W[5][k_enter], 0)
                for a in range(3):
                    R[a][k_enter] = o[a]
                    R[3 + a][k_enter] = d[a]
                inst[k_enter] = i
                n_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                node[k_enter] = 0
                nice[k_enter] = level_nice([q[k_enter] for q in R], w_pool)
                fast["niceEntries"] += int(nice[k_enter].sum())
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                pop(k_exit)
                nice[k_exit] = level_nice([q[k_exit] for q in W], w_tlas)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = nm.is_terminator(pw_u, row)
                pop(k_tri[term])
                ti, a = k_tri[~term], row[~term]
                if ti.size:
                    z, u4, v4 = pw[a], pw[a + 1], pw[a + 2]
                    rx, ry, rz, ex, ey, ez = (q[ti] for q in R)
                    one, zero = np.full_like(rx, F(1)), np.zeros_like(rx)
                    Oz = z[:, 3] - rx * z[:, 0] - ry * z[:, 1] - rz * z[:, 2]
                    ooDz = F(1) / _dot4(z, ex, ey, ez, zero)
                    t = Oz * ooDz
                    ok = (t > tmin[ti]) & (t < tmax[ti])
                    u = _dot4(u4, rx, ry, rz, one) + t * _dot4(u4, ex, ey, ez, zero)
                    ok &= u >= 0
                    v = _dot4(v4, rx, ry, rz, one) + t * _dot4(v4, ex, ey, ez, zero)
                    ok &= (v >= 0) & ((u + v) <= F(1))
                    tt = np.where(ok, t, FLT_MAX)
                    acc = (tt > tmin[ti]) & (tt < tmax[ti])
                    h = ti[acc]
                    tmax[h] = tt[acc]
                    res[h, 0] = tri_index[a[acc]].view(np.uint32)
                    res[h, 1] = tt[acc].astype(F).view(np.uint32)
                    res[h, 2] = np.where(ok[acc], u[acc], F(0)).astype(F).view(np.uint32)
                    res[h, 3] = np.where(ok[acc], v[acc], F(0)).astype(F).view(np.uint32)
                    res_inst[h] = inst[h]
                    ended = acc if any_hit else np.zeros_like(acc)
                    node[ti[ended]] = SENTINEL
                    # the word behind the triangle came with it: a terminator there ends the leaf in this iteration
                    behind = ~ended & (pw_u[a + 3, 0] == TERM)
                    pop(ti[behind])
                    go = ~ended & ~behind
                    node[ti[go]] -= 3
    return res, res_inst, fast
