"""numpy spec of the FAST path of the two-level trace over 4-wide trees: ntr_instanced_wide_validate, ntr_trace_instanced_wide_fast and
ntr_trace_instanced_wide_fast_stats (test helper; this docstring is the normative text).  It is tests/np_instanced_fast.py, point for
point, over the wide buffers of tests/np_instanced_wide.py.

EXTENSION: the reference has neither instancing nor wide trees.  The device (csrc/instanced_validate_kernels.hip,
csrc/trace_instanced_wide_body.h with NTR_TIW_FAST) equals validate() in both words and trace() in all four result words, the instance
id, the seven wide counters and the four counters below.

validate(wide_tlas_bytes, wide_pool_bytes) -> (withheld_tlas, withheld_pool).  np_instanced_fast's rule -- ntr_bvh_validate's for
FINITE, FASTDIV, NOTINY and ORDERED, stated as what is WITHHELD -- over EVERY 128-byte slot of a buffer: words 0..11 and 16..27 of a slot
are twelve (lo, hi) pairs; words 12..15 (the links) and 28..31 (the count) are not looked at.  Padding slots (k >= count: a copy of slot
0's box), empty slots, nodes no link reaches and slack behind the last wide BLAS count.  An empty buffer withholds nothing.
np_instanced_fast.granted(w) is what ntr_instanced_flags_read returns.

trace(flags, ...): the records and the counters are np_instanced_wide.trace's, or with a seed np_instanced_seeded.trace_wide's, called
as they are; plain division throughout.  The wide loop is then walked again in lockstep, all rays one step per iteration as a wave's
lanes take them, carrying np_instanced_fast's `nice` (level_nice: at the start from the world ray against flags[0], on entering an
instance from the object ray against flags[1], at the exit marker from the world ray against flags[0]).  A step of the walk is one
iteration of the DEVICE's wide loop: a wide node of either level, an entering link, a marker, or a triangle -- and a triangle step also
looks at word 0 of the row behind the triangle and pops when that is the terminator (unless an any-hit ray just ended), where
np_instanced_wide takes a step of its own for that row.  Wave w is rays [64 w, 64 w + 64); waveSteps, fastWaveSteps, niceStarts and
niceEntries are np_instanced_fast's.
"""
import numpy as np

import np_bvh_wide as bw
import np_instanced_fast as nfa
import np_instanced_masked as nm
import np_instanced_seeded as nsd
import np_instanced_wide as nw
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, TERM, _dot4, _smax, _smin, xform

FOUR = nfa.FOUR
FAST_COUNTERS = nfa.FAST_COUNTERS
WAVE = nfa.WAVE
granted = nfa.granted
level_nice = nfa.level_nice


# ---- validate -------------------------------------------------------------------------------------------------------------------------
def withheld_wide(nodes):
    """The withheld bits of one wide node buffer (any view of whole 128-byte slots; may be empty)."""
    w = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8).view(np.uint32).reshape(-1, 32)
    box = np.concatenate([w[:, 0:12], w[:, 16:28]], axis=1).view(F).astype(np.float64)      # NaN stays NaN, every float32 is exact
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


def validate(wide_tlas_bytes, wide_pool_bytes):
    """-> (withheld_tlas, withheld_pool): d_flags[0] and d_flags[1] after ntr_instanced_wide_validate."""
    return withheld_wide(wide_tlas_bytes), withheld_wide(wide_pool_bytes)


# ---- trace ----------------------------------------------------------------------------------------------------------------------------
def trace(flags, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit=False, inst_masks=None, ray_masks=None,
          ray_mask=0xFFFFFFFF, seed=None, seed_instance=-1):
    """flags: (withheld_tlas, withheld_pool).  wide_pool: np_instanced_wide.widen_pool's dict, or the wide pool's bytes.  seed: None
    (unseeded) or one record per ray as np_instanced_seeded takes it.
    -> (id int32, t float32, u float32, v float32, instance int32, counters dict, fast counters dict)"""
    if seed is None:
        out = nw.trace(wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask)
    else:
        out = nsd.trace_wide(seed, seed_instance, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks,
                             ray_mask)
    words, inst, fast = _walk(flags, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask, seed,
                              seed_instance)
    want = np.stack([np.ascontiguousarray(x).view(np.uint32) for x in out[:4]], axis=1)
    assert np.array_equal(words, want) and np.array_equal(inst, out[4]), "np_instanced_wide_fast: the lockstep walk left the spec's records"
    return out + (fast,)


def _walk(flags, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask, seed, seed_instance):
    """The wide loop in the device's iterations, carrying `nice`.  -> (record words (n, 4) uint32, instance int32, fast counters)"""
    w_tlas, w_pool = int(flags[0]), int(flags[1])

    def padded(buf):                                   # a zero node behind the extent: what a read beyond it gives
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        return np.concatenate([b, np.zeros(2 * nw.WIDE_BYTES, np.uint8)]).view(F), b.size
    tl, tl_bytes = padded(wide_tlas)
    wp, wp_bytes = padded(wide_pool["nodes"] if isinstance(wide_pool, dict) else wide_pool)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1)
    pw = np.concatenate([pw, np.zeros(64, np.uint8)]).view(F).reshape(-1, 4)   # zeros behind the extent: what a read beyond it gives
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(wide_records).view(np.uint32).reshape(-1, 16)
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
    w_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    w_ext = np.zeros(n, np.int64)
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
            raise RuntimeError("np_instanced_wide_fast: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

    def wide(idx, buf, byte):
        """np_bvh_wide's wide-node step for rays idx on the nodes at `byte` of buf (np_instanced_wide.trace's)."""
        b = byte // 4
        bi = buf.view(np.int32)
        rx, ry, rz, ex, ey, ez = (a[idx] for a in R)
        k_n = idx.size
        key = np.full((k_n, 4), np.inf, F)
        cand = np.zeros((k_n, 4), bool)
        links = np.zeros((k_n, 4), np.int64)
        for k in range(4):
            g = [buf[b + w] for w in bw.WBOX[k]]
            t0x, t1x = (g[0] - rx) / ex, (g[1] - rx) / ex
            t0y, t1y = (g[2] - ry) / ey, (g[3] - ry) / ey
            t0z, t1z = (g[4] - rz) / ez, (g[5] - rz) / ez
            mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
            mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
            links[:, k] = bi[b + bw.WLINK + k]
            cand[:, k] = (links[:, k] != 0) & (mn <= mx) & (mx >= tmin[idx]) & (mn <= tmax[idx])
            key[:, k] = mn
        order = np.lexsort((np.where(cand, np.arange(4), np.arange(4) + 4), np.where(cand, key + F(0), F(np.inf))), axis=1)
        c = cand.sum(axis=1)
        rows = np.arange(k_n)
        for pos in (3, 2, 1):                       # farthest first
            sel = c > pos
            push(idx[sel], links[rows[sel], order[sel, pos]])
        sel = c > 0
        node[idx[sel]] = links[rows[sel], order[sel, 0]]
        pop(idx[~sel])

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
                wide(k_top_inner, tl, np.minimum(node[k_top_inner], tl_bytes))
            if k_bot_inner.size:
                nd = node[k_bot_inner]
                o = w_off[k_bot_inner] + nd
                readable = (nd < w_ext[k_bot_inner]) & (o < nw.NO_NODE)
                wide(k_bot_inner, wp, np.where(readable, np.minimum(o, wp_bytes), wp_bytes))
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
                w_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                w_ext[k_enter] = rec[i, 14]
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
