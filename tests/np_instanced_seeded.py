"""numpy spec of the seeded two-level trace: ntr_trace_instanced_seeded, ntr_trace_instanced_seeded_stats and, over 4-wide trees,
ntr_trace_instanced_wide_seeded, ntr_trace_instanced_wide_seeded_stats (test helper; this docstring is the normative text).

EXTENSION: the reference has no instancing.  The device (csrc/trace_instanced_body.h with NTR_TI_SEEDED, csrc/trace_instanced_wide_body.h
with SEEDED) equals trace() and trace_wide() bit for bit in all four result words and the instance id, and in every counter.

Use.  A static world plus moving instances: the world is one BLAS of the pool in its own space, traced by the single-level kernel
(ntr_trace_bvh on the BLAS's range of the pool); its records SEED the two-level trace over the instances, which therefore starts with
tmax at the world hit, keeps the world hit where no instance is nearer, and never starts an any-hit ray that the world occludes.

Rule.  trace(seed, seed_instance, ...) is np_instanced_masked.trace with another initial state; trace_wide(seed, seed_instance, ...)
is np_instanced_wide.trace with the same change.  seed is one result record per ray, four words (id, t, w2, w3); seed_instance is any
int32 and is stored verbatim.
  - s_hit = seed.id != -1.
  - tmax0 = seed.t if s_hit, else ray.tmax.
  - The hit record starts as the seed's four words, verbatim.
  - The instance starts as seed_instance if s_hit, else -1.
  - !(tmin < tmax0): no traversal (the degenerate rule, applied to tmax0).
  - any hit and s_hit: no traversal.
  - Everything else is the unseeded loop from that state, unchanged: the mask rule, the exit marker, the stack of 104, the counters.  A
    hit that the loop accepts overwrites all four words and the instance, exactly as in the unseeded trace.
  - A ray whose traversal accepts nothing ends with the seed's four words verbatim, w2 and w3 included -- they are not interpreted -- and
    this holds for a seed that is a miss too: its t is stored as the seed has it, not as the ray has it.
  - seed.t is taken as it is: a NaN, an infinity or a negative t makes the ray degenerate or not by the comparison above and nothing
    else.  Whatever the seed holds, nothing outside the buffers is read.
Counters: np_instanced_masked's eight; numHits counts the final records with id != -1, seeds that stayed among them.
Algorithmic bytes: the unseeded formula plus 16 numRays for the seed read.
"""
import numpy as np

import np_bvh_wide as bw
import np_instanced_masked as nm
import np_instanced_wide as nw
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, _dot4, _smax, _smin, xform
from np_instanced_masked import COUNTERS, is_terminator, visible

WIDE_BYTES = bw.WIDE_BYTES
NO_NODE = nw.NO_NODE


def algorithmic_bytes(c, instance_masks=False, ray_masks=False):
    return nm.algorithmic_bytes(c, instance_masks, ray_masks) + 16 * c["numRays"]


def algorithmic_bytes_wide(c, instance_masks=False, ray_masks=False):
    return nw.algorithmic_bytes(c, instance_masks, ray_masks) + 16 * c["numRays"]


def seed_words(seed):
    """A seed in any layout of 16 bytes per ray (nt.RESULT_DTYPE, (n, 4) words) as (n, 4) uint32."""
    return np.ascontiguousarray(seed).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, 4)


def seed_of(ids, t, w2=0, w3=0):
    """(n, 4) uint32 seed words from ids, float32 t and two more words."""
    ids = np.asarray(ids, np.int32)
    s = np.zeros((ids.shape[0], 4), np.uint32)
    s[:, 0] = ids.view(np.uint32)
    s[:, 1] = np.ascontiguousarray(np.broadcast_to(np.asarray(t, F), ids.shape)).view(np.uint32)
    s[:, 2], s[:, 3] = w2, w3
    return s


def trace(seed, seed_instance, tlas_nodes, root_link, records, pool, rays, any_hit=False, inst_masks=None, ray_masks=None, ray_mask=0xFFFFFFFF):
    """-> (id int32, t float32, u float32, v float32, instance int32, counters dict)"""
    return _trace(False, seed, seed_instance, tlas_nodes, root_link, records, pool, None, rays, any_hit, inst_masks, ray_masks, ray_mask, None)


def trace_wide(seed, seed_instance, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit=False, inst_masks=None, ray_masks=None,
               ray_mask=0xFFFFFFFF, probe=None):
    """wide_pool: np_instanced_wide.widen_pool's dict, or the wide pool's bytes.  -> as trace()"""
    return _trace(True, seed, seed_instance, wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask,
                  probe)


# ---- the two loops restated with a seeded initial state: np_instanced_masked.trace and np_instanced_wide.trace --------------------------
def _trace(wide_form, seed, seed_instance, tlas_nodes, root_link, records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask, probe):
    def padded(buf, pad):                              # zeros behind the extent: what a read beyond it gives
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        return np.concatenate([b, np.zeros(pad, np.uint8)]).view(F), b.size
    if wide_form:
        tl, tl_bytes = padded(tlas_nodes, 2 * WIDE_BYTES)
        bn, bn_bytes = padded(wide_pool["nodes"] if isinstance(wide_pool, dict) else wide_pool, 2 * WIDE_BYTES)
    else:
        tl, tl_bytes = padded(tlas_nodes, 64)          # (an empty buffer when N == 1)
        bn = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).view(F)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    M = np.full(num_inst, 0xFFFFFFFF, np.uint32) if inst_masks is None else np.ascontiguousarray(inst_masks).view(np.uint32).reshape(-1)
    m = np.full(n, int(ray_mask) & 0xFFFFFFFF, np.uint32) if ray_masks is None else np.ascontiguousarray(ray_masks).view(np.uint32).reshape(-1)
    assert M.shape[0] == num_inst and m.shape[0] == n
    sw = seed_words(seed)
    assert sw.shape[0] == n
    seed_instance = int(np.int32(seed_instance))
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["numRays"] = n
    W = [rays[k].astype(F) for k in ("ox", "oy", "oz", "dx", "dy", "dz")]
    R = [w.copy() for w in W]
    tmin = rays["tmin"].astype(F)
    # the seeded state: the record is the seed's words (kept as words: w2 and w3 are not floats to this spec), tmax the seed's t on a hit
    res = sw.copy()
    s_hit = sw[:, 0].view(np.int32) != -1
    tmax = np.where(s_hit, sw[:, 1].view(F), rays["tmax"].astype(F)).astype(F)
    res_inst = np.where(s_hit, seed_instance, -1).astype(np.int32)
    node = np.full(n, int(root_link), np.int64)
    inst = np.full(n, -1, np.int64)
    n_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    w_ext = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL
    if any_hit:
        node[s_hit] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_seeded: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1
        if probe is not None and idx.size:
            probe["maxStack"] = max(probe.get("maxStack", 0), int(sp[idx].max()))

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

    def wide(idx, buf, byte):
        """np_bvh_wide's wide-node step for rays idx on the nodes at `byte` of buf."""
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
        # candidates first, by ascending mn (a candidate's mn is no NaN; -0 + 0 == +0: floats compare, not words), ties by k
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
            is_exit = act & (node == EXIT_MARKER)
            is_inner = act & (node >= 0) & (node < SENTINEL)
            top = inst < 0
            k_top_inner = np.flatnonzero(is_inner & top)
            k_enter = np.flatnonzero(act & (node < 0) & top)
            k_bot_inner = np.flatnonzero(is_inner & ~top)
            k_tri = np.flatnonzero(act & (node < 0) & ~top)
            k_exit = np.flatnonzero(is_exit)
            k_other = np.flatnonzero(act & (node > SENTINEL) & ~is_exit)      # a positive word that is no link: dropped
            assert k_top_inner.size + k_enter.size + k_bot_inner.size + k_tri.size + k_exit.size + k_other.size == int(act.sum())
            cnt["numTopInnerVisits"] += k_top_inner.size
            cnt["numInnerVisits"] += k_bot_inner.size
            if wide_form:
                if k_top_inner.size:
                    wide(k_top_inner, tl, np.minimum(node[k_top_inner], tl_bytes))
                if k_bot_inner.size:
                    nd = node[k_bot_inner]
                    o = n_off[k_bot_inner] + nd
                    readable = (nd < w_ext[k_bot_inner]) & (o < NO_NODE)
                    wide(k_bot_inner, bn, np.where(readable, np.minimum(o, bn_bytes), bn_bytes))
            else:
                if k_top_inner.size:
                    inner(k_top_inner, tl, 0)
                if k_bot_inner.size:
                    inner(k_bot_inner, bn, n_off[k_bot_inner])
            if k_other.size:
                pop(k_other)
            if k_enter.size:
                i = ~node[k_enter]
                in_range = (i >= 0) & (i < num_inst)
                pop(k_enter[~in_range])                       # no instance: popped, counted as nothing, its mask never read
                k_enter, i = k_enter[in_range], i[in_range]
                seen = visible(M, m, i, k_enter)
                cnt["numInstancesMasked"] += int((~seen).sum())
                pop(k_enter[~seen])                           # refused: no marker, no transform; tmax, hit and instance untouched
                k_enter, i = k_enter[seen], i[seen]
                cnt["numInstanceEntries"] += k_enter.size
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
                w_ext[k_enter] = rec[i, 14]
                node[k_enter] = 0
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                pop(k_exit)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = is_terminator(pw_u, row)
                cnt["numLeafVisits"] += int(term.sum())
                cnt["numTriTests"] += int((~term).sum())
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
                    # (a missed test that updateHit accepts at t = FLT_MAX -- tmax = +inf -- records u = v = 0, as np_tracer's t)
                    h = ti[acc]
                    tmax[h] = tt[acc]
                    res[h, 0] = tri_index[a[acc]].view(np.uint32)
                    res[h, 1] = tt[acc].astype(F).view(np.uint32)
                    res[h, 2] = np.where(ok[acc], u[acc], F(0)).astype(F).view(np.uint32)
                    res[h, 3] = np.where(ok[acc], v[acc], F(0)).astype(F).view(np.uint32)
                    res_inst[h] = inst[h]
                    node[ti] -= 3
                    if any_hit:
                        node[h] = SENTINEL
    res_id = res[:, 0].copy().view(np.int32)
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res[:, 1].copy().view(F), res[:, 2].copy().view(F), res[:, 3].copy().view(F), res_inst, cnt
