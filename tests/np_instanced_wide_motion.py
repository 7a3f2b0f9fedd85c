"""numpy spec of motion blur over the 4-wide trees: ntr_tlas_wide_motion_refit, ntr_trace_instanced_wide_motion and
ntr_trace_instanced_wide_motion_stats.

EXTENSION: the reference has no instancing, no wide trees and no motion.  This docstring is the normative text; the device
(csrc/tlas_wide_motion_refit_kernels.hip, csrc/trace_instanced_wide_body.h under NTR_TIW_MOTION) equals wide_motion_refit() byte for
byte and trace() bit for bit in all four result words, the instance id and every counter.  The definitions come from the specs this one
joins and are not restated:
  np_instanced_motion   keys, time (clamp_time), pose (lerp, invert_many), the moving flag (moving), the 128-byte key entry
                        (motion_keys), the entering step's order of checks, and singular poses
  np_instanced_wide     the wide pool, the wide TLAS, the wide record and the wide loop
  np_wide_refit         the wide leaf box (wide_instance_box), the tolerant walk and the climb (rules 4, 5, 6, 1 and 7)

wide_motion_refit(wide_tlas_nodes, root_link, wide_records, wide_pool_nodes, blas_ranges, wide_ranges, inst0, inst1).
  np_wide_refit.refit_wide_tlas over inst0 with the three changes np_instanced_motion.motion_refit makes to np_tlas_refit.refit:
  record i      np_instanced_wide.widen_tlas's record of key-0 instance i (words 12..14 zero for a blas index outside [0, numBlas)),
                with word 15 = 1 where instance i is moving, else 0.  Written for every instance, as refit_wide_tlas writes it.
  motion keys   np_instanced_motion.motion_keys(inst0, inst1): byte for byte what motion_refit writes for the same two arrays, for
                EVERY instance.  The all-wide update path therefore needs no binary motion refit.
  leaf box      of a leaf ~i: np_wide_refit.wide_instance_box under key 0's objectToWorld, united -- min / max in the integer order
                (np_hlbvh.f2i) -- for a moving instance with wide_instance_box under key 1's.  Both come from the union of the root
                slots of i's wide BLAS; the pool's node 0 is not read.  Inner slots, link 0, padding, topology and the scene box are
                refit_wide_tlas's.  N == 1: record 0, key entry 0 and the scene box.
  stats         refit_wide_tlas's numNodes and numLeaves, and numMoving: the moving instances among all N.  err_bits are
                refit_wide_tlas's.
  A later plain np_wide_refit.refit_wide_tlas or np_instanced_wide.widen_tlas writes word 15 = 0 everywhere and thereby freezes the
  scene at key 0.

trace(wide_tlas, root_link, wide_records, motion_keys, pool, wide_pool, rays, any_hit, times, time, inst_masks, ray_masks, ray_mask).
  np_instanced_wide.trace (the masked loop) with np_instanced_motion.trace's step "top level, link ~i" in place of its own: the checks
  1..5 of np_instanced_motion in that order -- index in range; masks; room for the marker; if word 15 of wide record i is non-zero, the
  two keys are read at byte 128 * i of the motion key buffer (an entry outside the buffer reads as zeros), M(t_r) is formed and
  inverted, and a zero or non-finite determinant makes the step a POP counted as numSingular only; then the marker is pushed and the
  ray transformed by worldToObject(t_r) -- the record's words 0..11 for a static instance.  Words 12..14 of the wide record (offset, row
  offset, extent) are used as they are: the BLAS is key 0's.  Everything else is np_instanced_wide.trace's.

Counters: np_instanced_wide's eight, numMovingEntries and numSingular.

Algorithmic bytes (algorithmic_bytes): np_instanced_wide's formula, plus 128 (numMovingEntries + numSingular) -- the two keys -- plus
4 numRays when per-ray times are given.

KNOWN LIMIT, np_instanced_wide's: inside the shutter the records may differ from np_instanced_motion.trace's (the binary trees) where
two triangles are hit at the same t -- the visiting order decides.  The closest-hit t itself is the same: both trees' boxes contain
the swept instance.
"""
import numpy as np

import np_bvh_wide as bw
import np_hlbvh
import np_instanced_motion as mo
import np_instanced_wide as niw
import np_wide_refit as wr
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, _dot4, _smax, _smin, xform
from np_instanced_masked import is_terminator, visible
from np_instanced_wide import NO_NODE, WIDE_BYTES

COUNTERS = mo.COUNTERS
KEY_WORDS, KEY_BYTES = mo.KEY_WORDS, mo.KEY_BYTES


def algorithmic_bytes(c, instance_masks=False, ray_masks=False, ray_times=False):
    return (niw.algorithmic_bytes(c, instance_masks, ray_masks) + KEY_BYTES * (c["numMovingEntries"] + c["numSingular"])
            + (4 * c["numRays"] if ray_times else 0))


# ---- the refit -------------------------------------------------------------------------------------------------------------------------
def wide_sweep_box(wide_pool_nodes, wide_range, m0, m1, is_moving):
    """-> six float32 as lo.x hi.x lo.y hi.y lo.z hi.z: wide_instance_box under key 0, united with the one under key 1 for a moving
    instance."""
    b = wr.wide_instance_box(wide_pool_nodes, wide_range, m0)
    if is_moving:
        b1 = wr.wide_instance_box(wide_pool_nodes, wide_range, m1)
        i = np_hlbvh.f2i(np.stack([b, b1]))
        out = np.empty(6, np.int32)
        out[wr.LO], out[wr.HI] = i[:, wr.LO].min(axis=0), i[:, wr.HI].max(axis=0)
        b = np_hlbvh.i2f(out).astype(F)
    return b


def wide_motion_refit(wide_tlas_nodes, root_link, wide_records, wide_pool_nodes, blas_ranges, wide_ranges, inst0, inst1):
    """-> dict(nodes int32 (M, 32), records uint32 (N, 16), motion_keys uint32 (N, 32), scene_box float32[6] min.xyz max.xyz,
    stats dict(numNodes, numLeaves, numMoving), err_bits).  np_wide_refit.refit_wide_tlas restated with the swept leaf box, word 15
    and the key buffer."""
    n = inst0.shape[0]
    assert inst1.shape[0] == n
    num_blas = len(wide_ranges)
    wi = np.ascontiguousarray(wide_tlas_nodes).reshape(-1).view(np.int32).reshape(-1, bw.WIDE_WORDS).copy()
    wf = wi.view(F)
    rec = np.ascontiguousarray(wide_records).reshape(-1).view(np.uint32).reshape(-1, 16)[:n].copy()
    assert n >= 1 and rec.shape[0] == n and int(root_link) == (0 if n >= 2 else ~0)
    mv = mo.moving(inst0, inst1)
    keys = mo.motion_keys(inst0, inst1)
    num_moving = int(mv.sum())
    good = (inst0["blas"] >= 0) & (inst0["blas"] < num_blas)
    err = 0 if good.all() else wr.TL_ERR_BLAS
    rec[:] = niw.widen_tlas(None, ~0, inst0, blas_ranges, wide_ranges)["records"]
    rec[:, 15] = mv.astype(np.uint32)
    box_of = lambda i: wide_sweep_box(wide_pool_nodes, wide_ranges[int(inst0[i]["blas"])], inst0[i]["objectToWorld"],  # noqa: E731
                                      inst1[i]["objectToWorld"], mv[i])
    if n == 1:
        scene = wr._min_max(box_of(0)) if good[0] else np.zeros(6, F)
        return dict(nodes=wi, records=rec, motion_keys=keys, scene_box=scene, stats=dict(numNodes=0, numLeaves=1, numMoving=num_moving),
                    err_bits=err)
    levels, followed, e = wr._walk(wi, wr.TL_ERR_LINK)
    err |= e
    reached = [m for lv in levels for m in lv]
    well = np.zeros((wi.shape[0], 4), bool)
    leaves = 0
    for m in reached:
        for k in range(wr._count(wi, m)):
            link = int(wi[m, bw.WLINK + k])
            if link >= 0:
                continue
            leaves += 1
            i = ~link
            if i >= n:
                err |= wr.TL_ERR_LEAF
            elif good[i]:
                wf[m, wr.WBOX[k]] = box_of(i)
                well[m, k] = True
    node_well = wr._climb(wi, levels, followed, well)
    scene = wr._min_max(wr._fold(wf[0][wr.WBOX[:wr._count(wi, 0)]])) if wi.shape[0] and node_well[0] else np.zeros(6, F)
    return dict(nodes=wi, records=rec, motion_keys=keys, scene_box=scene,
                stats=dict(numNodes=len(reached), numLeaves=leaves, numMoving=num_moving), err_bits=err)


# ---- the trace: np_instanced_wide.trace restated with np_instanced_motion's time-sampled entering step -------------------------------
def trace(wide_tlas, root_link, wide_records, motion_keys, pool, wide_pool, rays, any_hit=False, times=None, time=0.0, inst_masks=None,
          ray_masks=None, ray_mask=0xFFFFFFFF):
    """wide_pool: widen_pool's dict, or the wide pool's bytes.  -> (id int32, t float32, u float32, v float32, instance int32, counters
    dict)"""
    def padded(buf):                                   # a zero node behind the extent: what a read beyond it gives
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        return np.concatenate([b, np.zeros(2 * WIDE_BYTES, np.uint8)]).view(F), b.size
    tl, tl_bytes = padded(wide_tlas)
    wp, wp_bytes = padded(wide_pool["nodes"] if isinstance(wide_pool, dict) else wide_pool)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(wide_records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    keys = np.ascontiguousarray(motion_keys).view(np.uint8).reshape(-1)
    keys = keys[:keys.size // KEY_BYTES * KEY_BYTES].view(F).reshape(-1, KEY_WORDS)
    tm = mo.clamp_time(np.full(n, time, F) if times is None else np.ascontiguousarray(times).view(F).reshape(-1))
    M = np.full(num_inst, 0xFFFFFFFF, np.uint32) if inst_masks is None else np.ascontiguousarray(inst_masks).view(np.uint32).reshape(-1)
    m = np.full(n, int(ray_mask) & 0xFFFFFFFF, np.uint32) if ray_masks is None else np.ascontiguousarray(ray_masks).view(np.uint32).reshape(-1)
    assert M.shape[0] == num_inst and m.shape[0] == n and tm.shape[0] == n
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["numRays"] = n
    W = [rays[k].astype(F) for k in ("ox", "oy", "oz", "dx", "dy", "dz")]
    R = [w.copy() for w in W]
    tmin = rays["tmin"].astype(F)
    tmax = rays["tmax"].astype(F).copy()
    res_id = np.full(n, -1, np.int32)
    res_inst = np.full(n, -1, np.int32)
    res_t = tmax.copy()
    res_u = np.zeros(n, F)
    res_v = np.zeros(n, F)
    node = np.full(n, int(root_link), np.int64)
    inst = np.full(n, -1, np.int64)
    w_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    w_ext = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_wide_motion: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

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
            if k_top_inner.size:
                wide(k_top_inner, tl, np.minimum(node[k_top_inner], tl_bytes))
            if k_bot_inner.size:
                nd = node[k_bot_inner]
                o = w_off[k_bot_inner] + nd
                readable = (nd < w_ext[k_bot_inner]) & (o < NO_NODE)
                wide(k_bot_inner, wp, np.where(readable, np.minimum(o, wp_bytes), wp_bytes))
            if k_other.size:
                pop(k_other)
            m_i = np.zeros((0, 12), F)
            if k_enter.size:
                i = ~node[k_enter]
                in_range = (i >= 0) & (i < num_inst)
                pop(k_enter[~in_range])                       # 1. no instance: popped, counted as nothing, its mask never read
                k_enter, i = k_enter[in_range], i[in_range]
                seen = visible(M, m, i, k_enter)
                cnt["numInstancesMasked"] += int((~seen).sum())
                pop(k_enter[~seen])                           # 2. refused: no key is read
                k_enter, i = k_enter[seen], i[seen]
                if (sp[k_enter] >= MAX_STACK).any():          # 3. room for the marker
                    raise RuntimeError("np_instanced_wide_motion: stack overflow")
                m_i = rec_f[i, :12].copy()
                mv = rec[i, 15] != 0                          # 4. a moving instance is posed at the ray's time
                if mv.any():
                    im = i[mv]
                    there = im < keys.shape[0]
                    k0, k1 = np.zeros((im.size, 12), F), np.zeros((im.size, 12), F)
                    k0[there], k1[there] = keys[im[there], 0:12], keys[im[there], 16:28]
                    w2o, ok = mo.invert_many(mo.lerp(k0, k1, tm[k_enter[mv]]))
                    m_i[mv] = w2o
                    cnt["numSingular"] += int((~ok).sum())
                    cnt["numMovingEntries"] += int(ok.sum())
                    good = np.ones(k_enter.size, bool)
                    good[np.flatnonzero(mv)[~ok]] = False
                    pop(k_enter[~good])                       # singular: a pop, nothing else touched
                    k_enter, i, m_i = k_enter[good], i[good], m_i[good]
                cnt["numInstanceEntries"] += k_enter.size
            if k_enter.size:
                push(k_enter, EXIT_MARKER)                    # 5.
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
                    res_t[h] = tt[acc]
                    res_u[h] = np.where(ok[acc], u[acc], F(0))
                    res_v[h] = np.where(ok[acc], v[acc], F(0))
                    res_id[h] = tri_index[a[acc]]
                    res_inst[h] = inst[h]
                    node[ti] -= 3                              # (the row after a triangle is read by the next step: a terminator pops)
                    if any_hit:
                        node[h] = SENTINEL
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res_t, res_u, res_v, res_inst, cnt
