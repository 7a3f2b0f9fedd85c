"""numpy spec of motion blur in instanced scenes: ntr_tlas_motion_refit, ntr_trace_instanced_motion, ntr_trace_instanced_motion_stats.

EXTENSION: the reference has no instancing and no motion.  This docstring is the normative text; the device
(csrc/tlas_motion_refit_kernels.hip, csrc/trace_instanced_body.h under NTR_TI_MOTION) equals motion_refit() byte for byte and trace()
bit for bit in all four result words, the instance id and every counter.  np_instanced.py states the pool, the instance, the record,
invert and instance_box; np_tlas_refit.py the refit's rules 1..7; np_instanced_masked.py the masked trace.  They are imported or, where
a step changes in their middle, restated.

Keys.  Two NtrInstance arrays of N entries: key 0 is the shutter open, key 1 the close.  The BLAS index and worldToObject are taken
  from key 0; of key 1 only objectToWorld is read.  Instance i is MOVING iff any of the twelve objectToWorld words differs bitwise
  between the keys (moving()).

Time.  Ray r has time t_r = rayTimes[r] when per-ray times are given, else the launch's scalar time.  It is clamped by
  t > 0 ? (t < 1 ? t : 1) : 0 -- a NaN gives 0 (clamp_time()).

Pose.  lerp(a, b, t), per component, with u = 1.0f - t:
    a                  where t == 0, or where a and b are the same word
    b                  where t == 1
    u * a + t * b      otherwise, in binary32, both products rounded before the sum (no contraction)
  So M(0) and M(1) are the keys bit for bit, signed zeros included, and a component that does not move never changes.
  worldToObject(t) = np_instanced.invert(M(t)): binary64, each of the 12 results rounded once (invert_many() is that function over
  many matrices, with a flag instead of an exception for a zero or non-finite determinant).

motion_refit(tlas_nodes, root_link, records, pool_nodes, blas_ranges, inst0, inst1).  np_tlas_refit.refit over inst0 with three changes:
  leaf box      of a moving instance: the union, min / max in the integer order (np_hlbvh.f2i), of np_instanced.instance_box under
                key 0's and under key 1's objectToWorld.  Every corner moves on a straight line between its two end positions, up to
                rounding, so the union bounds the sweep; no padding.  A static instance's box is np_tlas_refit's.  Inner boxes and the
                scene box climb as in np_tlas_refit.
  record i      np_tlas_refit's record of key-0 instance i, except that word 15 is 1 for a moving instance and 0 otherwise.  (An
                instance whose blas index names no BLAS keeps its record, as in np_tlas_refit rule 7.)
  motion keys   beside the records, 128 bytes (32 words) per instance: words 0..11 objectToWorld of key 0, words 16..27 objectToWorld
                of key 1, every other word zero.  Written for EVERY instance -- static ones and ones with a bad blas index too --
                so the whole buffer is deterministic.
  stats         np_tlas_refit's numNodes and numLeaves, and numMoving: the moving instances among all N.
  A later plain np_tlas_refit.refit writes word 15 = 0 everywhere and thereby freezes the scene at key 0.

trace(tlas_nodes, root_link, records, motion_keys, pool, rays, any_hit, times, time, masks).  np_instanced_masked.trace with one change
to the step "top level, link ~i".  The checks run in this order:
  1. index in range (else a pop, counted as nothing);
  2. masks, as in np_instanced_masked (a refusal is a pop, counted as numInstancesMasked; no key is read);
  3. room for the marker (this spec raises, as np_instanced_masked does);
  4. if word 15 of record i is non-zero, the two keys are read from the motion key buffer at byte 128 * i (an entry outside the buffer
     reads as zeros), M(t_r) = lerp(key 0, key 1, t_r) is formed and inverted.  A zero or non-finite determinant makes the step a POP:
     no marker, no transform, nothing else touched; it is counted as numSingular, and as neither an entry nor a masked step;
  5. the marker is pushed and the ray is transformed by worldToObject(t_r) -- the record's words 0..11 for a static instance -- with
     np_instanced.xform.  A moving instance that is entered counts as numInstanceEntries AND numMovingEntries.
  Words 12..14 of the record (the BLAS's ranges) are used as they are: the BLAS is key 0's.
  Everything else (exit marker, world ray reloaded on leaving, stack, degenerate rays, any hit) is np_instanced_masked.trace's.

Counters: np_instanced_masked's eight, numMovingEntries and numSingular.

Algorithmic bytes (algorithmic_bytes): np_instanced_masked's formula, plus 128 (numMovingEntries + numSingular) -- the two keys -- plus
4 numRays when per-ray times are given.
"""
import numpy as np

import np_hlbvh
import np_instanced as ni
import np_instanced_masked as nm
import np_tlas_refit as tr
from np_bvh_refit import BOX_WORDS, HI, LO, _union, levels_of
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, _dot4, _smax, _smin, xform

COUNTERS = nm.COUNTERS + ("numMovingEntries", "numSingular")
KEY_WORDS, KEY_BYTES = 32, 128


def algorithmic_bytes(c, instance_masks=False, ray_masks=False, ray_times=False):
    return (nm.algorithmic_bytes(c, instance_masks, ray_masks) + KEY_BYTES * (c["numMovingEntries"] + c["numSingular"])
            + (4 * c["numRays"] if ray_times else 0))


# ---- time and pose --------------------------------------------------------------------------------------------------------------------
def clamp_time(t):
    """t > 0 ? (t < 1 ? t : 1) : 0, elementwise; a NaN gives 0."""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        return np.where(t > 0, np.where(t < 1, t, F(1)), F(0)).astype(F)


def lerp(a, b, t):
    """M(t) of the keys a, b (..., 12) at the clamped times t (a scalar, or one per leading index)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    t = np.asarray(t, F)
    if t.ndim:
        t = t[..., None]
    t = np.broadcast_to(t, a.shape)
    with np.errstate(all="ignore"):
        u = (F(1) - t).astype(F)
        v = ((u * a).astype(F) + (t * b).astype(F)).astype(F)
    same = a.view(np.uint32) == b.view(np.uint32)
    return np.where((t == 0) | same, a, np.where(t == 1, b, v)).astype(F)


def invert_many(m):
    """np_instanced.invert over (k, 12) matrices -> (worldToObject (k, 12) float32, ok (k,)); a row that is not ok is zero."""
    m = np.asarray(m, F).reshape(-1, 12).astype(np.float64)
    m00, m01, m02, t0, m10, m11, m12, t1, m20, m21, m22, t2 = (m[:, k] for k in range(12))
    with np.errstate(all="ignore"):
        c00 = m11 * m22 - m12 * m21
        c01 = m12 * m20 - m10 * m22
        c02 = m10 * m21 - m11 * m20
        det = (m00 * c00 + m01 * c01) + m02 * c02
        ok = np.isfinite(det) & (det != 0.0)
        rows = [[c00 / det, (m02 * m21 - m01 * m22) / det, (m01 * m12 - m02 * m11) / det],
                [c01 / det, (m00 * m22 - m02 * m20) / det, (m02 * m10 - m00 * m12) / det],
                [c02 / det, (m01 * m20 - m00 * m21) / det, (m00 * m11 - m01 * m10) / det]]
        out = np.zeros((m.shape[0], 12), F)
        for r in range(3):
            for c in range(3):
                out[:, 4 * r + c] = rows[r][c].astype(F)
            out[:, 4 * r + 3] = (-((rows[r][0] * t0 + rows[r][1] * t1) + rows[r][2] * t2)).astype(F)
    out[~ok] = 0
    return out, ok


def moving(inst0, inst1):
    a = np.ascontiguousarray(inst0["objectToWorld"]).view(np.uint32).reshape(-1, 12)
    b = np.ascontiguousarray(inst1["objectToWorld"]).view(np.uint32).reshape(-1, 12)
    return (a != b).any(axis=1)


def motion_keys(inst0, inst1):
    """The motion key buffer: uint32 (N, 32)."""
    k = np.zeros((inst0.shape[0], KEY_WORDS), np.uint32)
    k[:, 0:12] = np.ascontiguousarray(inst0["objectToWorld"]).view(np.uint32).reshape(-1, 12)
    k[:, 16:28] = np.ascontiguousarray(inst1["objectToWorld"]).view(np.uint32).reshape(-1, 12)
    return k


# ---- the refit -------------------------------------------------------------------------------------------------------------------------
def sweep_box(pool_nodes, blas_range, m0, m1, is_moving):
    """-> six float32 in a node's box order: instance_box under key 0, united with the one under key 1 for a moving instance."""
    lo, hi = ni.instance_box(pool_nodes, blas_range, m0)
    if is_moving:
        lo1, hi1 = ni.instance_box(pool_nodes, blas_range, m1)
        lo = np_hlbvh.i2f(np.minimum(np_hlbvh.f2i(lo), np_hlbvh.f2i(lo1)))
        hi = np_hlbvh.i2f(np.maximum(np_hlbvh.f2i(hi), np_hlbvh.f2i(hi1)))
    return tr._box6(lo, hi)


def motion_refit(tlas_nodes, root_link, records, pool_nodes, blas_ranges, inst0, inst1):
    """-> dict(nodes int32 (N - 1, 16), records uint32 (N, 16), motion_keys uint32 (N, 32), scene_box float32[6] min.xyz max.xyz,
    stats dict(numNodes, numLeaves, numMoving), err_bits).  np_tlas_refit.refit restated with the swept leaf box and word 15."""
    n = inst0.shape[0]
    assert inst1.shape[0] == n
    num_blas = len(blas_ranges)
    nodes = np.ascontiguousarray(tlas_nodes).reshape(-1).view(np.int32).reshape(-1, 16).copy()
    nf = nodes.view(F)
    rec = np.ascontiguousarray(records).reshape(-1).view(np.uint32).reshape(-1, 16)[:n].copy()
    assert n >= 1 and nodes.shape[0] == n - 1 and rec.shape[0] == n and int(root_link) == (0 if n >= 2 else ~0)
    mv = moving(inst0, inst1)
    keys = motion_keys(inst0, inst1)
    err = 0
    good_inst = (inst0["blas"] >= 0) & (inst0["blas"] < num_blas)
    if not good_inst.all():
        err |= tr.ERR_BLAS
    for i in np.flatnonzero(good_inst):
        rec[i] = tr.record_of(inst0[i], blas_ranges)
        rec[i, 15] = 1 if mv[i] else 0
    box_of = lambda i: sweep_box(pool_nodes, blas_ranges[int(inst0[i]["blas"])], inst0[i]["objectToWorld"], inst1[i]["objectToWorld"], mv[i])
    num_moving = int(mv.sum())
    if n == 1:
        scene = box_of(0) if good_inst[0] else np.zeros(6, F)
        return dict(nodes=nodes, records=rec, motion_keys=keys, scene_box=np.concatenate([scene[LO], scene[HI]]).astype(F),
                    stats=dict(numNodes=0, numLeaves=1, numMoving=num_moving), err_bits=err)
    S = n - 1
    links = nodes[:, 12:14].astype(np.int64)
    bad_link = (links > 0) & ((links % 64 != 0) | (links // 64 >= S))
    if bad_link.any():
        err |= tr.ERR_LINK
    walk = nodes.copy()
    walk[:, 12:14][bad_link] = 0
    levels = levels_of(walk)
    reached = np.concatenate(levels)
    leaf = links[reached] < 0
    if ((~links[reached])[leaf] >= n).any():
        err |= tr.ERR_LEAF
    well = np.zeros((S, 2), bool)
    for slots in reversed(levels):
        for s in slots:
            for k in (0, 1):
                c = int(links[s, k])
                if c < 0:
                    i = ~c
                    if i < n and good_inst[i]:
                        nf[s, BOX_WORDS[k]] = box_of(i)
                        well[s, k] = True
                elif c > 0 and not bad_link[s, k]:
                    ch = c // 64
                    if well[ch].all():
                        nf[s, BOX_WORDS[k]] = _union(nf[ch:ch + 1, BOX_WORDS[0]], nf[ch:ch + 1, BOX_WORDS[1]])[0]
                        well[s, k] = True
    if well[0].all():
        root = _union(nf[0:1, BOX_WORDS[0]], nf[0:1, BOX_WORDS[1]])[0]
        scene = np.concatenate([root[LO], root[HI]]).astype(F)
    else:
        scene = np.zeros(6, F)
    stats = dict(numNodes=int(reached.size), numLeaves=int(leaf.sum()), numMoving=num_moving)
    return dict(nodes=nodes, records=rec, motion_keys=keys, scene_box=scene, stats=stats, err_bits=err)


# ---- the trace: np_instanced_masked.trace restated with the time-sampled entering step -----------------------------------------------
def trace(tlas_nodes, root_link, records, motion_keys, pool, rays, any_hit=False, times=None, time=0.0, inst_masks=None, ray_masks=None,
          ray_mask=0xFFFFFFFF):
    """-> (id int32, t float32, u float32, v float32, instance int32, counters dict)"""
    tl = np.ascontiguousarray(tlas_nodes).view(np.uint8).reshape(-1)
    tl = np.concatenate([tl, np.zeros(64, np.uint8)]).view(F)        # (an empty buffer when N == 1)
    pn = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).view(F)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    keys = np.ascontiguousarray(motion_keys).view(np.uint8).reshape(-1)
    keys = keys[:keys.size // KEY_BYTES * KEY_BYTES].view(F).reshape(-1, KEY_WORDS)
    tm = clamp_time(np.full(n, time, F) if times is None else np.ascontiguousarray(times).view(F).reshape(-1))
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
    n_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_motion: stack overflow")
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
            is_exit = act & (node == EXIT_MARKER)
            is_inner = act & (node >= 0) & (node < SENTINEL)
            top = inst < 0
            k_top_inner = np.flatnonzero(is_inner & top)
            k_enter = np.flatnonzero(act & (node < 0) & top)
            k_bot_inner = np.flatnonzero(is_inner & ~top)
            k_tri = np.flatnonzero(act & (node < 0) & ~top)
            k_exit = np.flatnonzero(is_exit)
            assert k_top_inner.size + k_enter.size + k_bot_inner.size + k_tri.size + k_exit.size == int(act.sum())
            cnt["numTopInnerVisits"] += k_top_inner.size
            cnt["numInnerVisits"] += k_bot_inner.size
            if k_top_inner.size:
                inner(k_top_inner, tl, 0)
            if k_bot_inner.size:
                inner(k_bot_inner, pn, n_off[k_bot_inner])
            m_i = np.zeros((0, 12), F)
            if k_enter.size:
                i = ~node[k_enter]
                in_range = (i >= 0) & (i < num_inst)
                pop(k_enter[~in_range])                       # 1. no instance: popped, counted as nothing
                k_enter, i = k_enter[in_range], i[in_range]
                seen = nm.visible(M, m, i, k_enter)
                cnt["numInstancesMasked"] += int((~seen).sum())
                pop(k_enter[~seen])                           # 2. refused: no key is read
                k_enter, i = k_enter[seen], i[seen]
                if (sp[k_enter] >= MAX_STACK).any():          # 3. room for the marker
                    raise RuntimeError("np_instanced_motion: stack overflow")
                m_i = rec_f[i, :12].copy()
                mv = rec[i, 15] != 0                          # 4. a moving instance is posed at the ray's time
                if mv.any():
                    im = i[mv]
                    there = im < keys.shape[0]
                    k0, k1 = np.zeros((im.size, 12), F), np.zeros((im.size, 12), F)
                    k0[there], k1[there] = keys[im[there], 0:12], keys[im[there], 16:28]
                    w2o, ok = invert_many(lerp(k0, k1, tm[k_enter[mv]]))
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
                n_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                node[k_enter] = 0
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                pop(k_exit)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = nm.is_terminator(pw_u, row)
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
                    h = ti[acc]
                    tmax[h] = tt[acc]
                    res_t[h] = tt[acc]
                    res_u[h] = np.where(ok[acc], u[acc], F(0))
                    res_v[h] = np.where(ok[acc], v[acc], F(0))
                    res_id[h] = tri_index[a[acc]]
                    res_inst[h] = inst[h]
                    node[ti] -= 3
                    if any_hit:
                        node[h] = SENTINEL
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res_t, res_u, res_v, res_inst, cnt
