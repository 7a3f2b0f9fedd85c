"""numpy spec of deforming BLASes in the motion-blurred two-level trace: ntr_tlas_deform_refit, ntr_trace_instanced_deform,
ntr_trace_instanced_deform_stats.

EXTENSION: the reference has no instancing and no motion.  This docstring is the normative text; the device
(csrc/tlas_deform_refit_kernels.hip, csrc/trace_instanced_body.h under NTR_TI_DEFORM) equals deform_refit() byte for byte and trace()
bit for bit in all four result words, the instance id and every counter.  np_instanced_motion.py states the time, lerp, invert_many, the
keys and moving(); np_bvh_motion.py states deform_lerp, motion_refit over one tree and the vertex rows; np_instanced_masked.py the masks.
They are imported; only the steps that change are restated.

Pool, key 1.  Beside nodes, woop and tri_index the pool has three more buffers: nodes1 with the pool's node bytes, vrows0 and vrows1 with
  the pool's row bytes each.  deforming[numBlas] (uint32, non-zero: deforming) says which BLASes have motion.  For a deforming BLAS b the
  slices at its range hold exactly what np_bvh_motion.motion_refit over that BLAS's slices writes: nodes0 (in `nodes`), woop, nodes1,
  vrows0, vrows1 (pool_motion_refit()).  For a BLAS that is not deforming nothing of nodes1, vrows0 or vrows1 is ever read; the caller
  need not initialise those bytes.

deform_refit(tlas_nodes, root_link, records, pool_nodes, pool_nodes1, blas_ranges, deforming, inst0, inst1).
np_instanced_motion.motion_refit with these changes:
  leaf box     Instance i has BLAS b.  K = {key-0 transform, key-1 transform} if the instance is moving, else {key 0}.  J = {nodes,
               nodes1} if b is deforming, else {nodes}.  The box is the union, in the integer order, of
               np_instanced.instance_box(pool nodes j, range b, M_k) over ALL pairs (k, j) of K x J: up to four boxes.
               Why four: a posed point is M(t) c(t) with both factors linear in t, a quadratic Bezier curve with the control points
               M0 c0, (M0 c1 + M1 c0) / 2 and M1 c1.  It lies in the hull of the four products M_k c_j, not in the hull of its two ends
               M0 c0 and M1 c1.  The object box at time t lies, up to rounding, in the hull of the two keys' object boxes, whose
               corners go through M(t) in the same way, so the union of the four instance boxes bounds the sweep.  No padding, as
               everywhere in the instanced path.  (test_instanced_deform_cpu.py counts posed boxes outside both unions: none for the
               four, some for the two-box union on `grid`.)
  word 15      bit 0 is moving, as in motion_refit; bit 1 says that the instance's BLAS is deforming.  Values 0..3.
  stats        motion_refit's, plus numDeforming: the instances whose BLAS is deforming.
  With no deforming BLAS every byte of nodes, records and keys is motion_refit's.  The motion key buffer is unchanged and is written for
  every instance.  A later plain np_tlas_refit.refit, or a motion_refit, rewrites word 15 without bit 1; records with bit 1 set are meant
  for this trace only.

trace(tlas_nodes, root_link, records, motion_keys, pool, rays, any_hit, times, time, masks).  np_instanced_motion.trace with these
changes:
  entering step        unchanged: bit 0 of word 15 alone decides the pose.  A lane that enters remembers bit 1 until its exit marker.
  inner step, in a deforming instance      the twelve box words are deform_lerp(nodes word, nodes1 word, t_r) at nodesOffset + node; the
                       links come from nodes.  Then the unchanged slab test and order (np_bvh_motion's inner step at a pool offset).
  triangle step, in a deforming instance   row rowOffset + ~node of vrows0 is a terminator iff its W word is 0x80000000.  Otherwise the
                       nine vertex words of that row and the two behind it, from vrows0 and vrows1, are posed by deform_lerp,
                       np_hlbvh.woop_rows forms the Woop rows and the unchanged triangle test runs on them (np_bvh_motion's triangle
                       step at a pool offset).  The hit row, the record and the instance id are as in the masked trace.
  In an instance whose BLAS is not deforming every step is np_instanced_motion.trace's.

Counters: np_instanced_motion's ten, plus numDeformEntries, numDeformInnerVisits and numDeformTriTests; each of the three is counted in
numInstanceEntries, numInnerVisits and numTriTests too.

Algorithmic bytes (algorithmic_bytes): np_instanced_motion's formula, plus 64 per deforming inner visit (the second key's node: 128 in
all, as np_bvh_motion) and 48 per deforming triangle test (six vertex rows: 96 in all).

Consequences, the yardsticks of the tests:
  a.  with no deforming BLAS the refit equals motion_refit byte for byte and the trace np_instanced_motion.trace in all five words and
      ten counters
  b.  one identity instance of a deforming BLAS, nothing moving, finite rays: id, t, u, v and the bottom-level counters equal
      np_bvh_motion.trace over that BLAS
  c.  at t = 0 and t = 1 the records and the masked counters equal np_instanced_masked.trace over the same top-level node buffer with
      that key's records and the pool refitted to that key (key 1's pool: nodes1's boxes with nodes' links, the Woop rows of
      np_bvh_refit.refit(pos1))
  d.  at a scalar interior time the closest hit's id, t and instance equal np_instanced.trace over the posed scene (lerped transforms,
      np_bvh_motion.posed_static_tree per deforming BLAS, a freshly built top-level tree), and the hit mask the binary64 brute force
"""
import numpy as np

import np_bvh_motion as bm
import np_hlbvh
import np_instanced as ni
import np_instanced_masked as nm
import np_instanced_motion as mo
import np_tlas_refit as tr
from np_bvh_refit import BOX_WORDS, HI, LO, _union, levels_of
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, _dot4, _smax, _smin, xform

COUNTERS = mo.COUNTERS + ("numDeformEntries", "numDeformInnerVisits", "numDeformTriTests")
TERM = bm.TERM
MOVING, DEFORMING = 1, 2          # the bits of record word 15


def algorithmic_bytes(c, instance_masks=False, ray_masks=False, ray_times=False):
    return mo.algorithmic_bytes(c, instance_masks, ray_masks, ray_times) + 64 * c["numDeformInnerVisits"] + 48 * c["numDeformTriTests"]


# ---- the pool's key 1 ------------------------------------------------------------------------------------------------------------------
def pool_motion_refit(pool, meshes, epsilon=0.0, fill=0xCD):
    """meshes: per BLAS None (static) or (tri, pos0, pos1).  -> the pool with np_bvh_motion.motion_refit run over every deforming BLAS's
    slices: dict(nodes, woop, tri_index, ranges, nodes1, vrows0, vrows1 uint8; deforming uint32 [numBlas]).  The bytes of nodes1, vrows0
    and vrows1 that belong to no deforming BLAS are `fill`: no step may read them."""
    nodes = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).copy()
    woop = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).copy()
    tri_index = np.ascontiguousarray(pool["tri_index"], np.int32).reshape(-1)
    nodes1 = np.full(nodes.size, fill, np.uint8)
    vrows0, vrows1 = np.full(woop.size, fill, np.uint8), np.full(woop.size, fill, np.uint8)
    assert len(meshes) == len(pool["ranges"])
    for (n_off, n_bytes, w_off, w_bytes), mesh in zip(pool["ranges"], meshes):
        if mesh is None:
            continue
        tri, pos0, pos1 = mesh
        m = bm.motion_refit(nodes[n_off:n_off + n_bytes], woop[w_off:w_off + w_bytes], tri_index[w_off // 16:(w_off + w_bytes) // 16], tri, pos0,
                            pos1, epsilon)
        nodes[n_off:n_off + n_bytes] = m["nodes0"].view(np.uint8).reshape(-1)
        nodes1[n_off:n_off + n_bytes] = m["nodes1"].view(np.uint8).reshape(-1)
        woop[w_off:w_off + w_bytes] = m["woop"]
        vrows0[w_off:w_off + w_bytes] = m["vrows0"].view(np.uint8).reshape(-1)
        vrows1[w_off:w_off + w_bytes] = m["vrows1"].view(np.uint8).reshape(-1)
    return dict(nodes=nodes, woop=woop, tri_index=tri_index, ranges=list(pool["ranges"]), nodes1=nodes1, vrows0=vrows0, vrows1=vrows1,
                deforming=np.array([0 if m is None else 1 for m in meshes], np.uint32))


# ---- the refit -------------------------------------------------------------------------------------------------------------------------
def sweep_box(pool_nodes, pool_nodes1, blas_range, m0, m1, is_moving, is_deforming, pairs=None):
    """-> six float32 in a node's box order: the union of instance_box over K x J.  pairs: the (k, j) to unite instead (the tests' two-box
    rule, which does NOT bound the sweep)."""
    K = (m0, m1) if is_moving else (m0,)
    J = (pool_nodes, pool_nodes1) if is_deforming else (pool_nodes,)
    lo = hi = None
    for k, m in enumerate(K):
        for j, nodes in enumerate(J):
            if pairs is not None and (k, j) not in pairs:
                continue
            l, h = ni.instance_box(nodes, blas_range, m)
            lo = l if lo is None else np_hlbvh.i2f(np.minimum(np_hlbvh.f2i(lo), np_hlbvh.f2i(l)))
            hi = h if hi is None else np_hlbvh.i2f(np.maximum(np_hlbvh.f2i(hi), np_hlbvh.f2i(h)))
    return tr._box6(lo, hi)


def deform_refit(tlas_nodes, root_link, records, pool_nodes, pool_nodes1, blas_ranges, deforming, inst0, inst1):
    """-> dict(nodes int32 (N - 1, 16), records uint32 (N, 16), motion_keys uint32 (N, 32), scene_box float32[6] min.xyz max.xyz,
    stats dict(numNodes, numLeaves, numMoving, numDeforming), err_bits).  np_instanced_motion.motion_refit restated with the four-box leaf
    and bit 1 of word 15."""
    n = inst0.shape[0]
    assert inst1.shape[0] == n
    num_blas = len(blas_ranges)
    deforming = np.asarray(deforming, np.uint32).reshape(-1)
    assert deforming.shape[0] == num_blas
    nodes = np.ascontiguousarray(tlas_nodes).reshape(-1).view(np.int32).reshape(-1, 16).copy()
    nf = nodes.view(F)
    rec = np.ascontiguousarray(records).reshape(-1).view(np.uint32).reshape(-1, 16)[:n].copy()
    assert n >= 1 and nodes.shape[0] == n - 1 and rec.shape[0] == n and int(root_link) == (0 if n >= 2 else ~0)
    mv = mo.moving(inst0, inst1)
    keys = mo.motion_keys(inst0, inst1)
    err = 0
    good_inst = (inst0["blas"] >= 0) & (inst0["blas"] < num_blas)
    if not good_inst.all():
        err |= tr.ERR_BLAS
    df = np.zeros(n, bool)
    df[good_inst] = deforming[inst0["blas"][good_inst]] != 0
    for i in np.flatnonzero(good_inst):
        rec[i] = tr.record_of(inst0[i], blas_ranges)
        rec[i, 15] = (MOVING if mv[i] else 0) | (DEFORMING if df[i] else 0)
    box_of = lambda i: sweep_box(pool_nodes, pool_nodes1, blas_ranges[int(inst0[i]["blas"])], inst0[i]["objectToWorld"],
                                 inst1[i]["objectToWorld"], mv[i], df[i])
    counts = dict(numMoving=int(mv.sum()), numDeforming=int(df.sum()))
    if n == 1:
        scene = box_of(0) if good_inst[0] else np.zeros(6, F)
        return dict(nodes=nodes, records=rec, motion_keys=keys, scene_box=np.concatenate([scene[LO], scene[HI]]).astype(F),
                    stats=dict(numNodes=0, numLeaves=1, **counts), err_bits=err)
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
    stats = dict(numNodes=int(reached.size), numLeaves=int(leaf.sum()), **counts)
    return dict(nodes=nodes, records=rec, motion_keys=keys, scene_box=scene, stats=stats, err_bits=err)


# ---- the trace: np_instanced_motion.trace restated with the two bottom-level steps of a deforming instance ----------------------------
def trace(tlas_nodes, root_link, records, motion_keys, pool, rays, any_hit=False, times=None, time=0.0, inst_masks=None, ray_masks=None,
          ray_mask=0xFFFFFFFF):
    """pool: pool_motion_refit's dict.  -> (id int32, t float32, u float32, v float32, instance int32, counters dict)"""
    tl = np.ascontiguousarray(tlas_nodes).view(np.uint8).reshape(-1)
    tl = np.concatenate([tl, np.zeros(64, np.uint8)]).view(F)        # (an empty buffer when N == 1)
    pn = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).view(F)
    pn1 = np.ascontiguousarray(pool["nodes1"]).view(np.uint8).reshape(-1).view(F)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    v0 = np.ascontiguousarray(pool["vrows0"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    v1 = np.ascontiguousarray(pool["vrows1"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    v0_u = v0.view(np.uint32)
    assert pn1.shape == pn.shape and v0.shape == pw.shape and v1.shape == pw.shape
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    keys = np.ascontiguousarray(motion_keys).view(np.uint8).reshape(-1)
    keys = keys[:keys.size // mo.KEY_BYTES * mo.KEY_BYTES].view(F).reshape(-1, mo.KEY_WORDS)
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
    deform = np.zeros(n, bool)                                       # bit 1 of the entered record, until the exit marker
    n_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    tri_of = np.arange(3, dtype=np.int32)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_deform: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

    def inner(idx, buf, base, buf1=None):
        """buf1: the second key's node buffer -- the box words are posed at the lanes' times; the links are buf's"""
        b = (base + node[idx]) // 4
        g = (lambda k: buf[b + k]) if buf1 is None else (lambda k: bm.deform_lerp(buf[b + k], buf1[b + k], tm[idx]))
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

    def triangles(ti, a, z, u4, v4):
        """The unchanged triangle test of rays ti at pool rows a on the Woop rows z, u4, v4"""
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
            k_bot_inner = np.flatnonzero(is_inner & ~top & ~deform)
            k_def_inner = np.flatnonzero(is_inner & ~top & deform)
            k_tri = np.flatnonzero(act & (node < 0) & ~top & ~deform)
            k_def_tri = np.flatnonzero(act & (node < 0) & ~top & deform)
            k_exit = np.flatnonzero(is_exit)
            assert (k_top_inner.size + k_enter.size + k_bot_inner.size + k_def_inner.size + k_tri.size + k_def_tri.size + k_exit.size
                    == int(act.sum()))
            cnt["numTopInnerVisits"] += k_top_inner.size
            cnt["numInnerVisits"] += k_bot_inner.size + k_def_inner.size
            cnt["numDeformInnerVisits"] += k_def_inner.size
            if k_top_inner.size:
                inner(k_top_inner, tl, 0)
            if k_bot_inner.size:
                inner(k_bot_inner, pn, n_off[k_bot_inner])
            if k_def_inner.size:
                inner(k_def_inner, pn, n_off[k_def_inner], pn1)
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
                    raise RuntimeError("np_instanced_deform: stack overflow")
                m_i = rec_f[i, :12].copy()
                mv = (rec[i, 15] & MOVING) != 0               # 4. bit 0 alone decides the pose
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
                    pop(k_enter[~good])                       # singular: a pop, before any deform read
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
                deform[k_enter] = (rec[i, 15] & DEFORMING) != 0   # remembered until the exit marker
                cnt["numDeformEntries"] += int(deform[k_enter].sum())
                n_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                node[k_enter] = 0
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                deform[k_exit] = False
                pop(k_exit)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = nm.is_terminator(pw_u, row)
                cnt["numLeafVisits"] += int(term.sum())
                cnt["numTriTests"] += int((~term).sum())
                pop(k_tri[term])
                ti, a = k_tri[~term], row[~term]
                if ti.size:
                    triangles(ti, a, pw[a], pw[a + 1], pw[a + 2])
            if k_def_tri.size:
                row = r_off[k_def_tri] + ~node[k_def_tri]
                term = v0_u[row, 3] == TERM                   # the W word: a vertex x of -0.0f is the same word as the terminator
                cnt["numLeafVisits"] += int(term.sum())
                cnt["numTriTests"] += int((~term).sum())
                cnt["numDeformTriTests"] += int((~term).sum())
                pop(k_def_tri[term])
                ti, a = k_def_tri[~term], row[~term]
                if ti.size:
                    p0 = np.stack([v0[a, :3], v0[a + 1, :3], v0[a + 2, :3]], 1)          # [m, 3 verts, 3 axes]
                    p1 = np.stack([v1[a, :3], v1[a + 1, :3], v1[a + 2, :3]], 1)
                    posed = np.ascontiguousarray(bm.deform_lerp(p0, p1, tm[ti][:, None, None]).reshape(-1, 3))
                    idx = np.ascontiguousarray((3 * np.arange(ti.size, dtype=np.int32))[:, None] + tri_of[None, :])
                    rows = np_hlbvh.woop_rows(idx, posed).reshape(-1, 3, 4)
                    triangles(ti, a, rows[:, 0], rows[:, 1], rows[:, 2])
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res_t, res_u, res_v, res_inst, cnt
