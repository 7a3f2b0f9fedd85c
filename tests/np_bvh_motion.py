"""numpy spec of deformation motion blur over one Compact tree: ntr_bvh_motion_refit, ntr_trace_bvh_motion, ntr_trace_bvh_motion_stats.

EXTENSION: the reference's scenes are static.  This docstring is the normative text; the device (csrc/bvh_motion_refit_kernels.hip,
csrc/trace_motion_kernels.hip) equals motion_refit() byte for byte and trace() bit for bit in all four result words and every counter.
np_bvh_refit.py states the refit, np_tracer.py the traversal, np_instanced_motion.py the time; they are imported or, where a step
changes in their middle, restated.

Keys.  One mesh topology (tri, numTris) and two vertex arrays: pos0 is the shutter's opening, pos1 its close.  The tree is one
  BVHLayout_Compact tree of any builder; its topology, leaves, triIndex and terminators are used as they are.

Time.  Ray r has time t_r = times[r] when per-ray times are given, else the launch's scalar time, clamped by
  np_instanced_motion.clamp_time: t > 0 ? (t < 1 ? t : 1) : 0, so a NaN gives 0.

Pose.  deform_lerp(a, b, t), per word, with u = fl(1 - t):
    a                            where t == 0
    b                            where t == 1
    fl(fl(u * a) + fl(t * b))    otherwise (binary32, both products rounded before the sum: no contraction)
  This is NOT np_instanced_motion.lerp: there is no "a and b are the same word" shortcut.  The same function poses box words and vertex
  words, and that is the point: rounding is monotonic and u, t >= 0, so lo0 <= v0 and lo1 <= v1 imply
  deform_lerp(lo0, lo1, t) <= deform_lerp(v0, v1, t) -- the posed box contains the posed triangle EXACTLY, at every level of the tree,
  with no padding.  (With the shortcut a box word that happens not to move would stay put while a vertex beside it wobbles past it.)
  The price: a vertex that does not move may wobble by an ulp inside the shutter, since fl(fl(u * a) + fl(t * a)) need not be a; of
  4 M random words 12 % changed.  That is harmless, because a triangle's Woop rows are recomputed from the posed vertices anyway.

motion_refit(nodes, woop, tri_index, tri, pos0, pos1, epsilon) -> dict:
  nodes0, woop   exactly np_bvh_refit.refit(nodes, woop, tri_index, tri, pos0, epsilon)
  nodes1         the nodes of np_bvh_refit.refit(nodes, woop, tri_index, tri, pos1, epsilon): all 64 bytes of every slot, so links,
                 split words and the slots no link reaches are copies of the input's
  vrows0, vrows1 two buffers shaped like woop (uint32 [rows, 4]).  For every row group r, r+1, r+2 that a reached leaf holds, the rows
                 are (x, y, z, 0) of vertices 0, 1, 2 of triangle tri_index[r] under that key.  A reached leaf's terminator row is
                 (0, 0, 0, 0x80000000).  Every other row is zero.  The terminator lives in the W word because a vertex x of -0.0f is
                 legal and is the same word as the terminator: the trace tests w, never x.
  scene_box      the union (integer order, np_hlbvh.f2i) of the two keys' scene boxes, min.xyz max.xyz
  stats          np_bvh_refit's (they are the same for both keys)

trace(nodes0, nodes1, vrows0, vrows1, tri_index, rays, any_hit, times, time) -> (id, t, u, v[, stats]).  np_tracer.trace's loop with two
  changed steps:
  inner step   the twelve box words are deform_lerp(nodes0 word, nodes1 word, t_r); the links come from nodes0
  leaf step    the row group at `row` is a terminator iff word 3 of vrows0[row] is 0x80000000.  Otherwise the nine vertex words of rows
               row, row+1, row+2 (words 0..2 each) are posed with deform_lerp, np_hlbvh.woop_rows (the restatement of
               woop_rows_verts) gives the three Woop rows, and np_tracer's triangle step runs on them
  Everything else is np_tracer.trace's: the visiting order, the stack of 100, degenerate rays (tmin >= tmax: a miss without traversal),
  the miss record (id -1, t = tmax, u = v = 0), the recorded miss at tmax = +inf, any hit.  u and v are recorded with an accepted hit, as
  the device's result record holds them.

Counters: np_tracer's four.  Algorithmic bytes (algorithmic_bytes): 128 per inner visit (two keys' 64), 96 per triangle test (six
vertex rows), 16 per terminator, 48 per ray (32 in, 16 out), and 4 more per ray when per-ray times are given.

Two consequences, the yardsticks of the tests:
  ends      at t = 0 the records equal np_tracer.trace's (and ntr_trace_bvh's) over the tree refitted to pos0, word for word, and at
            t = 1 those over the tree refitted to pos1: the posed words are the keys' own, and the Woop rows of a key's vertices are the
            refit's rows
  between   at a scalar time t the records equal np_tracer.trace over the POSED STATIC TREE (posed_static_tree): nodes0 with its box
            words lerped, rows made by np_bvh_refit.refit(..., deform_lerp(pos0, pos1, t), 0)
"""
import numpy as np

import np_bvh_refit as rf
import np_hlbvh
from np_instanced_motion import clamp_time
from np_tracer import FLT_MAX, _dot4, _smax, _smin

F = np.float32
TERM = rf.TERM
MAX_STACK = 100
COUNTERS = ("numInnerVisits", "numTriTests", "numLeafVisits", "numHits")
BOX_WORD_COUNT = 12


def algorithmic_bytes(c, num_rays, ray_times=False):
    return 128 * c["numInnerVisits"] + 96 * c["numTriTests"] + 16 * c["numLeafVisits"] + (52 if ray_times else 48) * num_rays


# ---- pose ------------------------------------------------------------------------------------------------------------------------------
def deform_lerp(a, b, t):
    """Per word; t a scalar or an array that broadcasts against a and b.  t is taken as given (clamp first)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    t = np.broadcast_to(np.asarray(t, F), np.broadcast(a, b, np.asarray(t)).shape)
    with np.errstate(all="ignore"):
        u = (F(1) - t).astype(F)
        v = ((u * a).astype(F) + (t * b).astype(F)).astype(F)
    return np.where(t == 0, a, np.where(t == 1, b, v)).astype(F)


# ---- the refit -------------------------------------------------------------------------------------------------------------------------
def vertex_rows(nodes, woop, tri_index, tri, pos):
    """The vertex rows of one key: uint32 [rows, 4]."""
    ni = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16)
    w = np.ascontiguousarray(woop).reshape(-1).view(np.uint32).reshape(-1, 4)
    tidx = np.ascontiguousarray(tri_index, np.int32).reshape(-1)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    levels = rf.levels_of(ni)
    leaf_node, leaf_k, of_leaf, rows = rf.leaf_rows(ni, w, levels)
    out = np.zeros_like(w)
    if rows.size:
        v = pos[tri[tidx[rows].astype(np.int64)]].view(np.uint32)     # [m, 3 verts, 3 axes]
        for j in range(3):
            out[rows + j, 0:3] = v[:, j]
    first = (~ni[leaf_node, 12 + leaf_k]).astype(np.int64)
    groups = np.bincount(of_leaf, minlength=leaf_node.size).astype(np.int64)
    out[first + 3 * groups] = np.array([0, 0, 0, TERM], np.uint32)
    return out


def motion_refit(nodes, woop, tri_index, tri, pos0, pos1, epsilon):
    """-> dict(nodes0, nodes1 int32 [slots, 16]; woop uint8 []; vrows0, vrows1 uint32 [rows, 4]; scene_box float32 [6]; stats)."""
    r0 = rf.refit(nodes, woop, tri_index, tri, pos0, epsilon)
    r1 = rf.refit(nodes, woop, tri_index, tri, pos1, epsilon)
    b0, b1 = np_hlbvh.f2i(r0["scene_box"]), np_hlbvh.f2i(r1["scene_box"])
    box = np.concatenate([np.minimum(b0[:3], b1[:3]), np.maximum(b0[3:], b1[3:])])
    return dict(nodes0=r0["nodes"], nodes1=r1["nodes"], woop=r0["woop"],
                vrows0=vertex_rows(nodes, woop, tri_index, tri, pos0), vrows1=vertex_rows(nodes, woop, tri_index, tri, pos1),
                scene_box=np_hlbvh.i2f(box).astype(F), stats=r0["stats"])


def posed_static_tree(m, tri_index, tri, pos0, pos1, t):
    """The static tree that the motion tree IS at the scalar time t (clamped here): (nodes int32 [slots, 16], woop uint8 [])."""
    t = clamp_time(t)
    nodes = m["nodes0"].copy()
    nodes.view(F)[:, :BOX_WORD_COUNT] = deform_lerp(m["nodes0"].view(F)[:, :BOX_WORD_COUNT], m["nodes1"].view(F)[:, :BOX_WORD_COUNT], t)
    pos = deform_lerp(np.asarray(pos0, F).reshape(-1, 3), np.asarray(pos1, F).reshape(-1, 3), t)
    return nodes, rf.refit(m["nodes0"], m["woop"], tri_index, tri, pos, 0.0)["woop"]


# ---- the trace -------------------------------------------------------------------------------------------------------------------------
def ray_times(n, times, time):
    """The clamped time of each of n rays."""
    if times is None:
        return clamp_time(np.full(n, time, F))
    times = np.asarray(times, F).reshape(-1)
    assert times.shape[0] >= n
    return clamp_time(times[:n])


def trace(nodes0, nodes1, vrows0, vrows1, tri_index, rays, any_hit=False, times=None, time=0.0, return_stats=False):
    """Returns (id int32, t, u, v float32) per ray; with return_stats also the four counters."""
    n_inner = n_tri = n_leaf = 0
    n0_f = np.ascontiguousarray(nodes0).reshape(-1).view(F)
    n1_f = np.ascontiguousarray(nodes1).reshape(-1).view(F)
    n0_i = n0_f.view(np.int32)
    v0_f = np.ascontiguousarray(vrows0).reshape(-1).view(F).reshape(-1, 4)
    v1_f = np.ascontiguousarray(vrows1).reshape(-1).view(F).reshape(-1, 4)
    v0_u = v0_f.view(np.uint32)
    tri_index = np.asarray(tri_index, dtype=np.int32)
    n = rays.shape[0]
    tr = ray_times(n, times, time)
    ox, oy, oz = rays["ox"].astype(F), rays["oy"].astype(F), rays["oz"].astype(F)
    dx, dy, dz = rays["dx"].astype(F), rays["dy"].astype(F), rays["dz"].astype(F)
    tmin = rays["tmin"].astype(F)
    tmax = rays["tmax"].astype(F).copy()

    res_id = np.full(n, -1, dtype=np.int32)
    res_t = tmax.copy()
    res_u = np.zeros(n, F)
    res_v = np.zeros(n, F)
    node = np.zeros(n, dtype=np.int64)
    stack = np.zeros((n, MAX_STACK), dtype=np.int64)
    sp = np.ones(n, dtype=np.int64)
    tri_cur = np.full(n, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        done = ~(tmin < tmax)                               # a degenerate ray is a miss without traversal
    one, zero = F(1.0), F(0.0)
    tri_of = np.arange(3, dtype=np.int32)

    def pop(mask):
        idx = np.nonzero(mask)[0]
        sp[idx] -= 1
        node[idx] = stack[idx, sp[idx]]
        done[idx[sp[idx] <= 0]] = True

    with np.errstate(all="ignore"):
        while not done.all():
            act = ~done
            # ---- leaf step: one triangle per iteration
            enter = act & (tri_cur < 0) & (node < 0)
            tri_cur[enter] = -node[enter] - 1
            inleaf = np.nonzero(act & (tri_cur >= 0))[0]
            if inleaf.size:
                ta = tri_cur[inleaf]
                term = v0_u[ta, 3] == TERM                  # the W word
                tl = inleaf[term]
                n_leaf += int(tl.size)
                tri_cur[tl] = -1
                m = np.zeros(n, dtype=bool)
                m[tl] = True
                pop(m)
                ti = inleaf[~term]
                if ti.size:
                    n_tri += int(ti.size)
                    a = tri_cur[ti]
                    tt_ = tr[ti]
                    k0 = np.stack([v0_f[a, :3], v0_f[a + 1, :3], v0_f[a + 2, :3]], 1)          # [m, 3 verts, 3 axes]
                    k1 = np.stack([v1_f[a, :3], v1_f[a + 1, :3], v1_f[a + 2, :3]], 1)
                    posed = np.ascontiguousarray(deform_lerp(k0, k1, tt_[:, None, None]).reshape(-1, 3))
                    idx = np.ascontiguousarray((3 * np.arange(ti.size, dtype=np.int32))[:, None] + tri_of[None, :])
                    rows = np_hlbvh.woop_rows(idx, posed).reshape(-1, 3, 4)
                    z, u4, v4 = rows[:, 0], rows[:, 1], rows[:, 2]
                    rx, ry, rz = ox[ti], oy[ti], oz[ti]
                    ex, ey, ez = dx[ti], dy[ti], dz[ti]
                    Oz = z[:, 3] - rx * z[:, 0] - ry * z[:, 1] - rz * z[:, 2]
                    ooDz = one / _dot4(np.stack([ex, ey, ez, np.zeros_like(ex)], 1), z[:, 0], z[:, 1], z[:, 2], z[:, 3])
                    t = Oz * ooDz
                    ok = (t > tmin[ti]) & (t < tmax[ti])
                    u = _dot4(u4, rx, ry, rz, np.full_like(rx, one)) + t * _dot4(u4, ex, ey, ez, np.full_like(rx, zero))
                    ok &= (u >= 0)
                    v = _dot4(v4, rx, ry, rz, np.full_like(rx, one)) + t * _dot4(v4, ex, ey, ez, np.full_like(rx, zero))
                    ok &= (v >= 0) & ((u + v) <= one)
                    tt = np.where(ok, t, FLT_MAX)
                    acc = (tt > tmin[ti]) & (tt < tmax[ti])
                    hi = ti[acc]
                    tmax[hi] = tt[acc]
                    res_t[hi] = tt[acc]
                    res_u[hi] = np.where(ok, u, zero)[acc]
                    res_v[hi] = np.where(ok, v, zero)[acc]
                    res_id[hi] = tri_index[a[acc]]
                    tri_cur[ti] += 3
                    if any_hit:
                        done[hi] = True
                        tri_cur[hi] = -1
            # ---- inner step
            inner = np.nonzero(~done & (tri_cur < 0) & (node >= 0) & ~enter)[0]
            if inner.size:
                n_inner += int(inner.size)
                b = node[inner] // 4
                tt_ = tr[inner]
                g = lambda k: deform_lerp(n0_f[b + k], n1_f[b + k], tt_)
                rx, ry, rz = ox[inner], oy[inner], oz[inner]
                ex, ey, ez = dx[inner], dy[inner], dz[inner]

                def box(lox, hix, loy, hiy, loz, hiz):
                    t0x, t0y, t0z = (lox - rx) / ex, (loy - ry) / ey, (loz - rz) / ez
                    t1x, t1y, t1z = (hix - rx) / ex, (hiy - ry) / ey, (hiz - rz) / ez
                    mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
                    mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
                    return mn, mx
                mn0, mx0 = box(g(0), g(1), g(2), g(3), g(8), g(9))
                mn1, mx1 = box(g(4), g(5), g(6), g(7), g(10), g(11))
                c0 = n0_i[b + 12].astype(np.int64)
                c1 = n0_i[b + 13].astype(np.int64)
                i0 = (mn0 <= mx0) & (mx0 >= tmin[inner]) & (mn0 <= tmax[inner])
                i1 = (mn1 <= mx1) & (mx1 >= tmin[inner]) & (mn1 <= tmax[inner])
                both = i0 & i1
                swp = both & (mn0 > mn1)
                near = np.where(swp, c1, c0)
                far = np.where(swp, c0, c1)
                bi = inner[both]
                if (sp[bi] >= MAX_STACK).any():
                    raise RuntimeError("np_bvh_motion: stack overflow")
                node[bi] = near[both]
                stack[bi, sp[bi]] = far[both]
                sp[bi] += 1
                o0 = i0 & ~i1
                node[inner[o0]] = c0[o0]
                o1 = i1 & ~i0
                node[inner[o1]] = c1[o1]
                m = np.zeros(n, dtype=bool)
                m[inner[~i0 & ~i1]] = True
                pop(m)
    if return_stats:
        return res_id, res_t, res_u, res_v, dict(numInnerVisits=n_inner, numTriTests=n_tri, numLeafVisits=n_leaf,
                                                 numHits=int((res_id >= 0).sum()))
    return res_id, res_t, res_u, res_v
