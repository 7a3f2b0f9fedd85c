"""numpy spec of instance visibility masks and counters in the two-level trace: ntr_trace_instanced_masked, ntr_trace_instanced_stats.

EXTENSION: the reference has no instancing.  This docstring is the normative text; the device (csrc/trace_instanced_body.h in its masked
and instrumented variants) equals trace() bit for bit in all four result words and the instance id, and in every counter.

Rule.  ntr_trace_instanced's rule, tests/np_instanced.py, with one change to the step "top level, link ~i":
  - Ray r carries a mask m_r.  m_r = d_rayMasks[r] when per-ray masks are given, else the launch's rayMask.
  - Instance i carries a mask M_i.  M_i = d_instanceMasks[i] when instance masks are given, else 0xFFFFFFFF.
  - If (M_i & m_r) != 0, the ray enters instance i exactly as in np_instanced.trace.
  - Otherwise the step is a pop: no exit marker is pushed; the ray is not transformed; tmax, the hit and the instance id are untouched.
  - All 32 bits are mask bits.  Bit 31 is not a sign.
  - A ray with m_r == 0 still walks the top level and ends as a miss (id -1, t = ray.tmax, u = v = 0, instance -1).  One rule, no
    special case.
Nothing else changes: degenerate rays, any hit, the 16 + 88 stack, the exit marker, a link ~i with i >= numInstances (popped, and its
mask is never read).

Counters are summed over the rays of a launch.  A "step" is one iteration of a ray in trace()'s loop.
  numRays             rays of the launch
  numTopInnerVisits   inner steps on the top level
  numInstanceEntries  entering steps that entered
  numInstancesMasked  entering steps the masks refused
  numInnerVisits      inner steps inside instances
  numTriTests         rows tested that are not a terminator
  numLeafVisits       terminator rows read
  numHits             rays whose record has id != -1
Two kinds of entering step count as neither an entry nor a masked step: a step whose index is outside [0, numInstances), and a step that
finds no room for the marker (this spec raises there, as np_instanced.trace does).  One ray is traced by one lane with no sharing, so
the device's counters are deterministic and equal these exactly, for closest hit and any hit.  (The device reads a triangle's 48 bytes
together with the word after them and so takes the terminator that follows a triangle in the same iteration; that word is a terminator
row read all the same, and it is not read when an any-hit ray ended on the triangle -- as here, where such a ray makes no further step.)

Algorithmic bytes of a launch (algorithmic_bytes):
  52 numRays + 64 (numTopInnerVisits + numInstanceEntries + numInnerVisits) + 32 numInstanceEntries + 48 numTriTests + 16 numLeafVisits
  + 4 numHits, plus 4 (numInstanceEntries + numInstancesMasked) when instance masks are given and 4 numRays when per-ray masks are given
(52 numRays: the ray, the record and the instance id; 64 (...): the 64-byte fetches; 32 numInstanceEntries: the world ray reloaded on
leaving).
"""
import numpy as np

from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, TERM, _dot4, _smax, _smin, xform

COUNTERS = ("numRays", "numTopInnerVisits", "numInstanceEntries", "numInstancesMasked", "numInnerVisits", "numTriTests", "numLeafVisits",
            "numHits")


def algorithmic_bytes(c, instance_masks=False, ray_masks=False):
    n = (52 * c["numRays"] + 64 * (c["numTopInnerVisits"] + c["numInstanceEntries"] + c["numInnerVisits"]) + 32 * c["numInstanceEntries"]
         + 48 * c["numTriTests"] + 16 * c["numLeafVisits"] + 4 * c["numHits"])
    return n + (4 * (c["numInstanceEntries"] + c["numInstancesMasked"]) if instance_masks else 0) + (4 * c["numRays"] if ray_masks else 0)


def visible(M, m, i, k):
    """The entering steps' test, one call per batch of entering steps in range: rays k at instances i."""
    return (M[i] & m[k]) != 0               # all 32 bits are mask bits


def is_terminator(rows_u32, row):
    """The bottom level's row test, one call per batch of rows read."""
    return rows_u32[row, 0] == TERM


# ---- the two-level trace with masks and counters: np_instanced.trace restated -----------------------------------------------------------
def trace(tlas_nodes, root_link, records, pool, rays, any_hit=False, inst_masks=None, ray_masks=None, ray_mask=0xFFFFFFFF):
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
    M = np.full(num_inst, 0xFFFFFFFF, np.uint32) if inst_masks is None else np.ascontiguousarray(inst_masks).view(np.uint32).reshape(-1)
    m = np.full(n, int(ray_mask) & 0xFFFFFFFF, np.uint32) if ray_masks is None else np.ascontiguousarray(ray_masks).view(np.uint32).reshape(-1)
    assert M.shape[0] == num_inst and m.shape[0] == n
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
            raise RuntimeError("np_instanced_masked: stack overflow")
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
                    node[ti] -= 3
                    if any_hit:
                        node[h] = SENTINEL
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res_t, res_u, res_v, res_inst, cnt
