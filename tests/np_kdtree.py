"""Independent restatement of the kd-tree path (test helper): the spatial-median builder with CudaKDTree's buffer emission in
plain Python, and the trace_kdtree kernel as a lock-step, vectorised numpy binary32 tracer in the style of np_tracer.py.

Follows src/rt/kdtree/NaiveKDTreeBuilder.cpp:43-158, KDTree.cpp:59-69, src/rt/cuda/CudaKDTree.cpp:94-160,
CudaKDTreeTracer.cpp:97 and fermi_kdtree_while_while_leafRef.cu:244-624 (SHORTSTACK 0), with the deviations stated in
include/ntrace_amd.h: a root leaf is stored under one inner node, a miss records (-1, ray.tmax, 0, 0), and popping the stack's
bottom ends traversal.
"""
import numpy as np

F = np.float32
EMPTY = np.int32(-2147483648)        # 0x80000000: empty leaf child / list terminator


def _f32bits(x):
    return int(np.array([x], dtype=F).view(np.int32)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# spatial-median builder + DFS emission
# ---------------------------------------------------------------------------------------------------------------------------
def spatial_median(tri, pos, max_leaf=1, max_depth=18):
    """Returns dict(nodes int32[n,4], tri_index int32[], scene_min, scene_max float32[3], delta float32, stats)."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    n = tri.shape[0]
    v = pos[tri]                                         # [n, 3 vertices, 3]
    bmin = v.min(axis=1).tolist()                        # float32 values held exactly as Python floats
    bmax = v.max(axis=1).tolist()
    root_lo = [float(F(min(b[k] for b in bmin))) for k in range(3)]
    root_hi = [float(F(max(b[k] for b in bmax))) for k in range(3)]

    refs = list(range(n))                                # the reference stack (triangle ids)
    out_idx = []                                         # KDTree::getTriIndices
    dups = [0]

    def build(num, lo, hi, level):
        if num <= max_leaf or level >= max_depth:
            start = len(out_idx)
            for _ in range(num):
                out_idx.append(refs.pop())
            return ("leaf", start, len(out_idx))
        dim = level % 3
        p = float((F(lo[dim]) + F(hi[dim])) / F(2))
        left_start = len(refs) - num
        left_end = left_start
        right_start = len(refs)
        i = left_end
        while i < right_start:
            t = refs[i]
            if bmax[t][dim] <= p:
                refs[i], refs[left_end] = refs[left_end], refs[i]
                left_end += 1
            elif bmin[t][dim] >= p:
                right_start -= 1
                refs[i], refs[right_start] = refs[right_start], refs[i]
                i -= 1
            i += 1
        for i in range(left_end, right_start):
            refs.append(refs[i])
            left_end += 1
            dups[0] += 1
        nl = left_end - left_start
        nr = len(refs) - right_start
        lhi = list(hi)
        lhi[dim] = p
        rlo = list(lo)
        rlo[dim] = p
        right = build(nr, rlo, hi, level + 1)
        left = build(nl, lo, lhi, level + 1)
        return ("inner", p, dim, left, right)

    root = build(n, root_lo, root_hi, 0)
    return _emit(root, out_idx, tri, pos, n, dups[0])


def _emit(root, out_idx, tri, pos, num_tris, dups):
    ref_tris = []
    tri_index = []

    def leaf(node):
        _, lo, hi = node
        start = len(tri_index)
        for k in range(lo, hi):
            tri_index.append(out_idx[k])
            ref_tris.append(out_idx[k])
        if hi == lo:
            return int(EMPTY)
        tri_index.append(int(EMPTY))
        return ~start

    nodes = []
    if root[0] == "leaf":
        c0 = leaf(root)
        vmax = pos[tri[np.array(ref_tris, dtype=np.int64)]].reshape(-1, 3).max(axis=0) if ref_tris else np.full(3, -3.402823466e38, F)
        nodes.append([c0, int(EMPTY), _f32bits(vmax[0]), 0])
    else:
        stack = [(root, 0)]
        nxt = 1
        table = {}
        while stack:
            node, idx = stack.pop()
            ch = []
            for c in (node[3], node[4]):
                if c[0] == "leaf":
                    ch.append(leaf(c))
                else:
                    ch.append(nxt)
                    stack.append((c, nxt))
                    nxt += 1
            table[idx] = [ch[0], ch[1], _f32bits(node[1]), (node[2] << 28)]
        nodes = [table[i] for i in range(nxt)]
    nodes = np.array(nodes, dtype=np.int64).astype(np.int32).reshape(-1, 4)
    tri_index = np.array(tri_index, dtype=np.int64).astype(np.int32)
    if ref_tris:
        vv = pos[tri[np.array(ref_tris, dtype=np.int64)]].reshape(-1, 3)
        smin, smax = vv.min(axis=0).astype(F), vv.max(axis=0).astype(F)
    else:
        smin, smax = np.full(3, 3.402823466e38, F), np.full(3, -3.402823466e38, F)
    stats = kdtree_stats(nodes, tri_index)
    stats["percentDuplicates"] = float(F(dups) / F(num_tris) * F(100))
    return dict(nodes=nodes, tri_index=tri_index, scene_min=smin, scene_max=smax, delta=delta_of(smin, smax), stats=stats)


def delta_of(smin, smax):
    """CudaKDTreeTracer.cpp:97: length(max + min) * 1e-6 in binary32, the squares summed left to right."""
    s = np.asarray(smax, dtype=F) + np.asarray(smin, dtype=F)
    return F(np.sqrt(F(F(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])) * F(1e-6))


def kdtree_stats(nodes, tri_index):
    """Counts over the buffers: inner nodes, leaves, empty leaves, references, depth (inner nodes on the longest path)."""
    nodes = np.asarray(nodes, dtype=np.int32).reshape(-1, 4)
    tri_index = np.asarray(tri_index, dtype=np.int32)
    st = dict(numInnerNodes=0, numLeafNodes=0, numEmptyLeaves=0, numTriRefs=0, maxDepth=0)
    stack = [(0, 1)]
    while stack:
        i, d = stack.pop()
        st["numInnerNodes"] += 1
        st["maxDepth"] = max(st["maxDepth"], d)
        for c in nodes[i, :2].tolist():
            if c >= 0:
                stack.append((c, d + 1))
                continue
            st["numLeafNodes"] += 1
            if c == int(EMPTY):
                st["numEmptyLeaves"] += 1
                continue
            k = ~c
            while tri_index[k] != EMPTY:
                st["numTriRefs"] += 1
                k += 1
            if k == ~c:
                st["numEmptyLeaves"] += 1
    return st


def leaf_cells(nodes, tri_index, scene_min, scene_max):
    """[(cell_min, cell_max, [triangle ids])] for every leaf, the cells found by walking down from the scene box."""
    nodes = np.asarray(nodes, dtype=np.int32).reshape(-1, 4)
    out = []
    stack = [(0, np.asarray(scene_min, dtype=np.float64).copy(), np.asarray(scene_max, dtype=np.float64).copy())]
    while stack:
        i, lo, hi = stack.pop()
        split = float(np.array([nodes[i, 2]], dtype=np.int32).view(F)[0])
        axis = (int(nodes[i, 3]) >> 28) & 0xF
        for side, c in enumerate(nodes[i, :2].tolist()):
            clo, chi = lo.copy(), hi.copy()
            if side == 0:
                chi[axis] = min(chi[axis], split)
            else:
                clo[axis] = max(clo[axis], split)
            if c >= 0:
                stack.append((c, clo, chi))
                continue
            ids = []
            if c != int(EMPTY):
                k = ~c
                while tri_index[k] != EMPTY:
                    ids.append(int(tri_index[k]))
                    k += 1
            out.append((clo, chi, ids))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# traversal: trace_kdtree, lock-step over the batch
# ---------------------------------------------------------------------------------------------------------------------------
def trace(nodes, woop, tri_index, scene_min, scene_max, rays, max_stack=64):
    """Returns a RESULT-like structured array (id, t, padA, padB) equal bit for bit to ntr_trace_kdtree's records."""
    nodes = np.asarray(nodes, dtype=np.int32).reshape(-1, 4)
    woop_f = np.frombuffer(np.ascontiguousarray(woop).tobytes(), dtype=F).reshape(-1, 4)
    tri_index = np.asarray(tri_index, dtype=np.int32)
    bmin = np.asarray(scene_min, dtype=F)
    bmax = np.asarray(scene_max, dtype=F)
    delta = delta_of(bmin, bmax)
    n = rays.shape[0]
    ox, oy, oz = (rays[k].astype(F) for k in ("ox", "oy", "oz"))
    dx, dy, dz = (rays[k].astype(F) for k in ("dx", "dy", "dz"))
    org = np.stack([ox, oy, oz], axis=1)
    eps = F(2.0 ** -80)
    with np.errstate(all="ignore"):
        idir = np.stack([F(1) / np.where(np.abs(d) > eps, d, np.copysign(eps, d)).astype(F) for d in (dx, dy, dz)], axis=1).astype(F)
        ood = (org * idir).astype(F)
        clo = (bmin[None, :] * idir - ood).astype(F)
        chi = (bmax[None, :] * idir - ood).astype(F)
        lo3, hi3 = np.fmin(clo, chi), np.fmax(clo, chi)
        tmin = (np.fmax(np.fmax(np.fmax(lo3[:, 0], lo3[:, 1]), lo3[:, 2]), rays["tmin"].astype(F)) - F(1e-4)).astype(F)
        tmax = (np.fmin(np.fmin(np.fmin(hi3[:, 0], hi3[:, 1]), hi3[:, 2]), rays["tmax"].astype(F)) + F(1e-4)).astype(F)

    node = np.zeros(n, dtype=np.int64)
    stack_n = np.zeros((n, max_stack), dtype=np.int64)
    stack_t = np.zeros((n, max_stack), dtype=F)
    sp = np.zeros(n, dtype=np.int64)
    hit = np.full(n, -1, dtype=np.int64)
    hu = np.zeros(n, dtype=F)
    hv = np.zeros(n, dtype=F)
    cur = np.full(n, -1, dtype=np.int64)                 # >= 0: position in triIndex inside a leaf
    check = np.ones(n, dtype=bool)                       # at an inner node: the loop's tmax >= tmin test comes first
    done = np.zeros(n, dtype=bool)

    def after_leaf(idx):
        h = hit[idx] != -1
        done[idx[h]] = True
        idx = idx[~h]
        tmin[idx] = tmax[idx]
        bottom = sp[idx] == 0
        done[idx[bottom]] = True
        idx = idx[~bottom]
        sp[idx] -= 1
        node[idx] = stack_n[idx, sp[idx]]
        tmax[idx] = stack_t[idx, sp[idx]]

    with np.errstate(all="ignore"):
        while True:
            act = np.nonzero(~done)[0]
            if act.size == 0:
                break
            # ---- inner nodes -------------------------------------------------------------------------------------------
            inn = act[node[act] >= 0]
            if inn.size:
                ok = tmax[inn] >= tmin[inn]
                done[inn[~ok]] = True
                i = inn[ok]
                cell = nodes[node[i]]
                axis = (cell[:, 3].astype(np.int64) >> 28) & 0xF
                split = cell[:, 2].view(F)
                o = org[i, axis]
                idd = idir[i, axis]
                t = ((split - o) * idd).astype(F)
                neg = (idd.view(np.uint32) >> 31) != 0
                first = np.where(neg, cell[:, 1], cell[:, 0]).astype(np.int64)
                second = np.where(neg, cell[:, 0], cell[:, 1]).astype(np.int64)
                near = t > tmax[i]
                far = ~near & (t < tmin[i])
                both = ~near & ~far
                node[i[near]] = first[near]
                node[i[far]] = second[far]
                b = i[both]
                assert (sp[b] < max_stack).all(), "stack overflow"
                stack_n[b, sp[b]] = second[both]
                stack_t[b, sp[b]] = tmax[b]
                sp[b] += 1
                node[b] = first[both]
                tmax[b] = t[both]
            # ---- leaves: one reference (or the leaf's end) per iteration -------------------------------------------------
            lf = act[(node[act] < 0) & ~done[act]]
            lf = lf[np.isin(lf, inn, invert=True)] if inn.size else lf
            if lf.size:
                enter = lf[cur[lf] < 0]
                empty = enter[(node[enter] & 0xF0000000) == 0x80000000]
                after_leaf(empty)
                start = enter[(node[enter] & 0xF0000000) != 0x80000000]
                cur[start] = ~node[start]
                i = lf[cur[lf] >= 0]
                tid = tri_index[cur[i]].astype(np.int64)
                term = tid == int(EMPTY)
                ended = i[term]
                cur[ended] = -1
                after_leaf(ended)
                i, tid = i[~term], tid[~term]
                cur[i] += 1
                w0, w1, w2 = woop_f[tid * 3], woop_f[tid * 3 + 1], woop_f[tid * 3 + 2]
                Ox_, Oy_, Oz_ = ox[i], oy[i], oz[i]
                Dx_, Dy_, Dz_ = dx[i], dy[i], dz[i]
                Oz = (((w0[:, 3] - Ox_ * w0[:, 0]) - Oy_ * w0[:, 1]) - Oz_ * w0[:, 2]).astype(F)
                inv = (F(1) / ((Dx_ * w0[:, 0] + Dy_ * w0[:, 1]) + Dz_ * w0[:, 2])).astype(F)
                t = (Oz * inv).astype(F)
                acc = (t >= (tmin[i] - delta)) & (t <= (tmax[i] + delta))
                Ox = (((w1[:, 3] + Ox_ * w1[:, 0]) + Oy_ * w1[:, 1]) + Oz_ * w1[:, 2]).astype(F)
                Dx = ((Dx_ * w1[:, 0] + Dy_ * w1[:, 1]) + Dz_ * w1[:, 2]).astype(F)
                u = (Ox + t * Dx).astype(F)
                acc &= (u >= F(0)) & (u <= F(1))
                Oy = (((w2[:, 3] + Ox_ * w2[:, 0]) + Oy_ * w2[:, 1]) + Oz_ * w2[:, 2]).astype(F)
                Dy = ((Dx_ * w2[:, 0] + Dy_ * w2[:, 1]) + Dz_ * w2[:, 2]).astype(F)
                vv = (Oy + t * Dy).astype(F)
                acc &= (vv >= F(0)) & ((u + vv) <= F(1))
                h = i[acc]
                tmax[h] = t[acc]
                hu[h] = u[acc]
                hv[h] = vv[acc]
                hit[h] = tid[acc]

    res = np.zeros(n, dtype=[("id", "<i4"), ("t", "<f4"), ("padA", "<i4"), ("padB", "<i4")])
    is_hit = hit != -1
    res["id"] = np.where(is_hit, hit, -1)
    res["t"] = np.where(is_hit, tmax, rays["tmax"].astype(F))
    res["padA"] = np.where(is_hit, hu.view(np.int32), 0)
    res["padB"] = np.where(is_hit, hv.view(np.int32), 0)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# coverage: every triangle that reaches into a leaf's cell is referenced by that leaf
# ---------------------------------------------------------------------------------------------------------------------------
def _sat_overlap(v, lo, hi, tol):
    """Triangles v [m, 3, 3] against boxes [lo, hi] ([m, 3]) in float64: True where no separating axis leaves a gap or an overlap of
    at most tol (a triangle that only touches a cell, or lies in one of its faces, does not count)."""
    c = (lo + hi) * 0.5
    h = (hi - lo) * 0.5
    p = v - c[:, None, :]
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], axis=1)
    axes = [np.broadcast_to(np.eye(3)[k], p[:, 0].shape) for k in range(3)]
    axes.append(np.cross(e[:, 0], e[:, 1]))
    for i in range(3):
        for k in range(3):
            axes.append(np.cross(np.eye(3)[k][None, :], e[:, i]))
    ok = np.ones(v.shape[0], dtype=bool)
    for a in axes:
        n = np.linalg.norm(a, axis=1)
        valid = n > 1e-12
        an = np.where(valid[:, None], a / np.where(valid, n, 1.0)[:, None], 0.0)
        proj = np.einsum("mvk,mk->mv", p, an)
        r = np.abs(an) @ np.ones(3) * 0.0 + (np.abs(an) * h).sum(axis=1)
        depth = np.minimum(proj.max(axis=1) + r, r - proj.min(axis=1))
        ok &= ~valid | (depth > tol)
    return ok


def coverage_violations(nodes, tri_index, scene_min, scene_max, tri, pos, rel_tol=1e-5):
    """[(leaf cell lo, hi, triangle id)] for every triangle that overlaps a leaf's cell with positive area (SAT with a margin of
    rel_tol x the scene's extent: touching a cell, lying in one of its faces, or crossing a zero-width cell does not count) and
    is missing from the leaf's list."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    v = np.asarray(pos, dtype=np.float64).reshape(-1, 3)[tri]
    tlo, thi = v.min(axis=1), v.max(axis=1)
    tol = rel_tol * float(np.max(np.asarray(scene_max, np.float64) - np.asarray(scene_min, np.float64)))
    nodes = np.asarray(nodes, dtype=np.int32).reshape(-1, 4)
    tri_index = np.asarray(tri_index, dtype=np.int32)
    bad = []
    stack = [(0, np.asarray(scene_min, np.float64), np.asarray(scene_max, np.float64), np.arange(tri.shape[0]))]
    while stack:
        i, lo, hi, cand = stack.pop()
        split = float(np.array([nodes[i, 2]], dtype=np.int32).view(F)[0])
        axis = (int(nodes[i, 3]) >> 28) & 0xF
        for side, ch in enumerate(nodes[i, :2].tolist()):
            clo, chi = lo.copy(), hi.copy()
            if side == 0:
                chi[axis] = min(chi[axis], split)
            else:
                clo[axis] = max(clo[axis], split)
            sel = cand[np.all((tlo[cand] < chi - tol) & (thi[cand] > clo + tol), axis=1)]
            if ch >= 0:
                stack.append((ch, clo, chi, sel))
                continue
            ids = set()
            if ch != int(EMPTY):
                k = ~ch
                while tri_index[k] != EMPTY:
                    ids.add(int(tri_index[k]))
                    k += 1
            miss = np.array([t for t in sel.tolist() if t not in ids], dtype=np.int64)
            if miss.size and np.all(chi - clo > tol):   # a flat cell meets a crossing triangle in a segment: no area
                ov = _sat_overlap(v[miss], np.broadcast_to(clo, (miss.size, 3)), np.broadcast_to(chi, (miss.size, 3)), tol)
                bad.extend((clo, chi, int(t)) for t in miss[ov])
    return bad
