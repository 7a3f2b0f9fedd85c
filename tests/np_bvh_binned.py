"""Independent restatement of the on-device binned SAH BVH build (ntr_persistent_bvh_build, csrc/bvh_build_kernels.hip): the
reference's persistent BVH builder as it is configured -- CudaTracerDefines.h SPLIT_TYPE 5, PLANE_COUNT 32, BINNING_TYPE 2,
AABB_TYPE 3, SAH_TERMINATION, COMPUTE_MEDIAN_BOUNDS, no clipping; config.conf block PersistentBVH (triLimit 16, triMaxLimit 16,
maxDepth 50, ci 1, ct 1); epsilon = FLT_EPSILON (Renderer.cpp:264) -- rebuilt breadth first, one level per round, in vectorised
numpy binary32.  The device build's three Compact buffers and its counts equal this module's byte for byte.

The rule (persistent_bvh.cu, rt_common.cu, CudaPersistentBVHBuilder.cpp):

  Candidates (findPlaneAABB, rt_common.cu:1007-1030).  Plane k = 0..31 of a task lies on axis k // 11 (11 on x, 11 on y, 10 on z)
    at pos = lo[a] + (hi[a] - lo[a]) * rpos, rpos = float32(1 + k % 11) / float32(12), each operation rounded on its own, over the
    task's box as written into its parent node.  The root's box is the scene box the caller passes (CudaPersistentBVHBuilder.cpp:21,
    485-495: Scene::getBBox).
  Sides (getPlaneCentroidPosition, rt_common.cu:440-468; binTrianglesAtomic, persistent_bvh.cu:2923-2990).  A triangle's box is the
    min / max of its vertices, its centroid c = fl(fl(mn + mx) * 0.5f).  With the plane (-1, 0, 0, pos) planeDistance is
    fl(pos - c[a]) (the other two products are +-0).  fl(pos - c[a]) < EPS (EPS = 1e-8f) is side -1, which the reference calls left
    and bins into children[0]: the triangles whose centroids lie at or above the plane (within EPS) go to child 0.
  Bins.  On one axis the positions are non-decreasing in k and fl(pos - c) is non-decreasing in pos, so the planes that put a
    triangle on side -1 form a prefix; its length b in 0..11 (0..10 on z) is the triangle's bin on that axis, and plane j of the
    axis has on side -1 exactly the triangles of bins > j.  Each (task, axis, bin) holds a count and the union of its triangles'
    boxes; the sweeps over 12 / 12 / 11 bins give every plane's counts and boxes exactly.
  Cost (taskFinishBinning, persistent_bvh.cu:1710-1800).  s_k = areaAABB(boxL) * float(nL) + areaAABB(boxR) * float(nR) over the
    sides' union boxes without epsilon, area = (dx*dy + dy*dz + dz*dx) * 2.  An empty side keeps the initial box (FLT_MAX, -FLT_MAX)
    (CudaPersistentBVHBuilder.cpp:470-471), whose area is inf, so its cost is inf * 0 = NaN.
  Choice.  CANONICAL: among the planes whose s_k is finite the lowest wins (+0 == -0), ties to the lowest k; a NaN or infinite s_k
    never wins (the reference's warp min ignores NaN; its first-lane ballot picks the lowest k).
  No split (persistent_bvh.cu:1815-1822, 2301-2303).  No winning plane, or a partition with an empty side, falls back to an object
    median: child 0 gets the first n // 2 of the task's references, child 1 the rest (triStart + n / 2).  The partition is stable,
    so a task's references are in ascending triangle id.
  Boxes.  A child's box is fl(min - eps) / fl(max + eps) of the union of its triangles' boxes.  The SAH path adds -eps / +eps to the
    bin union (persistent_bvh.cu:1855-1863); the median path (COMPUTE_MEDIAN_BOUNDS, AABB_TYPE 3) reduces per-triangle fl(min - eps)
    / fl(max + eps) (:4259-4261, :4347-4349).  Rounding x - eps and x + eps is monotone non-decreasing in x and an exact zero
    result is +0 whatever the sign of x, so both equal the union's fl(min - eps) / fl(max + eps).  Min and max use the total order
    -0 < +0 (the float-order integer atomics).  An empty child (only the one-triangle root below) has the box (FLT_MAX, -FLT_MAX).
  Termination (taskTerminationCriteria, persistent_bvh.cu:245-271; taskDecideType :357).  With the partition's nL, nR and the
    children's boxes (epsilon included) against the task's box: if nL + nR <= triMaxLimit and
    ci * float(n) < ct + ci * (fl(areaL / area * nL) + fl(areaR / area * nR)), the task is a leaf of all its references.
    Otherwise it is an inner node, and a child with <= triLimit references, or whose parent's depth is > maxDepth - 2, is a leaf.
    The root's depth is 0.
  DEVIATION: the root is never a leaf.  The reference's root leaf (parentIdx -1) has no Compact form: a Compact root is an inner
    node.  A root that termination ends -- numTris <= triLimit, or the SAH test -- is split anyway by its partition (the chosen
    plane, else the median) and both children are leaves.  One triangle: the median gives child 0 empty (a leaf of no triangles,
    box (FLT_MAX, -FLT_MAX), the LBVH's form, lbvh_kernels.hip:1146) and child 1 the triangle.
  Order.  CANONICAL: every child -- one already known to be a leaf included -- is a task of the next level, child 0 before child 1.
    Inner nodes are numbered in level order, the root 0.  Leaves take their Woop blocks in the same order: 3 rows per triangle
    (woop_rows.h) then one terminator row of 0x80000000, the triIndex entry of a triangle's first row its id, 0 elsewhere.
  Layout.  BVHLayout_Compact as ntr_lbvh_build writes it: 16 words per node, c0 x/y box, c1 x/y box, z boxes, child 0, child 1,
    the split axis (0 for a median split; the reference writes its parent index, which no tracer reads) and 0.  An inner child is
    64 * index, a leaf child ~row.

Statistics: numInnerNodes, numLeaves (the empty leaf included), numLevels (rounds), maxDepth (inner nodes on the longest
root-to-leaf path), medianFallbacks (tasks split, or ended, at the median), costLeaves (tasks the SAH test ended) and depthLeaves
(children with more than triLimit references made leaves by the depth cap).
"""
import numpy as np

import np_hlbvh

F = np.float32
EPS = F(1e-8)
FLT_MAX = F(np.finfo(np.float32).max)
FLT_EPSILON = F(np.finfo(np.float32).eps)
PLANES = 32
PER_AXIS = (PLANES + 2) // 3                                                # 11
AXIS_PLANES = (PER_AXIS, PER_AXIS, PLANES - 2 * PER_AXIS)                   # 11, 11, 10
RPOS = (np.arange(PER_AXIS) + 1).astype(F) / F(PER_AXIS + 1)

DEFAULTS = dict(triLimit=16, triMaxLimit=16, maxDepth=50, ci=1.0, ct=1.0, epsilon=float(FLT_EPSILON))

_BIG = int(np_hlbvh.f2i(FLT_MAX))
_SMALL = int(np_hlbvh.f2i(-FLT_MAX))


def area(lo, hi):
    """areaAABB of boxes lo, hi ([..., 3])."""
    with np.errstate(all="ignore"):
        d = (hi - lo).astype(F)
        return (((d[..., 0] * d[..., 1]) + (d[..., 1] * d[..., 2])) + (d[..., 2] * d[..., 0])) * F(2)


def tri_terms(tri, pos):
    """Per-triangle box lo, hi and centroid ([n, 3] float32); min / max in the order -0 < +0."""
    v = np.asarray(pos, dtype=F)[np.asarray(tri, dtype=np.int64)]          # [n, 3 verts, 3]
    i = np_hlbvh.f2i(v)
    lo = np_hlbvh.i2f(i.min(axis=1)).astype(F)
    hi = np_hlbvh.i2f(i.max(axis=1)).astype(F)
    with np.errstate(all="ignore"):
        c = ((lo + hi) * F(0.5)).astype(F)
    return lo, hi, c


def plane_positions(lo, hi, axis):
    """[T, planes of the axis] positions over task boxes lo, hi ([T, 3])."""
    m = AXIS_PLANES[axis]
    with np.errstate(all="ignore"):
        return (lo[:, axis:axis + 1] + (hi[:, axis:axis + 1] - lo[:, axis:axis + 1]) * RPOS[None, :m]).astype(F)


def side_neg(pos, c):
    """getPlaneCentroidPosition == -1 (child 0): fl(pos - c) < EPS."""
    with np.errstate(all="ignore"):
        return (pos - c).astype(F) < EPS


def _seg_reduce(key, vals, nseg, fn, init):
    out = np.full((nseg,) + vals.shape[1:], init, dtype=np.int64)
    fn.at(out, key, vals)
    return out


def _i2f(a):
    return np_hlbvh.i2f(np.asarray(a).astype(np.int32)).astype(F)


def _grow(lo_i, hi_i, eps):
    """fl(union lo - eps), fl(union hi + eps) from ordered-int unions; an empty union is (FLT_MAX, -FLT_MAX)."""
    lo, hi = _i2f(lo_i), _i2f(hi_i)
    with np.errstate(all="ignore"):
        glo = (lo - eps).astype(F)
        ghi = (hi + eps).astype(F)
    empty = lo_i > hi_i
    return np.where(empty, FLT_MAX, glo).astype(F), np.where(empty, -FLT_MAX, ghi).astype(F)


def build(tri, pos, scene_min=None, scene_max=None, params=None, trace_levels=None):
    """The device build.  Returns dict(nodes int32[m, 16], woop uint8[], tri_index int32[], stats dict).  trace_levels: a list that
    receives each level's decisions."""
    p = dict(DEFAULTS)
    p.update(params or {})
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = tri.shape[0]
    assert n >= 1
    if scene_min is None or scene_max is None:
        i = np_hlbvh.f2i(pos)
        scene_min, scene_max = _i2f(i.min(axis=0)), _i2f(i.max(axis=0))
    tri_limit, tri_max, max_depth = int(p["triLimit"]), int(p["triMaxLimit"]), int(p["maxDepth"])
    ci, ct, eps = F(p["ci"]), F(p["ct"]), F(p["epsilon"])
    tlo, thi, cen = tri_terms(tri, pos)
    tlo_i, thi_i = np_hlbvh.f2i(tlo).astype(np.int64), np_hlbvh.f2i(thi).astype(np.int64)
    woop12 = np_hlbvh.woop_rows(tri, pos)

    # level state: task boxes, reference ranges, parent slots (word index into the node array), forced leaves
    lo = np.asarray(scene_min, F).reshape(1, 3).copy()
    hi = np.asarray(scene_max, F).reshape(1, 3).copy()
    start = np.array([0], np.int64)
    count = np.array([n], np.int64)
    slot = np.array([-1], np.int64)
    forced = np.array([False])
    refs = np.arange(n, dtype=np.int64)

    nodes = []                 # per inner node: int32[16]
    leaf_blocks = []           # (row offset, tri ids) per leaf, in order
    rows = 0
    st = dict(numInnerNodes=0, numLeaves=0, numLevels=0, maxDepth=0, medianFallbacks=0, costLeaves=0, depthLeaves=0)
    level = 0
    while count.size:
        T = count.size
        st["numLevels"] += 1
        task_of = np.repeat(np.arange(T), count)
        pos_in = np.arange(refs.size) - np.repeat(start, count)
        cand = ~forced
        split_axis = np.zeros(T, np.int64)
        split_pos = np.zeros(T, F)
        nl = np.zeros(T, np.int64)
        box0 = np.zeros((T, 2, 3), np.int64)          # ordered-int unions (lo, hi) of child 0 / child 1
        box1 = np.zeros((T, 2, 3), np.int64)
        best_s = np.full(T, np.inf, F)
        best_k = np.full(T, -1, np.int64)
        # ---- binning: per axis the prefix length of the side -1 planes, then the sweeps -----------------------------------
        kbase = 0
        for a in range(3):
            m = AXIS_PLANES[a]
            pl = plane_positions(lo, hi, a)                                    # [T, m]
            neg = side_neg(pl[task_of], cen[refs, a][:, None])                 # [R, m]
            b = neg.sum(axis=1)
            assert np.array_equal(neg, np.arange(m)[None, :] < b[:, None]), "side -1 planes are not a prefix"
            key = task_of * (m + 1) + b
            nb = T * (m + 1)
            cnt = np.bincount(key, minlength=nb).reshape(T, m + 1)
            blo = _seg_reduce(key, tlo_i[refs], nb, np.minimum, _BIG).reshape(T, m + 1, 3)
            bhi = _seg_reduce(key, thi_i[refs], nb, np.maximum, _SMALL).reshape(T, m + 1, 3)
            pre_c, suf_c = np.cumsum(cnt, axis=1), np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]
            pre_lo, pre_hi = np.minimum.accumulate(blo, axis=1), np.maximum.accumulate(bhi, axis=1)
            suf_lo = np.minimum.accumulate(blo[:, ::-1], axis=1)[:, ::-1]
            suf_hi = np.maximum.accumulate(bhi[:, ::-1], axis=1)[:, ::-1]
            for j in range(m):             # plane j: side -1 = bins j+1..m, side +1 = bins 0..j
                cl, cr = suf_c[:, j + 1], pre_c[:, j]
                al = area(_i2f(suf_lo[:, j + 1]), _i2f(suf_hi[:, j + 1]))
                ar = area(_i2f(pre_lo[:, j]), _i2f(pre_hi[:, j]))
                with np.errstate(all="ignore"):
                    s = (al * cl.astype(F) + ar * cr.astype(F)).astype(F)
                win = cand & np.isfinite(s) & (s < best_s)
                best_s = np.where(win, s, best_s)
                best_k = np.where(win, kbase + j, best_k)
                split_axis = np.where(win, a, split_axis)
                split_pos = np.where(win, pl[:, j], split_pos)
                nl = np.where(win, cl, nl)
                box0 = np.where(win[:, None, None], np.stack([suf_lo[:, j + 1], suf_hi[:, j + 1]], 1), box0)
                box1 = np.where(win[:, None, None], np.stack([pre_lo[:, j], pre_hi[:, j]], 1), box1)
            kbase += m
        # ---- median fallback -----------------------------------------------------------------------------------------------
        median = cand & ((best_k < 0) | (nl == 0) | (nl == count))
        if median.any():
            first = pos_in < (count // 2)[task_of]
            sel = median[task_of]
            for mask, box in ((first, box0), (~first, box1)):
                k, r = task_of[sel & mask], refs[sel & mask]
                box[median, 0] = _seg_reduce(k, tlo_i[r], T, np.minimum, _BIG)[median]
                box[median, 1] = _seg_reduce(k, thi_i[r], T, np.maximum, _SMALL)[median]
            nl = np.where(median, count // 2, nl)
            split_axis = np.where(median, 0, split_axis)
        nr = count - nl
        c0lo, c0hi = _grow(box0[:, 0], box0[:, 1], eps)
        c1lo, c1hi = _grow(box1[:, 0], box1[:, 1], eps)
        # ---- termination ---------------------------------------------------------------------------------------------------
        with np.errstate(all="ignore"):
            a_par = area(lo, hi)
            lcost = ((area(c0lo, c0hi) / a_par) * nl.astype(F)).astype(F)
            rcost = ((area(c1lo, c1hi) / a_par) * nr.astype(F)).astype(F)
            sub = (ct + ci * (lcost + rcost)).astype(F)
            leaf_cost = (ci * count.astype(F)).astype(F)
        ended = cand & (nl + nr <= tri_max) & (leaf_cost < sub)
        deep = level > max_depth - 2
        f0 = (nl <= tri_limit) | deep
        f1 = (nr <= tri_limit) | deep
        if level == 0 and ended[0]:                   # DEVIATION: the root is split anyway, both children leaves
            ended[0] = False
            f0[0] = f1[0] = True
        leaf = forced | ended
        inner = ~leaf
        st["costLeaves"] += int(ended.sum())
        st["medianFallbacks"] += int(median.sum())
        if deep:
            st["depthLeaves"] += int((inner & (nl > tri_limit)).sum() + (inner & (nr > tri_limit)).sum())
        if trace_levels is not None:
            trace_levels.append(dict(leaf=leaf.copy(), ended=ended.copy(), median=median.copy(), axis=split_axis.copy(),
                                     split=split_pos.copy(), nl=nl.copy(), nr=nr.copy(), count=count.copy(), k=best_k.copy(),
                                     box0=(c0lo, c0hi), box1=(c1lo, c1hi)))
        # ---- numbering -----------------------------------------------------------------------------------------------------
        node_idx = len(nodes) + np.cumsum(inner) - inner
        for t in range(T):
            if inner[t]:
                w = np.zeros(16, np.int32)
                f = w.view(F)
                f[0], f[1], f[2], f[3] = c0lo[t, 0], c0hi[t, 0], c0lo[t, 1], c0hi[t, 1]
                f[4], f[5], f[6], f[7] = c1lo[t, 0], c1hi[t, 0], c1lo[t, 1], c1hi[t, 1]
                f[8], f[9], f[10], f[11] = c0lo[t, 2], c0hi[t, 2], c1lo[t, 2], c1hi[t, 2]
                w[14] = split_axis[t]
                nodes.append(w)
                val = 64 * int(node_idx[t])
            else:
                s0, c = int(start[t]), int(count[t])
                leaf_blocks.append((rows, refs[s0:s0 + c].copy()))
                val = ~rows
                rows += 3 * c + 1
            if slot[t] >= 0:
                nodes[int(slot[t]) // 16][int(slot[t]) % 16] = val
        st["numLeaves"] += int(leaf.sum())
        ninner = int(inner.sum())
        st["numInnerNodes"] += ninner
        if ninner:
            st["maxDepth"] = level + 1
        it = np.flatnonzero(inner)
        if it.size == 0:
            break
        # ---- partition: child 0 (side -1 / first half) then child 1, stable ------------------------------------------------
        sa = split_axis[task_of]
        neg = np.where(median[task_of], pos_in < (count // 2)[task_of], side_neg(split_pos[task_of], cen[refs, sa]))
        order = np.lexsort((np.arange(refs.size), ~neg, task_of))
        order = order[inner[task_of][order]]
        for t in it:
            s0, c = int(start[t]), int(count[t])
            assert int(neg[s0:s0 + c].sum()) == int(nl[t]), "partition disagrees with the binning"
        refs = refs[order]
        count = np.stack([nl[it], nr[it]], 1).reshape(-1).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
        lo = np.stack([c0lo[it], c1lo[it]], 1).reshape(-1, 3)
        hi = np.stack([c0hi[it], c1hi[it]], 1).reshape(-1, 3)
        slot = np.stack([16 * node_idx[it] + 12, 16 * node_idx[it] + 13], 1).reshape(-1).astype(np.int64)
        forced = np.stack([f0[it], f1[it]], 1).reshape(-1)
        level += 1

    nodes = np.array(nodes, np.int32).reshape(-1, 16)
    woop = np.zeros((rows, 4), np.uint32)
    tidx = np.zeros(rows, np.int32)
    for r0, ids in leaf_blocks:
        k = ids.size
        if k:
            woop[r0:r0 + 3 * k] = woop12[ids].reshape(-1, 4).view(np.uint32)
            tidx[r0:r0 + 3 * k:3] = ids
        woop[r0 + 3 * k] = 0x80000000
    return dict(nodes=nodes, woop=woop.reshape(-1).view(np.uint8).copy(), tri_index=tidx, stats=st)


def leaves(r):
    """[(node, side, box lo, box hi, triangle ids, row)] of every leaf, walking the tree in level order; checks that the inner
    nodes are numbered in level order."""
    nodes = r["nodes"]
    woop = r["woop"].view(np.uint32).reshape(-1, 4)
    tidx = r["tri_index"]
    out, nxt, queue = [], 1, [0]
    while queue:
        new = []
        for i in queue:
            f = nodes[i].view(F)
            boxes = ((f[[0, 2, 8]], f[[1, 3, 9]]), (f[[4, 6, 10]], f[[5, 7, 11]]))
            for side in range(2):
                c = int(nodes[i][12 + side])
                if c >= 0:
                    assert c % 64 == 0 and c // 64 == nxt, "inner nodes not in level order"
                    nxt += 1
                    new.append(c // 64)
                    continue
                row = ~c
                ids = []
                while woop[row, 0] != 0x80000000:
                    ids.append(int(tidx[row]))
                    row += 3
                out.append((i, side, boxes[side][0], boxes[side][1], np.array(ids, np.int64), ~c))
        queue = new
    assert nxt == nodes.shape[0]
    return out


def check_invariants(r, tri, pos, params=None):
    """Every triangle in exactly one leaf, every leaf box containing its triangles, level order of nodes and leaf blocks, ids
    ascending in a leaf, leaf sizes within the limits (unless the depth cap made a leaf)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    lo, hi, _ = tri_terms(tri, pos)
    seen = np.zeros(tri.shape[0], np.int64)
    rows = []
    for _, _, blo, bhi, ids, row in leaves(r):
        seen[ids] += 1
        rows.append(row)
        if ids.size:
            assert (lo[ids] >= blo).all() and (hi[ids] <= bhi).all(), "box does not contain its triangles"
            assert list(ids) == sorted(ids), "leaf not in ascending triangle id"
        if r["stats"]["depthLeaves"] == 0:
            assert ids.size <= max(p["triLimit"], p["triMaxLimit"]), "leaf larger than the limits"
    assert (seen == 1).all(), "a triangle is not in exactly one leaf"
    assert rows == sorted(rows), "leaf blocks not in level order"
    return True
