"""Independent restatement of the on-device kd-tree build (ntr_kdtree_device_build, csrc/kdtree_build_kernels.hip): the
reference's persistent kd-tree builder as it is configured -- CudaTracerDefines.h SPLIT_TYPE 5, PLANE_COUNT 32,
TRIANGLE_CLIPPING 0, BINNING_TYPE 2; config.conf block PersistentKDTree -- rebuilt breadth first, one level per round, in
vectorised numpy binary32.  The device build's three buffers, scene box and counts equal this module's byte for byte.

The rule (persistent_kdtree.cu, rt_common.cu, CudaPersistentKDTreeBuilder.cpp):

  Candidates (findPlaneAABB, rt_common.cu:1007-1030; taskFinishBinning, persistent_kdtree.cu:2282-2470).  Plane k = 0..31 of
    a task lies on axis k // 11 (planesPerAxis = (32 + 2) // 3 = 11, so x and y get 11 planes and z gets 10) at
    pos = lo[a] + (hi[a] - lo[a]) * rpos, rpos = float32(1 + k % 11) / float32(12), both operations rounded on their own
    (no fused multiply-add: the library is built with -ffp-contract=off).  pos lies in [lo[a], hi[a]].
  Classification (getPlanePosition, rt_common.cu:331-400, EPS = 1e-8f; the binning's `pos <= 0` -> left, `pos >= 0` -> right).
    With the plane (-1, 0, 0, pos) the distance of a vertex is fl(pos - x).  The triangle counts left iff some vertex has
    fl(pos - x) > -EPS and right iff some vertex has fl(pos - x) < EPS.  Rounded subtraction is monotone in x, so over the
    three vertices these are exactly fl(pos - xmin) > -EPS and fl(pos - xmax) < EPS: the build needs only each triangle's
    box.  A triangle touching or lying in the plane counts on both sides; nothing is clipped.
  Cost (areaAABB / areaAABBX/Y/Z, rt_common.cu:850-905).  s_k = areaL * float(nL) + areaR * float(nR) with
    area = (dx*dy + dy*dz + dz*dx) * 2 over the cell cut at pos.  The counts are integers, so the binning is exact.
  Split choice (the warp's min-reduction + first-lane ballot).  CANONICAL: among the planes whose s_k is finite, the lowest
    s_k wins (+0 and -0 are equal), then the lowest k -- that is, the lower axis, then the lower plane.  A NaN or infinite
    s_k never wins.  If no plane has a finite s_k (areas that overflow binary32), the task is a leaf (the reference would keep
    whatever plane its task record held).
  Termination (taskTerminationCriteria, persistent_kdtree.cu:454-510).  With the chosen plane,
    subdivisionCost = ct + ci * s / areaParent, leafCost = ci * float(n).  If subdivisionCost / leafCost > failRq the task's
    failure counter is incremented and, when it exceeds failureCount, the task is a leaf holding all its references.  A NaN
    ratio (a cell with zero area: zero extent in two axes) is not > failRq, so such a cell keeps subdividing, as in the
    reference.  Otherwise the task is an inner node and each child with <= triLimit references, or whose parent's depth
    is > maxDepth - 2, is a leaf (an empty one when it has none).  Children inherit the parent's failure counter after the
    increment (taskChildTask, persistent_kdtree.cu:912-913).  maxDepth = int(depthK1 * log2f(numTris) + depthK2)
    (CudaPersistentKDTreeBuilder.cpp:451); the root's depth is 0.  triMaxLimit is read by the reference only in its
    object-SAH path (persistent_kdtree.cu:4710, not compiled with SPLIT_TYPE 5) and has no effect here.
  DEVIATION: the reference's builder overwrites failureCount with int(failK1 * maxDepth + failK2)
    (CudaPersistentKDTreeBuilder.cpp:452); here failureCount is the parameter as given (config.conf: 0).
  Cells.  The root cell is the box of all triangles' vertices, its min / max taken in the total order -0 < +0.  A child's
    cell is the parent's with hi[axis] = pos (child 0) or lo[axis] = pos (child 1): the reference's fminf / fmaxf
    (taskCreateSubtask, persistent_kdtree.cu:932-980) with the plane inside the cell.  A plane that coincides with a cell
    face (a flat cell, or rounding at a tiny extent) is evaluated like any other.
  Root.  A root with <= triLimit triangles is a leaf, and so is a root that the failure test or the no-finite-cost rule ends.
    DEVIATION (as CudaKDTree): such a tree is one inner node on axis 0 at sceneMax.x over the leaf (child 0) and an empty
    leaf (child 1).
  Order.  A straddling reference goes to both children; the partition is stable, so every leaf lists its triangle ids in
    ascending order.  Inner nodes are numbered in level order, the root 0, child 0 before child 1; leaf lists are written to
    triIndex in the same order, each followed by 0x80000000; an empty leaf is the child value 0x80000000.

Every task -- including a child already known to be a leaf -- is a task of the next level, so a level's leaves and inner
nodes are both decided in that level's round.  Statistics: numInnerNodes, numLeafNodes (empty ones included),
numEmptyLeaves, numTriRefs (references in leaves), maxDepth (inner nodes on the longest path), numLevels (rounds) and
percentDuplicates = float(numTriRefs - numTris) / float(numTris) * 100.
"""
import numpy as np

import np_hlbvh
import np_kdtree

F = np.float32
EPS = F(1e-8)
EMPTY = -2147483648
PLANES = 32
PER_AXIS = (PLANES + 2) // 3                                    # 11
PLANE_AXIS = np.minimum(np.arange(PLANES) // PER_AXIS, 2)       # 11 x, 11 y, 10 z
RPOS = (np.arange(PLANES) % PER_AXIS + 1).astype(F) / F(PER_AXIS + 1)

DEFAULTS = dict(triLimit=16, triMaxLimit=16, failureCount=0, depthK1=1.2, depthK2=2.0, ci=1.0, ct=1.0, failRq=0.9)


def max_depth(num_tris, k1=1.2, k2=2.0):
    """CudaPersistentKDTreeBuilder.cpp:451: int(k1 * log2f(n) + k2) in binary32."""
    with np.errstate(all="ignore"):
        v = F(F(k1) * np.log2(F(num_tris)) + F(k2))
    return int(v)


def plane_positions(lo, hi):
    """[T, 32] candidate positions of tasks with cells lo, hi ([T, 3])."""
    a = PLANE_AXIS
    with np.errstate(all="ignore"):
        return (lo[:, a] + (hi[:, a] - lo[:, a]) * RPOS[None, :]).astype(F)


def split_areas(lo, hi, axis, pos):
    """areaAABBX/Y/Z: (areaL, areaR) of cells lo, hi ([m, 3]) cut on axis ([m]) at pos ([m])."""
    d = (hi - lo).astype(F)
    m = np.arange(lo.shape[0])
    with np.errstate(all="ignore"):
        dl = d.copy()
        dl[m, axis] = pos - lo[m, axis]
        dr = d.copy()
        dr[m, axis] = hi[m, axis] - pos
        return area(dl), area(dr)


def area(d):
    with np.errstate(all="ignore"):
        return ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]) * F(2)


def classify(pos, tmin, tmax):
    """(left, right) of triangles with extents tmin / tmax on the plane's axis against the plane at pos."""
    with np.errstate(all="ignore"):
        return (pos - tmin) > -EPS, (pos - tmax) < EPS


def tri_boxes(tri, pos):
    v = np.asarray(pos, dtype=F)[np.asarray(tri, dtype=np.int64)]           # [n, 3, 3]
    return v.min(axis=1), v.max(axis=1)


def scene_box(tri, pos):
    """Box of the triangles' vertices, min / max in the order -0 < +0."""
    v = np.asarray(pos, dtype=F)[np.asarray(tri, dtype=np.int64)].reshape(-1, 3)
    i = np_hlbvh.f2i(v)
    return np_hlbvh.i2f(i.min(axis=0)).astype(F), np_hlbvh.i2f(i.max(axis=0)).astype(F)


def build(tri, pos, params=None, woop=True, trace_levels=None):
    """The device build.  Returns dict(nodes int32[n, 4], tri_index int32[], woop uint8[] (None if woop=False), scene_min,
    scene_max float32[3], delta float32, stats dict).  trace_levels: a list that receives each level's decisions."""
    p = dict(DEFAULTS)
    p.update(params or {})
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = tri.shape[0]
    assert n >= 1
    tri_limit, fail_count = int(p["triLimit"]), int(p["failureCount"])
    ci, ct, fail_rq = F(p["ci"]), F(p["ct"]), F(p["failRq"])
    mdepth = max_depth(n, p["depthK1"], p["depthK2"])
    tlo, thi = tri_boxes(tri, pos)
    smin, smax = scene_box(tri, pos)

    # level state
    lo = smin[None, :].copy()
    hi = smax[None, :].copy()
    ref_start = np.array([0], np.int64)
    ref_count = np.array([n], np.int64)
    parent_slot = np.array([-1], np.int64)
    fail = np.array([0], np.int64)
    forced = np.array([n <= tri_limit])
    refs = np.arange(n, dtype=np.int64)

    nodes = []                                           # flat int list, 4 per inner node
    tri_index = []
    inner_base = 0
    st = dict(numInnerNodes=0, numLeafNodes=0, numEmptyLeaves=0, numTriRefs=0, maxDepth=0, numLevels=0)
    level = 0
    root_leaf = False
    while ref_count.size:
        T = ref_count.size
        st["numLevels"] += 1
        task_of = np.repeat(np.arange(T), ref_count)
        # ---- count + decide -------------------------------------------------------------------------------------------
        leaf = forced.copy()
        best = np.zeros(T, np.int64)
        split = np.zeros(T, F)
        nl = np.zeros(T, np.int64)
        nr = np.zeros(T, np.int64)
        fail_out = fail.copy()
        cand = np.flatnonzero(~forced)
        if cand.size:
            planes = plane_positions(lo[cand], hi[cand])                   # [C, 32]
            cnt_l = np.zeros((cand.size, PLANES), np.int64)
            cnt_r = np.zeros((cand.size, PLANES), np.int64)
            sel = np.isin(task_of, cand)
            cidx = np.searchsorted(cand, task_of[sel])
            rt = refs[sel]
            for k in range(PLANES):
                a = PLANE_AXIS[k]
                l, r = classify(planes[cidx, k], tlo[rt, a], thi[rt, a])
                cnt_l[:, k] = np.bincount(cidx, weights=l, minlength=cand.size).astype(np.int64)
                cnt_r[:, k] = np.bincount(cidx, weights=r, minlength=cand.size).astype(np.int64)
            s = np.empty((cand.size, PLANES), F)
            for k in range(PLANES):
                al, ar = split_areas(lo[cand], hi[cand], np.full(cand.size, PLANE_AXIS[k]), planes[:, k])
                with np.errstate(all="ignore"):
                    s[:, k] = al * cnt_l[:, k].astype(F) + ar * cnt_r[:, k].astype(F)
            fin = np.isfinite(s)
            key = np.where(fin, s, F(np.inf))
            k_best = np.argmin(key, axis=1)
            m = np.arange(cand.size)
            none = ~fin.any(axis=1)
            s_best = s[m, k_best]
            ax = PLANE_AXIS[k_best]
            pb = planes[m, k_best]
            with np.errstate(all="ignore"):
                d = (hi[cand] - lo[cand]).astype(F)
                a_par = area(d)
                sub = ct + (ci * s_best) / a_par
                ratio = sub / (ci * ref_count[cand].astype(F))
            failed = ratio > fail_rq
            fo = fail[cand] + failed
            is_leaf = none | (failed & (fo > fail_count))
            leaf[cand] = is_leaf
            best[cand] = k_best
            split[cand] = pb
            nl[cand] = cnt_l[m, k_best]
            nr[cand] = cnt_r[m, k_best]
            fail_out[cand] = fo
        axis = PLANE_AXIS[best]
        if trace_levels is not None:
            trace_levels.append(dict(leaf=leaf.copy(), plane=best.copy(), split=split.copy(), nl=nl.copy(), nr=nr.copy(),
                                     count=ref_count.copy()))
        inner = ~leaf
        if level == 0 and leaf[0]:
            root_leaf = True
        # ---- numbering (the task scan) ------------------------------------------------------------------------------
        ninner = int(inner.sum())
        node_idx = inner_base + np.cumsum(inner) - inner
        leaf_out = np.where(leaf & (ref_count > 0), ref_count + 1, 0)
        leaf_off = len(tri_index) + np.cumsum(leaf_out) - leaf_out
        nodes.extend([0] * (4 * ninner))
        for t in range(T):
            ps = int(parent_slot[t])
            if inner[t]:
                b = 4 * int(node_idx[t])
                nodes[b + 2] = int(np.array([split[t]], F).view(np.int32)[0])
                nodes[b + 3] = int(axis[t]) << 28
                val = int(node_idx[t])
            else:
                val = ~int(leaf_off[t]) if ref_count[t] > 0 else EMPTY
            if ps >= 0:
                nodes[ps] = val
        # ---- leaves --------------------------------------------------------------------------------------------------
        for t in np.flatnonzero(leaf):
            c = int(ref_count[t])
            if c:
                s0 = int(ref_start[t])
                tri_index.extend(refs[s0:s0 + c].tolist())
                tri_index.append(EMPTY)
        st["numLeafNodes"] += int(leaf.sum())
        st["numEmptyLeaves"] += int((leaf & (ref_count == 0)).sum())
        st["numTriRefs"] += int(ref_count[leaf].sum())
        if ninner:
            st["maxDepth"] = level + 1
        st["numInnerNodes"] += ninner
        inner_base += ninner
        # ---- partition: children of the inner tasks, child 0 then child 1 ---------------------------------------------
        it = np.flatnonzero(inner)
        if it.size == 0:
            break
        ax_r = axis[task_of]
        l_bit, r_bit = classify(split[task_of], tlo[refs, ax_r], thi[refs, ax_r])
        new_refs = []
        n_lo, n_hi, n_start, n_count, n_slot, n_fail, n_forced = [], [], [], [], [], [], []
        off = 0
        for t in it:
            s0, c = int(ref_start[t]), int(ref_count[t])
            seg = refs[s0:s0 + c]
            for side, bits in ((0, l_bit[s0:s0 + c]), (1, r_bit[s0:s0 + c])):
                part = seg[bits]
                new_refs.append(part)
                clo, chi = lo[t].copy(), hi[t].copy()
                if side == 0:
                    chi[axis[t]] = split[t]
                else:
                    clo[axis[t]] = split[t]
                n_lo.append(clo)
                n_hi.append(chi)
                n_start.append(off)
                n_count.append(part.size)
                off += part.size
                n_slot.append(4 * int(node_idx[t]) + side)
                n_fail.append(int(fail_out[t]))
                n_forced.append(part.size <= tri_limit or level > mdepth - 2)
            assert (nl[t], nr[t]) == (int(l_bit[s0:s0 + c].sum()), int(r_bit[s0:s0 + c].sum()))
        refs = np.concatenate(new_refs).astype(np.int64) if new_refs else np.zeros(0, np.int64)
        lo = np.array(n_lo, F).reshape(-1, 3)
        hi = np.array(n_hi, F).reshape(-1, 3)
        ref_start = np.array(n_start, np.int64)
        ref_count = np.array(n_count, np.int64)
        parent_slot = np.array(n_slot, np.int64)
        fail = np.array(n_fail, np.int64)
        forced = np.array(n_forced, bool)
        level += 1

    if root_leaf:
        nodes = [~0, EMPTY, int(np.array([smax[0]], F).view(np.int32)[0]), 0]
        tri_index = list(range(n)) + [EMPTY]
        st.update(numInnerNodes=1, numLeafNodes=2, numEmptyLeaves=1, numTriRefs=n, maxDepth=1)
    nodes = np.array(nodes, dtype=np.int64).astype(np.int32).reshape(-1, 4)
    tri_index = np.array(tri_index, dtype=np.int64).astype(np.int32)
    st["percentDuplicates"] = float(F(st["numTriRefs"] - n) / F(n) * F(100))
    st["depthLimit"] = mdepth
    out = dict(nodes=nodes, tri_index=tri_index, scene_min=smin, scene_max=smax, delta=np_kdtree.delta_of(smin, smax), stats=st,
               woop=None)
    if woop:
        out["woop"] = woop_buffer(tri, pos)
    return out


def woop_buffer(tri, pos):
    """The device builders' rows (woop_rows.h, calcWoopKernel) by triangle id, the buffer padded to 4096 B (CudaKDTree)."""
    rows = np_hlbvh.woop_rows(np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F))
    n = rows.shape[0]
    buf = np.zeros(((n * 48 + 4095) // 4096) * 4096, np.uint8)
    buf[:n * 48] = rows.view(np.uint8).reshape(-1)
    return buf
