"""Level-by-level restatement of the full-sweep SAH BVH build: SAHBVHBuilder::run / build as they stand in
ntrace_amd/host/bvh/SAHBVHBuilder.cpp (the reference's src/rt/bvh/SAHBVHBuilder.cpp:51-254 by the presorted route) with
Platform("GPU") -- node cost 1, triangle cost 1, batch sizes 1 -- and leaf preferences (minLeaf, maxLeaf), in numpy binary32.  The
device build (ntr_sah_device_build, csrc/sah_build_kernels.hip) equals this module's three Compact buffers and counts byte for
byte; the host tree (ntr_sah_build) has the same nodes in another numbering (walk_equal below compares them link by link).

The rule:

  Per triangle.  box = min / max over its three vertices in the total order -0 < +0 (the one freedom against the host, whose
    FW::min / max give a zero the sign of whichever operand came first; no area, cost or decision sees a zero's sign).  Key on axis
    d = fl(box.min[d] + box.max[d]).  With size = box.max - box.min, a triangle with
    min(min(size.x, size.y), size.z) < 0  or  fl(fl(size.x + size.y) + size.z) == max(max(size.x, size.y), size.z)
    -- a negative extent, or at most one non-zero extent -- is DROPPED before the build and reaches no leaf
    (SAHBVHBuilder.cpp run(), reference :141-151).  The root's box is the union over every triangle, the dropped ones too (:70-84).
  Order.  Each axis' sequence of the live triangles: ascending key under float compare (-0 == +0), ties by ascending triangle id
    (:106-115).  The three sequences are made once; every node owns the same range [begin, end) of all three.  NaN coordinates are
    out of contract.
  Sweep of a node of m references, box area A (AABB::area: (dx*dy + dy*dz + dz*dx) * 2, each operation rounded, 0 for a box with
    min > max on an axis): nodeSAH = fl(A * 2).  For every axis d = 0, 1, 2 and i = 1 .. m-1, with L the union of the first i boxes
    of the axis' sequence and R the union of the other m - i (unions are exact, any grouping gives them):
      sah     = fl(fl(nodeSAH + fl(area(L) * fl(i))) + fl(area(R) * fl(m - i)))
      balance = fl(fl(fl(i) * fl(i)) + fl(fl(m - i) * fl(m - i)))
    The winner is the lexicographic minimum of (sah, balance, axis, i) under float < and ==, starting from
    (FLT_MAX, FLT_MAX, -, numLeft 0) (:221-232, bestSplit): a candidate takes part iff sah <= FLT_MAX -- a NaN or infinite sah never
    wins, and a sah of exactly FLT_MAX wins only over "no split" (its balance is below FLT_MAX), as the host's comparison chain has
    it.  A node without a winner (m < 2, or areas times counts that overflow) keeps the host's default split: axis 0, numLeft 0,
    sah FLT_MAX -- ALL references go to child 1, none to child 0 -- and so does its child 1, down to the depth-64 leaf.
  Leaves (:155-156, :163-165).  Before the search: level != 0 and m <= minLeaf, or level >= 64.  After it: level != 0 and
    FW::min(leafSAH, sah) == leafSAH and m <= maxLeaf, with leafSAH = fl(A * fl(m)), FW::min(a, b) = a < b ? a : b and sah the
    winner's (FLT_MAX without one).  The root is never a leaf.  A leaf lists its triangles BACK TO FRONT of the sequence its range
    was last arranged by (:193-203): axis 2 when the search has run, the parent's split axis when it has not.
  Children.  The first numLeft of the winning axis' sequence are child 0, the rest child 1; a stable partition by that side keeps
    the two other sequences sorted.  Child boxes are the exact unions; an empty child has the box (FLT_MAX, -FLT_MAX).  Node word 14
    is SplitInfo::getBitCode() (BVHNode.hpp): the axis for a SAH split, 0 (the default split's axis) without a winner; word 15 is 0.
  Layout.  CANONICAL for the device build (the host's createCompact numbers by an explicit stack instead): every child is a task of
    the next level, child 0 before child 1; inner nodes are numbered in level order, the root 0; leaves take their Woop blocks in
    the same order: three rows per triangle (woop_rows.h, the device builders' function) then a terminator row of 0x80000000; the
    triIndex entry of a triangle's first row is its id, every other entry 0.  16 words per node: child 0 x / y box, child 1 x / y
    box, the z boxes, child 0, child 1 (64 * index of an inner child, ~row of a leaf), word 14, 0.  Leaf boxes carry no epsilon.

Statistics: numInnerNodes, numLeaves (empty ones included), numLevels (rounds), maxDepth (inner nodes on the longest root-to-leaf
path), numDropped.
"""
import numpy as np

import np_hlbvh

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
MAX_DEPTH = 64
TERM = 0x80000000

_BIG = int(np_hlbvh.f2i(FLT_MAX))
_SMALL = int(np_hlbvh.f2i(-FLT_MAX))


def _i2f(a):
    return np_hlbvh.i2f(np.asarray(a).astype(np.int32)).astype(F)


def area(lo, hi):
    """AABB::area of boxes lo, hi ([..., 3]): 0 for an invalid box."""
    with np.errstate(all="ignore"):
        d = (hi - lo).astype(F)
        a = (((d[..., 0] * d[..., 1]) + (d[..., 1] * d[..., 2])) + (d[..., 2] * d[..., 0])) * F(2)
    return np.where((lo <= hi).all(axis=-1), a, F(0)).astype(F)


def tri_terms(tri, pos):
    """Per triangle: box lo, hi ([n, 3]), keys ([n, 3]), dropped ([n] bool)."""
    v = np.asarray(pos, dtype=F)[np.asarray(tri, dtype=np.int64)]          # [n, 3 verts, 3]
    i = np_hlbvh.f2i(v)
    lo = np_hlbvh.i2f(i.min(axis=1)).astype(F)
    hi = np_hlbvh.i2f(i.max(axis=1)).astype(F)
    with np.errstate(all="ignore"):
        key = (lo + hi).astype(F)
        size = (hi - lo).astype(F)
        smin = np.minimum(np.minimum(size[:, 0], size[:, 1]), size[:, 2])
        smax = np.maximum(np.maximum(size[:, 0], size[:, 1]), size[:, 2])
        ssum = ((size[:, 0] + size[:, 1]).astype(F) + size[:, 2]).astype(F)
    return lo, hi, key, (smin < 0) | (ssum == smax)


def sweep(lo_i, hi_i, node_sah):
    """One axis: lo_i, hi_i are the ordered-int boxes ([m, 3]) in the axis' order.  Returns (sah, balance, numLeft) of the axis' best
    split, (FLT_MAX, FLT_MAX, 0) without one."""
    m = lo_i.shape[0]
    if m < 2:
        return FLT_MAX, FLT_MAX, 0
    pre_lo, pre_hi = np.minimum.accumulate(lo_i, axis=0), np.maximum.accumulate(hi_i, axis=0)
    suf_lo = np.minimum.accumulate(lo_i[::-1], axis=0)[::-1]
    suf_hi = np.maximum.accumulate(hi_i[::-1], axis=0)[::-1]
    al = area(_i2f(pre_lo[:-1]), _i2f(pre_hi[:-1]))
    ar = area(_i2f(suf_lo[1:]), _i2f(suf_hi[1:]))
    fi = np.arange(1, m).astype(F)
    fr = (m - np.arange(1, m)).astype(F)
    with np.errstate(all="ignore"):
        sah = ((node_sah + (al * fi).astype(F)).astype(F) + (ar * fr).astype(F)).astype(F)
        bal = ((fi * fi).astype(F) + (fr * fr).astype(F)).astype(F)
    cand = sah <= FLT_MAX
    if not cand.any():
        return FLT_MAX, FLT_MAX, 0
    s = sah[cand].min()
    tie = cand & (sah == s)
    b = bal[tie].min()
    i = int(np.flatnonzero(tie & (bal == b))[0])
    return F(s), F(b), i + 1


def build(tri, pos, min_leaf=1, max_leaf=1, trace_levels=None):
    """The device build.  Returns dict(nodes int32[m, 16], woop uint8[], tri_index int32[], stats dict)."""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = tri.shape[0]
    assert n >= 1 and min_leaf >= 1 and max_leaf >= min_leaf
    tlo, thi, key, dropped = tri_terms(tri, pos)
    tlo_i, thi_i = np_hlbvh.f2i(tlo).astype(np.int64), np_hlbvh.f2i(thi).astype(np.int64)
    woop12 = np_hlbvh.woop_rows(tri, pos)
    live = np.flatnonzero(~dropped)
    # ascending key, ties by id: a stable sort of the ascending ids by key + 0 (-0 == +0)
    order = [live[np.argsort((key[live, d] + F(0)).astype(F), kind="stable")] for d in range(3)]
    side = np.zeros(n, bool)

    # a task: (begin, end, box lo_i, box hi_i as ordered ints, the axis its range was last arranged by, its parent's link word)
    root_lo, root_hi = tlo_i.min(axis=0), thi_i.max(axis=0)
    tasks = [(0, live.size, root_lo, root_hi, 2, -1)]
    nodes, leaf_blocks, rows = [], [], 0
    st = dict(numInnerNodes=0, numLeaves=0, numLevels=0, maxDepth=0, numDropped=int(dropped.sum()))
    empty_lo, empty_hi = np.full(3, _BIG, np.int64), np.full(3, _SMALL, np.int64)
    level = 0
    while tasks:
        st["numLevels"] += 1
        nxt = []
        first_node = len(nodes)
        decisions = []
        for (b, e, lo_i, hi_i, arranged, slot) in tasks:
            m = e - b
            leaf_order = None
            if (level != 0 and m <= min_leaf) or level >= MAX_DEPTH:
                leaf_order = arranged
            else:
                with np.errstate(all="ignore"):
                    a = area(_i2f(lo_i), _i2f(hi_i))
                    leaf_sah = F(a * F(m))
                    node_sah = F(a * F(2))
                best = (FLT_MAX, FLT_MAX, 0, 0)            # sah, balance, axis, numLeft
                for d in range(3):
                    ids = order[d][b:e]
                    s, bal, nl = sweep(tlo_i[ids], thi_i[ids], node_sah)
                    if s < best[0] or (s == best[0] and bal < best[1]):
                        best = (s, bal, d, nl)
                min_sah = leaf_sah if leaf_sah < best[0] else best[0]
                if level != 0 and min_sah == leaf_sah and m <= max_leaf:
                    leaf_order = 2
            if leaf_order is not None:
                ids = order[leaf_order][b:e][::-1].copy()
                leaf_blocks.append((rows, ids))
                val = ~rows
                rows += 3 * ids.size + 1
                st["numLeaves"] += 1
            else:
                _, _, axis, nl = best
                chosen = order[axis][b:e]
                side[chosen[:nl]] = True
                side[chosen[nl:]] = False
                for d in range(3):
                    if d != axis:
                        seq = order[d][b:e]
                        sd = side[seq]
                        order[d][b:e] = np.concatenate([seq[sd], seq[~sd]])
                boxes = []
                for ids in (chosen[:nl], chosen[nl:]):
                    boxes.append((tlo_i[ids].min(axis=0), thi_i[ids].max(axis=0)) if ids.size else (empty_lo, empty_hi))
                idx = len(nodes)
                w = np.zeros(16, np.int32)
                f = w.view(F)
                (l0, h0), (l1, h1) = [(_i2f(x), _i2f(y)) for x, y in boxes]
                f[0], f[1], f[2], f[3] = l0[0], h0[0], l0[1], h0[1]
                f[4], f[5], f[6], f[7] = l1[0], h1[0], l1[1], h1[1]
                f[8], f[9], f[10], f[11] = l0[2], h0[2], l1[2], h1[2]
                w[14] = axis
                nodes.append(w)
                val = 64 * idx
                nxt.append((b, b + nl, boxes[0][0], boxes[0][1], axis, 16 * idx + 12))
                nxt.append((b + nl, e, boxes[1][0], boxes[1][1], axis, 16 * idx + 13))
                decisions.append((b, e, axis, nl, best[0]))
            if slot >= 0:
                nodes[slot // 16][slot % 16] = val
        if len(nodes) > first_node:
            st["maxDepth"] = level + 1
        if trace_levels is not None:
            trace_levels.append(decisions)
        tasks = nxt
        level += 1

    st["numInnerNodes"] = len(nodes)
    nodes = np.array(nodes, np.int32).reshape(-1, 16)
    woop = np.zeros((rows, 4), np.uint32)
    tidx = np.zeros(rows, np.int32)
    for r0, ids in leaf_blocks:
        k = ids.size
        if k:
            woop[r0:r0 + 3 * k] = woop12[ids].reshape(-1, 4).view(np.uint32)
            tidx[r0:r0 + 3 * k:3] = ids
        woop[r0 + 3 * k] = TERM
    return dict(nodes=nodes, woop=woop.reshape(-1).view(np.uint8).copy(), tri_index=tidx, stats=st)


def leaf_ids(woop, tri_index, row):
    """The triangle ids of the leaf whose block starts at `row`, in the block's order."""
    w = np.asarray(woop).view(np.uint32).reshape(-1, 4)
    ids = []
    while w[row, 0] != TERM:
        ids.append(int(tri_index[row]))
        row += 3
    return ids


def walk_equal(a, b):
    """Walks two Compact trees (nodes, woop, tri_index) from their roots in lockstep, child 0 with child 0, and demands the same inner
    / leaf kind at every link, the 12 box floats equal as float values (-0 == +0, nothing else tolerated), word 14 equal and the same
    triangle id sequence in every leaf.  Returns (inner nodes, leaves) visited."""
    na = np.asarray(a[0]).view(np.int32).reshape(-1, 16)
    nb = np.asarray(b[0]).view(np.int32).reshape(-1, 16)
    stack, inner, leaves = [(0, 0)], 0, 0
    while stack:
        ia, ib = stack.pop()
        inner += 1
        wa, wb = na[ia], nb[ib]
        fa, fb = wa[:12].view(F), wb[:12].view(F)
        assert np.array_equal(fa, fb), ("box", ia, ib, fa, fb)
        assert wa[14] == wb[14], ("word 14", ia, ib, int(wa[14]), int(wb[14]))
        for k in (12, 13):
            ca, cb = int(wa[k]), int(wb[k])
            assert (ca < 0) == (cb < 0), ("kind", ia, ib, k)
            if ca < 0:
                la, lb = leaf_ids(a[1], a[2], ~ca), leaf_ids(b[1], b[2], ~cb)
                assert la == lb, ("leaf", ia, ib, k, la, lb)
                leaves += 1
            else:
                assert ca % 64 == 0 and cb % 64 == 0
                stack.append((ca // 64, cb // 64))
    return inner, leaves


def check_layout(r):
    """Level-order numbering of inner nodes and leaf blocks, terminators, triIndex zeros and the extents against the counts."""
    nodes, tidx = r["nodes"], r["tri_index"]
    woop = r["woop"].view(np.uint32).reshape(-1, 4)
    st = r["stats"]
    assert nodes.shape[0] == st["numInnerNodes"] and woop.shape[0] == tidx.shape[0]
    nxt, row, queue, leaves, tris, depth = 1, 0, [0], 0, 0, 0
    while queue:
        depth += 1
        new = []
        for i in queue:
            assert nodes[i][15] == 0
            for side in range(2):
                c = int(nodes[i][12 + side])
                if c >= 0:
                    assert c == 64 * nxt, "inner nodes not in level order"
                    nxt += 1
                    new.append(c // 64)
                    continue
                assert ~c == row, "leaf blocks not in level order"
                while woop[row, 0] != TERM:
                    assert tidx[row + 1] == 0 and tidx[row + 2] == 0
                    tris += 1
                    row += 3
                assert (woop[row] == TERM).all() and tidx[row] == 0
                row += 1
                leaves += 1
        queue = new
    assert nxt == nodes.shape[0] and row == woop.shape[0]
    assert leaves == st["numLeaves"] and depth == st["maxDepth"] and st["numLevels"] == depth + 1
    return tris
