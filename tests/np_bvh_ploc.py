"""numpy spec of ntr_ploc_build: PLOC (parallel locally-ordered clustering, Meister and Bittner 2018) over the LBVH's Morton order.

EXTENSION: the reference has no PLOC.  This docstring is the normative text; the device build (csrc/bvh_ploc_kernels.hip) equals
build() byte for byte in nodes, Woop rows, triIndex, rounds and height.

Inputs.  The mesh (tri, pos), the scene box (scene_min, scene_max) and the radius R in 1..64.

Order.  ntr_lbvh_build's Morton codes and stable sort (np_hlbvh.morton_sorted): the code of a triangle's box centre over the scene
  box, ties by ascending triangle id.  No triangle is dropped.

Leaves.  One triangle per leaf, in sorted order.  Leaf p owns rows 4p .. 4p + 3: the triangle's three Woop rows (woop_rows.h) and a
  terminator row of 0x80000000; its link is ~(4p).  The triIndex entry of the first row is the triangle id, the other three are 0.
  The leaf's box is min / max of its three vertices in the floats' total order (-0 < +0); there is no epsilon.

Clusters.  A cluster is (box, link, height).  The list starts as the leaves in sorted order, each of height 0.

A round, while the list has n > 1 clusters:
  1. distance    d(i, j) = fl(fl(fl(dx * dy) + fl(dy * dz)) + fl(dz * dx)) of the union box of clusters i and j, dx = fl(hi.x - lo.x)
                 and likewise dy, dz; no contraction; the union by min / max in the total order; a NaN counts as +inf.
  2. neighbour   the candidates of cluster i are all j != i with |i - j| <= R inside the list.  nn[i] is the candidate of least key
                 (d, k, b): k = |i - j|, b = (min(i, j) // k) & 1; d compared as floats (+0 == -0), then k, then b.
                 The key is symmetric in i and j.  For a fixed i no two candidates share (k, b): the two candidates at distance k are
                 i - k and i + k, whose min(i, j) // k are i // k - 1 and i // k, which differ by exactly 1 and so in their low bit.
                 Hence every cluster has exactly one neighbour, and the pair (i, j) that holds the least key of the whole list is
                 mutual: nn[i] == j since no other candidate of i has a key as low, and likewise nn[j] == i.  A round therefore merges
                 at least one pair and the loop ends after at most N - 1 rounds.  (The b term lets a run of identical clusters pair up
                 (0,1) (2,3) ... and halve per round, where ties by k alone would make every cluster point at its left neighbour and
                 merge one pair per round.)
  3. merge       i and j = nn[i] merge iff nn[j] == i.  With m merging pairs in the round, the pair whose lower index has rank r
                 (ascending, from 0) among the pairs' lower indices gets node slot (n - 1 - m) + r: slots are handed out from the top,
                 the last round (n == 2) writes slot 0, the root, and exactly N - 1 slots are written.  The node is a Compact node
                 (compact_bvh.h): child 0 is the lower-index cluster, child 1 the upper one, with their boxes and links as they
                 stand; word 14 is 0, word 15 is 0.
  4. compaction  the merged cluster takes the lower index's place: box the union, link 64 * slot, height 1 + max of the two; the
                 upper index disappears; everything else keeps its relative order.

N == 1.  One node: child 0 an empty leaf (box (FLT_MAX, -FLT_MAX), link ~0, a terminator row only), child 1 the triangle (link ~1,
  rows 1..3, a terminator at row 4) -- the rows ntr_persistent_bvh_build gives for one triangle.  No round; height 1.

Height.  The height of the last cluster: the number of inner nodes on the longest root-to-leaf path.  Above 100 (the reference CPU
  tracer's stack, the bound of ntr_persistent_bvh_build) the device reports NTR_ERR_OVERFLOW; build() still returns the tree and
  the height for the tests to look at.
"""
import numpy as np

import np_hlbvh

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
TERM = np.uint32(0x80000000)
MAX_HEIGHT = 100


def distance(lo_i, hi_i, a, b):
    """d of the clusters at index arrays a and b (boxes in the ordered-int encoding np_hlbvh.f2i)."""
    lo = np_hlbvh.i2f(np.minimum(lo_i[a], lo_i[b]))
    hi = np_hlbvh.i2f(np.maximum(hi_i[a], hi_i[b]))
    with np.errstate(over="ignore", invalid="ignore"):
        e = (hi - lo).astype(F)
        d = ((e[:, 0] * e[:, 1]).astype(F) + (e[:, 1] * e[:, 2]).astype(F)).astype(F)
        d = (d + (e[:, 2] * e[:, 0]).astype(F)).astype(F)
    return np.where(np.isnan(d), F(np.inf), d).astype(F)


def neighbours(lo_i, hi_i, radius):
    """nn[i] of every cluster of a list of n >= 2."""
    n = lo_i.shape[0]
    idx = np.arange(n, dtype=np.int64)
    best_d = np.full(n, np.inf, F)
    best_t = np.full(n, np.iinfo(np.int64).max, np.int64)   # 2 * k + b
    nn = np.full(n, -1, np.int64)

    def offer(who, cand, d, t):
        better = (d < best_d[who]) | ((d == best_d[who]) & (t < best_t[who]))
        w = who[better]
        best_d[w] = d[better]
        best_t[w] = t[better]
        nn[w] = cand[better]

    for k in range(1, min(radius, n - 1) + 1):
        a = idx[:n - k]
        d = distance(lo_i, hi_i, a, a + k)
        t = 2 * k + ((a // k) & 1)
        offer(a, a + k, d, t)        # the upper candidate of a
        offer(a + k, a, d, t)        # the lower candidate of a + k: the same key
    assert (nn >= 0).all()
    return nn


def build(tri, pos, scene_min, scene_max, radius=8, trace_rounds=None):
    """-> dict(nodes (S, 16) int32, woop bytes (uint8), tri_index int32, stats dict(numNodes, numLeaves, numRounds, height),
    sizes: the list length at the start of every round).  trace_rounds: a list that receives (nn, merged lower indices) per round."""
    tri = np.ascontiguousarray(tri, np.int32)
    pos = np.ascontiguousarray(pos, F)
    n = tri.shape[0]
    assert 1 <= radius <= 64 and n >= 1
    mn, mx = np.asarray(scene_min, F), np.asarray(scene_max, F)
    _, order = np_hlbvh.morton_sorted(tri, pos, mn, mx)
    rows = np_hlbvh.woop_rows(tri, pos).view(np.uint32).reshape(n, 3, 4)
    v = pos[tri[order]]
    lo_i, hi_i = np_hlbvh.f2i(v).min(axis=1), np_hlbvh.f2i(v).max(axis=1)

    if n == 1:
        woop = np.zeros((5, 4), np.uint32)
        woop[0] = TERM
        woop[1:4] = rows[0]
        woop[4] = TERM
        tri_index = np.array([0, 0, 0, 0, 0], np.int32)
        nodes = np.zeros((1, 16), np.int32)
        nf = nodes.view(F)
        lo, hi = np_hlbvh.i2f(lo_i[0]), np_hlbvh.i2f(hi_i[0])
        nf[0, 0:4] = (FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX)
        nf[0, 4:8] = (lo[0], hi[0], lo[1], hi[1])
        nf[0, 8:12] = (FLT_MAX, -FLT_MAX, lo[2], hi[2])
        nodes[0, 12], nodes[0, 13] = ~0, ~1
        return dict(nodes=nodes, woop=woop.view(np.uint8).reshape(-1), tri_index=tri_index,
                    stats=dict(numNodes=1, numLeaves=2, numRounds=0, height=1), sizes=[])

    woop = np.zeros((n, 4, 4), np.uint32)
    woop[:, :3] = rows[order]
    woop[:, 3] = TERM
    tri_index = np.zeros((n, 4), np.int32)
    tri_index[:, 0] = order
    nodes = np.zeros((n - 1, 16), np.int32)
    written = np.zeros(n - 1, bool)
    link = ~(4 * np.arange(n, dtype=np.int64))
    height = np.zeros(n, np.int64)
    sizes = []
    while lo_i.shape[0] > 1:
        c = lo_i.shape[0]
        sizes.append(c)
        nn = neighbours(lo_i, hi_i, radius)
        idx = np.arange(c, dtype=np.int64)
        mutual = nn[nn] == idx
        low = np.flatnonzero(mutual & (idx < nn))
        up = nn[low]
        m = low.shape[0]
        assert m >= 1
        if trace_rounds is not None:
            trace_rounds.append((nn.copy(), low.copy()))
        slot = (c - 1 - m) + np.arange(m, dtype=np.int64)
        assert not written[slot].any()
        written[slot] = True
        lo_f, hi_f = np_hlbvh.i2f(lo_i), np_hlbvh.i2f(hi_i)
        nf = nodes.view(F)
        for k, who in enumerate((low, up)):
            nf[slot, 4 * k + 0], nf[slot, 4 * k + 1] = lo_f[who, 0], hi_f[who, 0]
            nf[slot, 4 * k + 2], nf[slot, 4 * k + 3] = lo_f[who, 1], hi_f[who, 1]
            nf[slot, 8 + 2 * k], nf[slot, 9 + 2 * k] = lo_f[who, 2], hi_f[who, 2]
            nodes[slot, 12 + k] = link[who].astype(np.int32)
        lo_i, hi_i = lo_i.copy(), hi_i.copy()
        lo_i[low] = np.minimum(lo_i[low], lo_i[up])
        hi_i[low] = np.maximum(hi_i[low], hi_i[up])
        link[low] = 64 * slot
        height[low] = 1 + np.maximum(height[low], height[up])
        keep = np.ones(c, bool)
        keep[up] = False
        lo_i, hi_i, link, height = lo_i[keep], hi_i[keep], link[keep], height[keep]
    assert written.all() and link[0] == 0
    return dict(nodes=nodes, woop=woop.view(np.uint8).reshape(-1), tri_index=tri_index.reshape(-1),
                stats=dict(numNodes=n - 1, numLeaves=n, numRounds=len(sizes), height=int(height[0])), sizes=sizes)


def nested_scene(n, ratio=1.25, first=1.0):
    """Triangle k is (0,0,0), (s,0,0), (0,s,s) with s = first * ratio ** k: every union is the larger box, so the clusters merge one
    pair per round from the small end: a chain of height n - 1.  1.25 ** k leaves binary32 beyond k = 397 and its square beyond 198: a
    longer chain takes a smaller ratio and a first size below 1 (nested_long)."""
    pos = np.zeros((3 * n, 3), F)
    s = (F(first) * F(ratio) ** np.arange(n, dtype=F)).astype(F)
    assert np.isfinite(s).all() and (np.diff(s) > 0).all() and np.isfinite(s[-1] * s[-1]) and s[0] * s[0] > np.finfo(F).tiny
    pos[1::3, 0] = s
    pos[2::3, 1] = s
    pos[2::3, 2] = s
    return np.arange(3 * n, dtype=np.int32).reshape(-1, 3), pos


def nested_long(n):
    """nested_scene for chains of up to about 1 400 triangles: s = 2 ** -45 * 1.0625 ** k, whose squares stay normal binary32 numbers."""
    return nested_scene(n, 1.0625, 2.0 ** -45)


def scene_box(pos):
    pos = np.asarray(pos, F).reshape(-1, 3)
    return pos.min(axis=0), pos.max(axis=0)
