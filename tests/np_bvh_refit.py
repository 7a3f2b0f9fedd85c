"""The rule of the on-device BVH refit (ntr_bvh_refit, csrc/bvh_refit_kernels.hip) in vectorised numpy binary32.  The refit is an
EXTENSION: the reference's scenes are static and it has no refit, so this docstring, not a reference line, is the normative text.
The device's node buffer, Woop rows and scene box equal this module's byte for byte.

Input: a BVHLayout_Compact tree (nodes: 16 words per 64-byte slot -- c0 lo.x hi.x lo.y hi.y, c1 lo.x hi.x lo.y hi.y, c0 lo.z hi.z,
c1 lo.z hi.z, child 0, child 1, split word, a fourth word; an inner child is the byte offset 64 * index, a leaf child ~row; triWoop:
per leaf 3 rows per triangle then a terminator row whose first word is 0x80000000; triIndex: per row, the triangle id at a
triangle's first row), the mesh (tri [n, 3], pos [v, 3]) and epsilon >= 0.

1. Topology stays.  Child words, the split word and the fourth word of the link float4, the terminators, triIndex, the rows behind a
   leaf's terminator and every node slot no link reaches come back untouched.  Reached means: the root (slot 0), and every slot
   named by a positive child word of a reached slot.  A child word 0 names nobody (the root is no child), so a zero-filled slot
   inside the extent (NtrLbvhResult) -- which reads as "two inner children at offset 0" -- is neither reached nor a parent.
2. Woop rows.  The rows r, r+1, r+2 of each row group of a leaf (r = ~child, r + 3, ... up to the first group whose first word is the
   terminator) are woop_rows.h of triangle triIndex[r] over the new positions: the device builders' function, restated by
   np_hlbvh.woop_rows (shared with np_bvh_binned), so the rows equal a fresh device build's bit for bit.
3. Leaf box.  Per axis lo = the minimum and hi = the maximum over the three vertices of every triangle of the leaf, then
   fl(lo - epsilon), fl(hi + epsilon) in binary32 (the LBVH's rule, emitTreeKernel.cu:417-562; epsilon 0 is the exact union, which
   CudaBVH::createCompact stores for a host SAH tree).  A leaf without rows (the one-triangle tree's empty child 0) keeps its box
   words.
4. Inner box.  The box of an inner child is the union of the two boxes stored in that child's node.  Epsilon is applied at leaves
   only.
5. Minimum and maximum are taken in the float-order integer encoding (np_hlbvh.f2i, the device's ord_enc): a total order with
   -0 < +0, so no result depends on the order of the operands.  NaN coordinates are out of contract: the result is unspecified.
6. Scene box: the union of the root's two boxes, as min.xyz max.xyz.

stats: numNodes (reached slots), numLeaves (leaf children of reached slots), numRows (their rows, terminators included).
"""
import numpy as np

import np_bvh_binned as bb

np_hlbvh = bb.np_hlbvh
F = np.float32
TERM = 0x80000000

# words of child k's box inside a node, as lo.x hi.x lo.y hi.y lo.z hi.z
BOX_WORDS = (np.array([0, 1, 2, 3, 8, 9]), np.array([4, 5, 6, 7, 10, 11]))
LO, HI = np.array([0, 2, 4]), np.array([1, 3, 5])


def _union(a, b):
    """Union of boxes a, b ([m, 6] float32 as lo.x hi.x lo.y hi.y lo.z hi.z) in the f2i order."""
    ia, ib = np_hlbvh.f2i(a), np_hlbvh.f2i(b)
    out = np.empty_like(ia)
    out[:, LO] = np.minimum(ia[:, LO], ib[:, LO])
    out[:, HI] = np.maximum(ia[:, HI], ib[:, HI])
    return np_hlbvh.i2f(out).astype(F)


def levels_of(ni):
    """Reached node slots by depth: a list of index arrays, [0] first."""
    S = ni.shape[0]
    seen = np.zeros(S, bool)
    seen[0] = True
    levels = [np.array([0], np.int64)]
    while levels[-1].size:
        c = ni[levels[-1], 12:14].reshape(-1).astype(np.int64)
        c = c[c > 0]
        assert (c % 64 == 0).all() and (c // 64 < S).all(), "child link outside the node extent"
        nxt = c // 64
        assert not seen[nxt].any() and np.unique(nxt).size == nxt.size, "not a tree"
        seen[nxt] = True
        levels.append(nxt)
    return levels[:-1]


def leaf_rows(ni, woop_u32, levels):
    """Leaf children of the reached slots and their row groups: (leaf node, leaf slot, per group: leaf number, first row)."""
    slots = np.concatenate(levels)
    links = ni[slots, 12:14]
    node = np.repeat(slots, 2).reshape(-1, 2)[links < 0]
    k = np.tile(np.array([0, 1]), slots.size).reshape(-1, 2)[links < 0]
    cur = (~links[links < 0]).astype(np.int64)
    active = np.arange(cur.size)
    of_leaf, rows = [], []
    while active.size:
        r = cur[active]
        live = woop_u32[r, 0] != TERM
        active, r = active[live], r[live]
        of_leaf.append(active)
        rows.append(r)
        cur[active] = r + 3
    return node, k, np.concatenate(of_leaf) if of_leaf else np.zeros(0, np.int64), np.concatenate(rows) if rows else np.zeros(0, np.int64)


def refit(nodes, woop, tri_index, tri, pos, epsilon):
    """Returns dict(nodes int32[slots, 16], woop uint8[], scene_box float32[6], stats dict)."""
    ni = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16).copy()
    nf = ni.view(F)
    w = np.ascontiguousarray(woop).reshape(-1).view(np.uint32).reshape(-1, 4).copy()
    tidx = np.ascontiguousarray(tri_index, np.int32).reshape(-1)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    eps = F(epsilon)
    assert eps >= 0 and np.isfinite(eps)

    levels = levels_of(ni)
    leaf_node, leaf_k, of_leaf, rows = leaf_rows(ni, w, levels)
    L = leaf_node.size
    if rows.size:
        t = tidx[rows].astype(np.int64)
        assert (t >= 0).all() and (t < tri.shape[0]).all()
        r12 = np_hlbvh.woop_rows(np.ascontiguousarray(tri[t]), pos).view(np.uint32).reshape(-1, 3, 4)
        for j in range(3):
            w[rows + j] = r12[:, j]
        # rule 3: per-leaf min / max over the vertices in the f2i order, then -/+ epsilon
        vi = np_hlbvh.f2i(pos[tri[t]]).astype(np.int64)                 # [m, 3 verts, 3 axes]
        lo_i = np.full((L, 3), np.iinfo(np.int64).max)
        hi_i = np.full((L, 3), np.iinfo(np.int64).min)
        np.minimum.at(lo_i, of_leaf, vi.min(axis=1))
        np.maximum.at(hi_i, of_leaf, vi.max(axis=1))
        full = np.zeros(L, bool)
        full[of_leaf] = True
        with np.errstate(all="ignore"):
            lo = (np_hlbvh.i2f(lo_i[full]).astype(F) - eps).astype(F)
            hi = (np_hlbvh.i2f(hi_i[full]).astype(F) + eps).astype(F)
        box = np.empty((lo.shape[0], 6), F)
        box[:, LO], box[:, HI] = lo, hi
        for k in (0, 1):
            sel = leaf_k[full] == k
            nf[leaf_node[full][sel][:, None], BOX_WORDS[k][None, :]] = box[sel]

    # rule 4, deepest level first: by then both boxes inside every child node are final
    for slots in reversed(levels):
        for k in (0, 1):
            c = ni[slots, 12 + k].astype(np.int64)
            par, ch = slots[c > 0], c[c > 0] // 64
            if par.size:
                nf[par[:, None], BOX_WORDS[k][None, :]] = _union(nf[ch][:, BOX_WORDS[0]], nf[ch][:, BOX_WORDS[1]])
    root = _union(nf[0:1, BOX_WORDS[0]], nf[0:1, BOX_WORDS[1]])[0]
    scene_box = np.concatenate([root[LO], root[HI]]).astype(F)
    stats = dict(numNodes=int(sum(s.size for s in levels)), numLeaves=int(L), numRows=int(rows.size * 3 + L))
    return dict(nodes=ni, woop=w.reshape(-1).view(np.uint8).copy(), scene_box=scene_box, stats=stats)


# ---- the deformations the tests move the meshes by (deterministic, binary32) ----------------------------------------------
DEFORM_K = F(9.0)                      # waves per scene diagonal, in radians: k = DEFORM_K / d
DEFORM_PHASE = np.array([0.3, 1.1, 2.3], F)


def diagonal(pos):
    pos = np.asarray(pos, F).reshape(-1, 3)
    e = (pos.max(axis=0) - pos.min(axis=0)).astype(np.float64)
    return F(np.sqrt((e * e).sum()))


def deform(pos, a):
    """pos' = pos + a * d * sin(k * pos[:, (1, 2, 0)] + phase), d the scene diagonal, every operation in binary32."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    d = diagonal(pos)
    if not d > 0:
        d = F(1)
    k = F(DEFORM_K / d)
    with np.errstate(all="ignore"):
        s = np.sin((k * pos[:, (1, 2, 0)]).astype(F) + DEFORM_PHASE).astype(F)
        return np.ascontiguousarray((pos + (F(F(a) * d) * s).astype(F)).astype(F))


def collapse(pos):
    """Every vertex moved to one point: all triangles degenerate, all boxes one point -/+ epsilon."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    return np.ascontiguousarray(np.tile(np.array([[0.25, -1.5, 3.0]], F), (pos.shape[0], 1)))


def moved(pos, how):
    """how: a float amplitude for deform, or "collapse"."""
    return collapse(pos) if how == "collapse" else deform(pos, how)
