"""The rule of the in-place refit of 4-wide trees (ntr_pool_wide_refit, csrc/wide_refit_batch_kernels.hip; ntr_tlas_wide_refit,
csrc/tlas_wide_refit_kernels.hip) in numpy binary32.  EXTENSION without a reference counterpart: this docstring is the normative text,
and the device's buffers equal this module's byte for byte.  The wide node is np_bvh_wide's, the wide pool and the wide record are
np_instanced_wide's, the leaf rule is np_bvh_refit's and the instance box is np_instanced's; they are imported, not restated.

refit_wide_blas(wide_nodes, woop, tri_index, tri, pos, epsilon, rewrite_rows): one wide tree whose links are relative to its own start.
1. Topology stays.  Words 12..15 and 28..31 of every wide node come back untouched, and so does every word of a wide node no link
   reaches (reached: node 0 and every node named by a link > 0 of a reached node), every terminator, triIndex and the rows behind a
   leaf's terminator.
2. Woop rows.  With rewrite_rows the rows of every leaf's row groups are np_bvh_refit's rule 2 (woop_rows.h over the new positions):
   bit for bit what ntr_bvh_refit_batch writes.  Without it the rows are only read, to find terminators and triIndex.
3. Leaf box.  Slot k < count with link < 0 gets np_bvh_refit's rule 3 over the leaf's triangles: min and max in the np_hlbvh.f2i total
   order, then fl(lo - eps), fl(hi + eps).  A leaf whose first row group is the terminator keeps its box words.
4. Inner box.  Slot k < count with link > 0 gets the union, in the f2i order, of the boxes of slots 0..count-1 of the node it names.
   Epsilon applies at leaves only.
5. Link 0 in a slot k < count: the slot keeps its box words and still takes part in its node's union, as np_bvh_refit's empty leaf.
6. Padding.  Slot k >= count keeps its link (0) and is a copy of slot 0's new box: np_bvh_wide's invariant "every box word of the wide
   tree is a box word of the binary tree".
7. Root box: the union of node 0's slots 0..count-1, as min.xyz max.xyz.
8. stats: numNodes, the reached wide nodes; numLeafLinks, the negative links (k < count) of reached nodes; numRows, as np_bvh_refit
   counts them (three per triangle and one terminator per leaf).
9. A bad part is never followed.  err_bits are ntr_bvh_refit's: 1 link, 2 row outside the extent, 4 triangle index, 8 vertex index.
   Bit 1 also covers a link > 0 that is no multiple of 128 or lies outside the tree's extent, a node named by two links, and a count
   word outside 2..4.  What the box words of a malformed tree hold afterwards is unspecified (here: a box is rewritten where everything
   below it is well formed, and the root box of such a tree is six zeros); rule 1 still holds for it, and every other tree of a batch
   is refitted completely.

refit_wide_pool(entries, wide_pool_nodes, pool_woop, pool_tri_index, tri, pos, rewrite_rows) applies refit_wide_blas to every entry's
slices.  An entry is (wideNodesOffset, wideNodesBytes, triWoopOffset, triWoopBytes, firstTri, numTris, epsilon): NtrWideRefitEntry's
fields.  Every byte outside the listed ranges stays; the boxes are 6 floats per entry, in entry order.

refit_wide_tlas(wide_tlas_nodes, root_link, wide_records, wide_pool_nodes, blas_ranges, wide_ranges, inst): the top level.
  Record i is the record np_instanced_wide.widen_tlas writes for the current inst[i] (words 12..14 zero for a blas index outside
  [0, numBlas)).  The box of a slot whose link is ~i is np_instanced.instance_box with the object box being the union, in the f2i order,
  of slots 0..count-1 of wide pool node wide_ranges[blas].nodesOffset in place of the binary node 0's two boxes.  Inner slots, link 0,
  padding and topology are rules 4, 5, 6 and 1 above; the scene box is rule 7 (N == 1, root link ~0, no node: instance 0's box, and only
  record 0 is written).  err_bits and "a box is rewritten exactly where everything below it is well formed" are np_tlas_refit's rule 7:
  1 a blas index outside [0, numBlas) (the leaf ~i is bad; the record is written all the same, with its empty extent), 2 a link > 0
  that names no wide node (or a node named twice, or a count word outside 2..4), 4 a leaf link ~i with i >= N.  The scene box of a tree
  whose root is not well formed is six zeros.
"""
import numpy as np

import np_bvh_refit as rf
import np_bvh_wide as bw
import np_instanced as ni
import np_instanced_wide as niw

np_hlbvh = rf.np_hlbvh
F = np.float32
TERM = rf.TERM
ERR_LINK, ERR_ROW, ERR_TRI, ERR_VERTEX = 1, 2, 4, 8
TL_ERR_BLAS, TL_ERR_LINK, TL_ERR_LEAF = 1, 2, 4
WBOX = np.array(bw.WBOX)                   # [4, 6]: the words of slot k's box as lo.x hi.x lo.y hi.y lo.z hi.z
LO, HI = rf.LO, rf.HI


def _fold(boxes):
    """Union of boxes [m, 6] in the f2i order -> [6]."""
    i = np_hlbvh.f2i(boxes)
    out = np.empty(6, np.int32)
    out[LO], out[HI] = i[:, LO].min(axis=0), i[:, HI].max(axis=0)
    return np_hlbvh.i2f(out).astype(F)


def _min_max(box):
    return np.concatenate([box[LO], box[HI]]).astype(F)


def _walk(wi, link_bit):
    """Rule 9's tolerant walk over wide nodes wi [M, 32] -> (levels, followed [M, 4] bool, err).  A node with a bad count word is reached
    and has no slots; a link that names no node, or a node named before, is noted and not followed."""
    M = wi.shape[0]
    seen = np.zeros(M, bool)
    followed = np.zeros((M, 4), bool)
    err = 0
    levels = [[0]] if M else []
    if M:
        seen[0] = True
    while levels and levels[-1]:
        nxt = []
        for n in levels[-1]:
            c = int(wi[n, bw.WCOUNT])
            if not 2 <= c <= 4:
                err |= link_bit
                continue
            for k in range(c):
                link = int(wi[n, bw.WLINK + k])
                if link <= 0:
                    continue
                if link % bw.WIDE_BYTES or link // bw.WIDE_BYTES >= M or seen[link // bw.WIDE_BYTES]:
                    err |= link_bit
                    continue
                seen[link // bw.WIDE_BYTES] = True
                followed[n, k] = True
                nxt.append(link // bw.WIDE_BYTES)
        levels.append(nxt)
    return [lv for lv in levels if lv], followed, err


def _count(wi, n):
    c = int(wi[n, bw.WCOUNT])
    return c if 2 <= c <= 4 else 0


def _climb(wi, levels, followed, well):
    """Rules 4, 5, 6 bottom-up.  well [M, 4]: the leaf slots that were formed (or kept) without an error; -> node_well [M]."""
    wf = wi.view(F)
    node_well = np.zeros(wi.shape[0], bool)
    for level in reversed(levels):
        for n in level:
            c = _count(wi, n)
            for k in range(c):
                link = int(wi[n, bw.WLINK + k])
                if link == 0:
                    well[n, k] = True                                                   # rule 5
                elif link > 0 and followed[n, k]:
                    ch = link // bw.WIDE_BYTES
                    if node_well[ch]:
                        wf[n, WBOX[k]] = _fold(wf[ch][WBOX[:_count(wi, ch)]])           # rule 4
                        well[n, k] = True
            if c and well[n, :c].all():
                node_well[n] = True
                for k in range(c, 4):
                    wf[n, WBOX[k]] = wf[n, WBOX[0]]                                     # rule 6
    return node_well


def refit_wide_blas(wide_nodes, woop, tri_index, tri, pos, epsilon, rewrite_rows=True):
    """-> dict(nodes int32[M, 32], woop uint8[], root_box float32[6] min.xyz max.xyz, stats dict, err_bits)"""
    wi = np.ascontiguousarray(wide_nodes).reshape(-1).view(np.int32).reshape(-1, bw.WIDE_WORDS).copy()
    wf = wi.view(F)
    w = np.ascontiguousarray(woop).reshape(-1).view(np.uint32).reshape(-1, 4).copy()
    tidx = np.ascontiguousarray(tri_index).reshape(-1).view(np.int32)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    eps = F(epsilon)
    assert eps >= 0 and np.isfinite(eps)
    R, T, V = w.shape[0], tri.shape[0], pos.shape[0]

    levels, followed, err = _walk(wi, ERR_LINK)
    reached = [n for lv in levels for n in lv]
    well = np.zeros((wi.shape[0], 4), bool)
    leaves = [(n, k, int(wi[n, bw.WLINK + k])) for n in reached for k in range(_count(wi, n)) if wi[n, bw.WLINK + k] < 0]
    rows, of_leaf = [], []
    for leaf, (n, k, link) in enumerate(leaves):
        r, bad, mine = ~link, 0, []
        while True:
            if r >= R:
                bad |= ERR_ROW
                break
            if w[r, 0] == TERM:
                break
            if r + 2 >= R:
                bad |= ERR_ROW
            elif not 0 <= tidx[r] < T:
                bad |= ERR_TRI
            elif (tri[tidx[r]] < 0).any() or (tri[tidx[r]] >= V).any():
                bad |= ERR_VERTEX
            else:
                mine.append(r)
            r += 3
        err |= bad
        well[n, k] = not bad
        rows += mine
        of_leaf += [leaf] * len(mine)
    rows, of_leaf = np.array(rows, np.int64), np.array(of_leaf, np.int64)
    if rows.size:
        t = tidx[rows].astype(np.int64)
        if rewrite_rows:                                                                # rule 2
            r12 = np_hlbvh.woop_rows(np.ascontiguousarray(tri[t]), pos).view(np.uint32).reshape(-1, 3, 4)
            for j in range(3):
                w[rows + j] = r12[:, j]
        vi = np_hlbvh.f2i(pos[tri[t]]).astype(np.int64)                                 # rule 3: [m, 3 verts, 3 axes]
        L = len(leaves)
        lo_i = np.full((L, 3), np.iinfo(np.int64).max)
        hi_i = np.full((L, 3), np.iinfo(np.int64).min)
        np.minimum.at(lo_i, of_leaf, vi.min(axis=1))
        np.maximum.at(hi_i, of_leaf, vi.max(axis=1))
        for leaf in np.unique(of_leaf):
            n, k, _ = leaves[leaf]
            if not well[n, k]:
                continue
            with np.errstate(all="ignore"):
                wf[n, WBOX[k][LO]] = (np_hlbvh.i2f(lo_i[leaf]).astype(F) - eps).astype(F)
                wf[n, WBOX[k][HI]] = (np_hlbvh.i2f(hi_i[leaf]).astype(F) + eps).astype(F)
    node_well = _climb(wi, levels, followed, well)
    root = _min_max(_fold(wf[0][WBOX[:_count(wi, 0)]])) if wi.shape[0] and node_well[0] else np.zeros(6, F)   # rule 7
    stats = dict(numNodes=len(reached), numLeafLinks=len(leaves), numRows=int(rows.size * 3 + len(leaves)))
    return dict(nodes=wi, woop=w.reshape(-1).view(np.uint8).copy(), root_box=root, stats=stats, err_bits=err)


def refit_wide_pool(entries, wide_pool_nodes, pool_woop, pool_tri_index, tri, pos, rewrite_rows=True):
    """-> dict(nodes uint8, woop uint8, boxes float32[E, 6], stats (sums), err_bits (of all entries), first_bad_entry (-1: none),
    per_entry: refit_wide_blas's results)."""
    nodes = np.ascontiguousarray(wide_pool_nodes).reshape(-1).view(np.uint8).copy()
    woop = np.ascontiguousarray(pool_woop).reshape(-1).view(np.uint8).copy()
    tidx = np.ascontiguousarray(pool_tri_index).reshape(-1).view(np.int32)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    per_entry = []
    for no, nb, wo, wb, first, n, eps in entries:
        r = refit_wide_blas(nodes[no:no + nb], woop[wo:wo + wb], tidx[wo // 16:(wo + wb) // 16], tri[first:first + n], pos, eps, rewrite_rows)
        nodes[no:no + nb] = r["nodes"].reshape(-1).view(np.uint8)
        woop[wo:wo + wb] = r["woop"]
        per_entry.append(r)
    stats = {k: sum(r["stats"][k] for r in per_entry) for k in ("numNodes", "numLeafLinks", "numRows")}
    bad = [k for k, r in enumerate(per_entry) if r["err_bits"]]
    err = 0
    for r in per_entry:
        err |= r["err_bits"]
    return dict(nodes=nodes, woop=woop, boxes=np.stack([r["root_box"] for r in per_entry]).astype(F), stats=stats, err_bits=err,
                first_bad_entry=bad[0] if bad else -1, per_entry=per_entry)


def wide_root_box(wide_pool_nodes, wide_range):
    """The object box of a wide BLAS: the union of its node 0's slots 0..count-1 -> [6] as lo.x hi.x lo.y hi.y lo.z hi.z."""
    wi = np.ascontiguousarray(wide_pool_nodes).reshape(-1).view(np.uint8)[wide_range[0]:wide_range[0] + bw.WIDE_BYTES].view(np.int32)
    c = min(max(int(wi[bw.WCOUNT]), 1), 4)     # (a count word outside 2..4 is out of contract for the pool handed to the top level)
    return _fold(wi.view(F)[WBOX[:c]])


def wide_instance_box(wide_pool_nodes, wide_range, object_to_world):
    """np_instanced.instance_box over the wide root's box -> [6] as lo.x hi.x lo.y hi.y lo.z hi.z."""
    b = wide_root_box(wide_pool_nodes, wide_range)
    node0 = np.zeros(12, F)                    # a binary node 0 whose two children both hold the box
    for k in (0, 1):
        node0[rf.BOX_WORDS[k]] = b
    lo, hi = ni.instance_box(node0, (0, 64, 0, 0), object_to_world)
    out = np.empty(6, F)
    out[LO], out[HI] = lo, hi
    return out


def refit_wide_tlas(wide_tlas_nodes, root_link, wide_records, wide_pool_nodes, blas_ranges, wide_ranges, inst):
    """-> dict(nodes int32 (M, 32), records uint32 (N, 16), scene_box float32[6] min.xyz max.xyz, stats (numNodes, numLeaves), err_bits)"""
    n = inst.shape[0]
    num_blas = len(wide_ranges)
    wi = np.ascontiguousarray(wide_tlas_nodes).reshape(-1).view(np.int32).reshape(-1, bw.WIDE_WORDS).copy()
    wf = wi.view(F)
    rec = np.ascontiguousarray(wide_records).reshape(-1).view(np.uint32).reshape(-1, 16)[:n].copy()
    assert n >= 1 and rec.shape[0] == n and int(root_link) == (0 if n >= 2 else ~0)
    good = (inst["blas"] >= 0) & (inst["blas"] < num_blas)
    err = 0 if good.all() else TL_ERR_BLAS
    fresh = niw.widen_tlas(None, ~0, inst[:1] if n == 1 else inst, blas_ranges, wide_ranges)["records"]
    box_of = lambda i: wide_instance_box(wide_pool_nodes, wide_ranges[int(inst[i]["blas"])], inst[i]["objectToWorld"])
    if n == 1:
        rec[0] = fresh[0]
        scene = _min_max(box_of(0)) if good[0] else np.zeros(6, F)
        return dict(nodes=wi, records=rec, scene_box=scene, stats=dict(numNodes=0, numLeaves=1), err_bits=err)
    rec[:] = fresh
    levels, followed, e = _walk(wi, TL_ERR_LINK)
    err |= e
    reached = [m for lv in levels for m in lv]
    well = np.zeros((wi.shape[0], 4), bool)
    leaves = 0
    for m in reached:
        for k in range(_count(wi, m)):
            link = int(wi[m, bw.WLINK + k])
            if link >= 0:
                continue
            leaves += 1
            i = ~link
            if i >= n:
                err |= TL_ERR_LEAF
            elif good[i]:
                wf[m, WBOX[k]] = box_of(i)
                well[m, k] = True
    node_well = _climb(wi, levels, followed, well)
    scene = _min_max(_fold(wf[0][WBOX[:_count(wi, 0)]])) if wi.shape[0] and node_well[0] else np.zeros(6, F)
    return dict(nodes=wi, records=rec, scene_box=scene, stats=dict(numNodes=len(reached), numLeaves=leaves), err_bits=err)
