"""numpy spec of ntr_bvh_refit_batch: many refits inside one pool.

EXTENSION: the reference has neither a refit nor instancing.  The rule is three lines: for every entry -- a BLAS's range
(nodesOffset, nodesBytes, triWoopOffset, triWoopBytes), its mesh [firstTri, +numTris) of the shared index array and its epsilon --
np_bvh_refit.refit runs over that entry's slices of the pool (nodes, triWoop, and triIndex from entry triWoopOffset / 16) with the mesh
tri[firstTri : firstTri + numTris], the shared positions and the entry's epsilon; the results are written back into those slices; the
boxes are the refits' scene boxes in entry order and the counts their sums.  Every byte outside the entries' ranges stays.
"""
import numpy as np

import np_bvh_refit as rf

F = np.float32
MAX_ENTRIES = 1 << 20


def refit(entries, nodes, woop, tri_index, tri, pos):
    """entries: a list of ((nodesOffset, nodesBytes, triWoopOffset, triWoopBytes), firstTri, numTris, epsilon); nodes, woop: the pool's
    bytes; tri_index: its int32 entries.  -> dict(nodes uint8, woop uint8, boxes float32[E, 6], stats: the sums of np_bvh_refit's,
    per_entry: its results)."""
    nodes = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8).copy()
    woop = np.ascontiguousarray(woop).reshape(-1).view(np.uint8).copy()
    tri_index = np.ascontiguousarray(tri_index).reshape(-1).view(np.int32)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    per_entry = []
    for (no, nb, wo, wb), first, n, eps in entries:
        r = rf.refit(nodes[no:no + nb], woop[wo:wo + wb], tri_index[wo // 16:(wo + wb) // 16], tri[first:first + n], pos, eps)
        nodes[no:no + nb] = r["nodes"].reshape(-1).view(np.uint8)
        woop[wo:wo + wb] = r["woop"]
        per_entry.append(r)
    stats = {k: sum(r["stats"][k] for r in per_entry) for k in ("numNodes", "numLeaves", "numRows")}
    return dict(nodes=nodes, woop=woop, boxes=np.stack([r["scene_box"] for r in per_entry]).astype(F), stats=stats, per_entry=per_entry)
