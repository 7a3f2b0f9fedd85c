"""numpy spec of ntr_bvh_motion_refit_batch: many two-key refits inside one pool.

EXTENSION: the reference has neither a refit nor instancing.  The rule: for every entry -- a BLAS's range (nodesOffset, nodesBytes,
triWoopOffset, triWoopBytes), its mesh [firstTri, +numTris) of the shared index array and its epsilon -- np_bvh_motion.motion_refit runs
over that entry's slices of the pool (nodes0, triWoop, and triIndex from entry triWoopOffset / 16) with the mesh
tri[firstTri : firstTri + numTris], the two shared position arrays and the entry's epsilon; its five results are written back into
those slices of nodes0, nodes1, triWoop, vertRows0 and vertRows1; the boxes are the refits' scene boxes (the union of the two keys'
roots) in entry order and the counts their sums.  Every byte outside the entries' ranges stays: the three key-1 buffers come in as the
caller's bytes, whatever they are.
"""
import numpy as np

import np_bvh_motion as bm

F = np.float32
MAX_ENTRIES = 1 << 20
BUFFERS = ("nodes0", "nodes1", "woop", "vrows0", "vrows1")


def motion_refit(entries, nodes0, nodes1, woop, vrows0, vrows1, tri_index, tri, pos0, pos1):
    """entries: a list of ((nodesOffset, nodesBytes, triWoopOffset, triWoopBytes), firstTri, numTris, epsilon); the five pool buffers as
    bytes; tri_index: the pool's int32 entries.  -> dict(nodes0, nodes1, woop, vrows0, vrows1 uint8; boxes float32 [E, 6]; stats: the
    sums of np_bvh_motion.motion_refit's; per_entry: its results)."""
    out = {k: np.ascontiguousarray(b).reshape(-1).view(np.uint8).copy() for k, b in zip(BUFFERS, (nodes0, nodes1, woop, vrows0, vrows1))}
    tri_index = np.ascontiguousarray(tri_index).reshape(-1).view(np.int32)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    per_entry = []
    for (no, nb, wo, wb), first, n, eps in entries:
        m = bm.motion_refit(out["nodes0"][no:no + nb], out["woop"][wo:wo + wb], tri_index[wo // 16:(wo + wb) // 16], tri[first:first + n],
                            pos0, pos1, eps)
        for k in BUFFERS:
            o, b = (no, nb) if k.startswith("nodes") else (wo, wb)
            out[k][o:o + b] = np.ascontiguousarray(m[k]).reshape(-1).view(np.uint8)
        per_entry.append(m)
    stats = {k: sum(m["stats"][k] for m in per_entry) for k in ("numNodes", "numLeaves", "numRows")}
    return dict(out, boxes=np.stack([m["scene_box"] for m in per_entry]).astype(F), stats=stats, per_entry=per_entry)
