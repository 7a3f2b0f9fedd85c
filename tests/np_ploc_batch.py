"""numpy spec of ntr_ploc_build_batch: many PLOC builds into one pool.

EXTENSION: the reference has neither PLOC nor instancing.  The rule is three lines: every mesh of the batch -- triangles
[firstTri, +numTris) of one shared index array, over its own box -- is built by np_bvh_ploc.build on its own (triangle ids relative to
firstTri); the results are laid out by np_instanced.make_pool in mesh order without gaps; the per-mesh counts are that build's stats.
Meshes may name overlapping or identical triangle ranges and need not cover the array.
"""
import numpy as np

import np_bvh_ploc as pl
import np_instanced as ni

F = np.float32
MAX_MESHES = 1 << 20
POOL_MAX_BYTES = 0xFFFFFF00


def capacity(num_tris):
    """-> (nodesBytes, triWoopBytes, triIndexBytes, ranges) of a batch whose meshes have num_tris triangles: max(n - 1, 1) nodes and 4 n
    rows (5 for n == 1) each, packed in mesh order."""
    n = np.asarray(num_tris, np.int64)
    assert n.ndim == 1 and n.size >= 1 and (n >= 1).all()
    nodes, rows = 64 * np.maximum(n - 1, 1), 16 * np.where(n == 1, 5, 4 * n)
    n_off, w_off = np.cumsum(nodes) - nodes, np.cumsum(rows) - rows
    ranges = [tuple(int(x) for x in r) for r in zip(n_off, nodes, w_off, rows)]
    return int(nodes.sum()), int(rows.sum()), int(rows.sum()) // 4, ranges


def build(meshes, tri, pos, radius=8):
    """meshes: a list of (firstTri, numTris, sceneMin, sceneMax).  -> dict(nodes uint8, woop uint8, tri_index int32, ranges, stats: a list
    of np_bvh_ploc stats, builds: the per-mesh np_bvh_ploc.build results)."""
    tri = np.ascontiguousarray(tri, np.int32)
    builds = [pl.build(tri[f:f + n], pos, mn, mx, radius) for f, n, mn, mx in meshes]
    pool = ni.make_pool([(b["nodes"], b["woop"], b["tri_index"]) for b in builds])
    return dict(pool, stats=[b["stats"] for b in builds], builds=builds)


def concat(parts):
    """parts: a list of (tri, pos) meshes.  -> (tri, pos, meshes): one shared index array and vertex array, and every part as a mesh over
    its own bounding box."""
    tris, poss, meshes = [], [], []
    t_off = v_off = 0
    for tri, pos in parts:
        tri, pos = np.asarray(tri, np.int32), np.asarray(pos, F)
        tris.append(tri + v_off)
        poss.append(pos)
        mn, mx = pl.scene_box(pos)
        meshes.append((t_off, tri.shape[0], mn, mx))
        t_off += tri.shape[0]
        v_off += pos.shape[0]
    return np.concatenate(tris).astype(np.int32), np.concatenate(poss).astype(F), meshes
