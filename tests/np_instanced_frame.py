"""numpy spec of ntr_instanced_hit_attributes: what a two-level hit needs before anything indexes by triangle.

EXTENSION: the reference has no instancing.  This docstring is the normative text; the device (csrc/instanced_attr_kernels.hip) equals
hit_attributes() in every word.  All arithmetic is binary32, every operation rounded once (no contraction), as np_instanced.xform does it.

Data.
  results     the records ntr_trace_instanced wrote: (id, t, padA, padB) -- id is the BLAS's own triangle id, relative to its mesh
  inst_ids    the instance of every ray's hit
  inst        np_instanced.INSTANCE_DTYPE
  blas_tris   (numBlas, 2) int32: BLAS k is triangles [firstTri, firstTri + numTris) of tri
  tri, pos    (numTrisTotal, 3) int32 vertex indices and (numVerts, 3) float32 positions, the CURRENT ones

Ray r is resolved iff
    id = results[r].id != -1,  i = inst_ids[r] in [0, numInstances),  b = inst[i].blas in [0, numBlas),
    id in [0, blas_tris[b].numTris),  g = blas_tris[b].firstTri + id in [0, numTrisTotal)  (the sum taken without wrap-around),
    and the three vertex indices (a, b, c) of triangle g in [0, numVerts).
out_results[r] is results[r] with id replaced by g when resolved and by -1 otherwise; t and the two pad words are copied verbatim.

Normal.  e1 = v[b] - v[a], e2 = v[c] - v[a];
    n_o = (e1.y * e2.z - e1.z * e2.y,  e1.z * e2.x - e1.x * e2.z,  e1.x * e2.y - e1.y * e2.x)       (Scene.cpp:112's cross product)
    with W = worldToObject of instance i, 3x4 row-major:  n_w.k = (W[0][k] * n_o.x + W[1][k] * n_o.y) + W[2][k] * n_o.z
    (the transpose of W's linear part, so the inverse transpose of objectToWorld)
    l2 = (n_w.x * n_w.x + n_w.y * n_w.y) + n_w.z * n_w.z
  A resolved ray whose l2 is finite and > 0 gets inv = 1 / sqrt(l2) and the normal (n_w.x * inv, n_w.y * inv, n_w.z * inv, 1);
  every other ray gets (0, 0, 0, 0).  The normal follows the object's winding: under a mirroring instance it is the world triangle's
  geometric normal negated.
"""
import numpy as np

F = np.float32


def hit_attributes(results, inst_ids, inst, blas_tris, tri, pos):
    """-> (out_results: a copy of results with the resolved ids, normals (n, 4) float32)"""
    results = np.asarray(results)
    n = results.shape[0]
    inst_ids = np.asarray(inst_ids, np.int32).astype(np.int64)
    blas_tris = np.asarray(blas_tris, np.int32).reshape(-1, 2).astype(np.int64)
    tri = np.asarray(tri, np.int32).reshape(-1, 3).astype(np.int64)
    pos = np.asarray(pos, F).reshape(-1, 3)
    num_inst, num_blas, num_tris, num_verts = inst.shape[0], blas_tris.shape[0], tri.shape[0], pos.shape[0]
    ids = results["id"].astype(np.int64)

    ok = (ids != -1) & (inst_ids >= 0) & (inst_ids < num_inst)
    i = np.where(ok, inst_ids, 0)
    b = inst["blas"].astype(np.int64)[i]
    ok &= (b >= 0) & (b < num_blas)
    b = np.where(ok, b, 0)
    ok &= (ids >= 0) & (ids < blas_tris[b, 1])
    g = blas_tris[b, 0] + ids
    ok &= (g >= 0) & (g < num_tris)
    g = np.where(ok, g, 0)
    v = tri[g]
    ok &= ((v >= 0) & (v < num_verts)).all(axis=1)
    v = np.where(ok[:, None], v, 0)

    out = results.copy()
    out["id"] = np.where(ok, g, -1).astype(np.int32)

    with np.errstate(all="ignore"):
        pa, pb, pc = pos[v[:, 0]], pos[v[:, 1]], pos[v[:, 2]]
        e1, e2 = (pb - pa).astype(F), (pc - pa).astype(F)

        def cross(p, q, r, s):
            return ((p * q).astype(F) - (r * s).astype(F)).astype(F)
        ox = cross(e1[:, 1], e2[:, 2], e1[:, 2], e2[:, 1])
        oy = cross(e1[:, 2], e2[:, 0], e1[:, 0], e2[:, 2])
        oz = cross(e1[:, 0], e2[:, 1], e1[:, 1], e2[:, 0])
        w = inst["worldToObject"].astype(F)[i].reshape(-1, 3, 4)
        nw = [(((w[:, 0, k] * ox).astype(F) + (w[:, 1, k] * oy).astype(F)).astype(F) + (w[:, 2, k] * oz).astype(F)).astype(F) for k in range(3)]
        l2 = (((nw[0] * nw[0]).astype(F) + (nw[1] * nw[1]).astype(F)).astype(F) + (nw[2] * nw[2]).astype(F)).astype(F)
        good = ok & np.isfinite(l2) & (l2 > 0)
        inv = (F(1.0) / np.sqrt(np.where(good, l2, F(1.0)).astype(F)).astype(F)).astype(F)
        normals = np.zeros((n, 4), F)
        for k in range(3):
            normals[:, k] = np.where(good, (nw[k] * inv).astype(F), F(0.0))
        normals[:, 3] = np.where(good, F(1.0), F(0.0))
    return out, normals
