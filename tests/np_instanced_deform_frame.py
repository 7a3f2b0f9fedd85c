"""numpy spec of motion-blurred frames over deforming BLASes: ntr_instanced_hit_attributes_deform.

EXTENSION: the reference has no instancing and no motion.  This docstring is the normative text; the device
(csrc/instanced_deform_attr_kernels.hip) equals hit_attributes_deform() in every word.  np_instanced_motion_frame.py states the
attributes of a hit on a moving instance, np_instanced_motion.py the clamp, np_bvh_motion.py the lerp of a deforming tree's words,
np_instanced_frame.py the cross product.  They are imported, not restated.

hit_attributes_deform(results, inst_ids, inst, blas_tris, tri, pos0, pos1, deforming, motion_keys, times=None, time=0.0).
  np_instanced_motion_frame.hit_attributes_motion in every respect -- the resolution rule, the id rewrite, the moving test from the key
  entry, W at the ray's time for a moving instance, the transpose, the normalisation, the (0, 0, 0, 0) cases -- except where the three
  vertices come from for a resolved ray r of instance i with b = inst[i].blas (the resolution has range checked b):
    time        t_r = times[r] when per-ray times are given, else the scalar time; clamped by np_instanced_motion.clamp_time: the time
                np_instanced_deform.trace posed that ray's triangle with
    static      deforming[b] == 0: the vertices are pos0[v]; nothing of pos1 is read
    deforming   deforming[b] != 0: each of the nine words is np_bvh_motion.deform_lerp(pos0[v], pos1[v], t_r) -- the keys themselves at
                t_r == 0 and t_r == 1, (1 - t_r) * a + t_r * b with both products rounded in between.  The vertex rows
                np_bvh_motion.motion_refit writes are the vertices' words verbatim, so this is, bit for bit, the triangle the ray was
                tested against
  The cross product is np_instanced_frame's, in its rounding order, over the posed words.  A posed triangle whose cross product has
  length 0 or a non-finite length resolves the id and gives the zero normal, as any such triangle does.  pos0 and pos1 both hold
  numVerts vertices; the index checks are np_instanced_frame's.  With no flag set, and at t_r == 0, the result is
  hit_attributes_motion over pos0; at t_r == 1 it is hit_attributes_motion over pos1.
"""
import numpy as np

import np_bvh_motion as bm
import np_instanced_motion as mo
import np_instanced_motion_frame as mf

F = np.float32


def hit_attributes_deform(results, inst_ids, inst, blas_tris, tri, pos0, pos1, deforming, motion_keys, times=None, time=0.0):
    """-> (out_results, normals (n, 4) float32), as np_instanced_frame.hit_attributes"""
    results = np.asarray(results)
    n = results.shape[0]
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    pos0 = np.asarray(pos0, F).reshape(-1, 3)
    pos1 = np.asarray(pos1).reshape(-1, 3)
    blas_tris = np.asarray(blas_tris, np.int32).reshape(-1, 2)
    deforming = np.asarray(deforming, np.uint32).reshape(-1)
    assert pos1.shape == pos0.shape and deforming.shape[0] == blas_tris.shape[0]
    times = None if times is None else np.ascontiguousarray(times).view(F).reshape(-1)[:n]
    # the resolution, the ids and every static BLAS's normal: the motion rule over key 0's vertices
    out, normals = mf.hit_attributes_motion(results, inst_ids, inst, blas_tris, tri, pos0, motion_keys, times=times, time=time)
    resolved = out["id"] >= 0
    i = np.where(resolved, np.asarray(inst_ids, np.int32), 0)
    sel = np.flatnonzero(resolved & (deforming[np.where(resolved, inst["blas"][i], 0)] != 0))
    if sel.size == 0:
        return out, normals
    # every deforming hit gets a mesh of its own: its triangle posed at t_r, as triangle k of one BLAS over 3 * m vertices; the motion
    # rule over that mesh takes W from the ray's instance as before
    t = mo.clamp_time(np.full(n, time, F) if times is None else times)[sel]
    v = tri[out["id"][sel]]
    posed = bm.deform_lerp(pos0[v], pos1[v].astype(F), t[:, None, None]).reshape(-1, 3)
    m = sel.size
    one = results[sel].copy()
    one["id"] = np.arange(m)
    inst_one = inst.copy()
    inst_one["blas"] = 0
    _, nrm = mf.hit_attributes_motion(one, np.asarray(inst_ids, np.int32)[sel], inst_one, np.array([(0, m)], np.int32),
                                      np.arange(3 * m, dtype=np.int32).reshape(m, 3), posed, motion_keys, times=None if times is None else times[sel],
                                      time=time)
    normals = normals.copy()
    normals[sel] = nrm
    return out, normals
