"""numpy spec of motion-blurred instanced frames: ntr_ray_times_primary, ntr_ray_times_secondary, ntr_instanced_hit_attributes_motion.

EXTENSION: the reference has no instancing and no motion.  This docstring is the normative text; the device
(csrc/ray_times_kernels.hip, csrc/instanced_motion_attr_kernels.hip) equals ray_times_primary() and ray_times_secondary() bit for bit
and hit_attributes_motion() in every word.  np_instanced_motion.py states the keys, the clamp, the lerp and the inverse;
np_instanced_frame.py the attributes of a hit.  They are imported, not restated.

ray_times_primary(n, slot_to_id, seed, open, close).  One time per PIXEL in the shutter [open, close], 0 <= open <= close <= 1.  All
  integer arithmetic is mod 2^32, all floating-point arithmetic binary32 with every operation rounded once (no contraction).  For slot s:
    id   = slot_to_id[s], or s without a table
    x    = (uint32)id + (seed + 1) * 0x9E3779B9
    x   ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
    u    = (float)(x >> 8) * 2^-24                 exact: 24 bits, in [0, 1 - 2^-24]
    span = close - open                            rounded once
    t    = open + u * span                         the product rounded, then the sum
    time = t < close ? t : close
  With open = 0 and close = 1 the time is u bit for bit.  The time depends on the pixel id and not on the slot: a permutation of the
  slots with the table permuted alike permutes the times alike.  Another seed gives another sample.

ray_times_secondary(in_times, first, count, num_samples).  out[k * num_samples + j] = in_times[first + k] for k < count,
  j < num_samples, the WORD copied verbatim (a NaN with its payload, a signed zero): ntr_raygen_ao_normals' slot rule -- output slot
  k * num_samples + j belongs to input slot first + k -- so a secondary ray sees its instance where its primary ray saw it.

hit_attributes_motion(results, inst_ids, inst, blas_tris, tri, pos, motion_keys, times=None, time=0.0).
  np_instanced_frame.hit_attributes in every respect -- the resolution rule, the id rewrite, the cross product, the transpose, the
  normalisation, the (0, 0, 0, 0) cases -- except where W comes from for a resolved ray r of instance i:
    time      t_r = times[r] when per-ray times are given, else the scalar time; clamped by np_instanced_motion.clamp_time
    moving    instance i is moving iff words 0..11 and 16..27 of its 32-word entry of motion_keys differ bitwise
              (np_instanced_motion.moving over a buffer np_instanced_motion.motion_refit wrote; there are no records here, so word 15
              cannot be read)
    static    W = inst[i].worldToObject, as np_instanced_frame
    moving    W = np_instanced_motion.invert_many(np_instanced_motion.lerp(key 0, key 1, t_r)): the matrix the motion trace
              transformed that ray with.  No inverse (a zero or non-finite determinant): the id is still resolved, the normal is
              (0, 0, 0, 0)
  The blas index is inst[i].blas (key 0's); pos is the current mesh.
"""
import numpy as np

import np_instanced_frame as nf
import np_instanced_motion as mo

F = np.float32
U = np.uint32


def hash_u32(ids, seed):
    """The hash x of the pixel ids (any integers, taken mod 2^32) under `seed`: uint32."""
    M = np.uint64(0xFFFFFFFF)
    x = (np.asarray(ids).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    x = (x + np.uint64((((int(seed) & 0xFFFFFFFF) + 1) * 0x9E3779B9) & 0xFFFFFFFF)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x.astype(U)


def ray_times_primary(n, slot_to_id=None, seed=0, open=0.0, close=1.0):
    """-> float32 (n,)"""
    ids = np.arange(n, dtype=np.int64) if slot_to_id is None else np.asarray(slot_to_id).reshape(-1)[:n]
    u = ((hash_u32(ids, seed) >> U(8)).astype(F) * F(2.0 ** -24)).astype(F)
    open, close = F(open), F(close)
    span = F(close - open)
    t = (open + (u * span).astype(F)).astype(F)
    return np.where(t < close, t, close).astype(F)


def ray_times_secondary(in_times, first, count, num_samples):
    """-> float32 (count * num_samples,), the words of in_times[first : first + count] repeated"""
    w = np.ascontiguousarray(in_times).view(U).reshape(-1)[first:first + count]
    assert w.shape[0] == count
    return np.repeat(w, num_samples).view(F)


def hit_attributes_motion(results, inst_ids, inst, blas_tris, tri, pos, motion_keys, times=None, time=0.0):
    """-> (out_results, normals (n, 4) float32), as np_instanced_frame.hit_attributes"""
    n = np.asarray(results).shape[0]
    num_inst = inst.shape[0]
    keys = np.ascontiguousarray(motion_keys).view(np.uint8).reshape(-1)
    keys = keys[:num_inst * mo.KEY_BYTES].view(U).reshape(num_inst, mo.KEY_WORDS)
    k0, k1 = keys[:, 0:12], keys[:, 16:28]
    moving = (k0 != k1).any(axis=1)
    t = mo.clamp_time(np.full(n, time, F) if times is None else np.ascontiguousarray(times).view(F).reshape(-1)[:n])
    # every ray gets an instance array of its own: row r is the instance of ray r posed at t_r (rays without one take row 0 of `inst`,
    # which the resolution refuses as before)
    ids = np.asarray(inst_ids, np.int32).astype(np.int64)
    there = (ids >= 0) & (ids < num_inst)
    i = np.where(there, ids, 0)
    per_ray = inst[i].copy()
    mv = there & moving[i]
    singular = np.zeros(n, bool)
    if mv.any():
        w2o, ok = mo.invert_many(mo.lerp(k0[i[mv]].view(F), k1[i[mv]].view(F), t[mv]))
        per_ray["worldToObject"][mv] = w2o.reshape((-1,) + per_ray["worldToObject"].shape[1:])   # (zero where there is no inverse)
        singular[np.flatnonzero(mv)[~ok]] = True
    out, normals = nf.hit_attributes(results, np.where(there, np.arange(n), -1).astype(np.int32), per_ray, blas_tris, tri, pos)
    assert (normals[singular] == 0).all()   # a zero W gives l2 == 0 (or a NaN): the zero normal
    return out, normals
