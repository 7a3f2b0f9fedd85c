"""Instanced frames without a device: the numpy rule of ntr_instanced_hit_attributes (tests/np_instanced_frame.py) against binary64 over
the flattened world triangles, and the argument tables of ntr_instanced_hit_attributes and ntr_raygen_ao_normals.  The helpers here
(the pool's meshes as one index array and one vertex array, the traced scenes) are shared with tests/test_instanced_frame_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_frame as nf

F = np.float32
_cache = {}

# The largest 1 - |dot| of the spec's normal with the binary64 normal of the flattened world triangle over the hits of the three
# scenes below, as measured, and the bound the test allows: 4 times that (the float32 cross products of the soups' slivers cancel).
MEASURED_ONE_MINUS_DOT = 1.45e-7
BOUND = 4.0 * MEASURED_ONE_MINUS_DOT


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def geometry(names):
    """The meshes of the named BLASes as ntr_ploc_build_batch takes them: one index array (vertex indices into the shared vertex array),
    one vertex array, and (firstTri, numTris) per BLAS."""
    tris, poss, blas_tris, t0, v0 = [], [], [], 0, 0
    for name in names:
        tri, pos, _ = isc.blas(name)
        tris.append(tri.astype(np.int32) + v0)
        poss.append(pos.astype(F))
        blas_tris.append((t0, tri.shape[0]))
        t0 += tri.shape[0]
        v0 += pos.shape[0]
    return np.concatenate(tris).astype(np.int32), np.concatenate(poss).astype(F), np.array(blas_tris, np.int32)


def traced(name):
    """A named scene of instanced_scenes with its spec tree, rays and the spec's closest-hit and any-hit records."""
    if name not in _cache:
        sc = isc.scene(name)
        pool = isc.pool_of(sc["names"])
        inst = ni.instances(sc["transforms"], sc["blas"])
        t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
        rays = isc.scene_rays(primary=(64, 32), random=2048)
        tri, pos, blas_tris = geometry(sc["names"])
        hits = {}
        for any_hit in (False, True):
            rid, rt, ru, rv, rinst = ni.trace(t["nodes"], t["root_link"], t["records"], pool, rays, any_hit)
            res = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
            res["id"], res["t"], res["padA"], res["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
            hits[any_hit] = (res, rinst.astype(np.int32))
        _cache[name] = dict(sc=sc, pool=pool, inst=inst, tlas=t, rays=rays, tri=tri, pos=pos, blas_tris=blas_tris, hits=hits)
    return _cache[name]


def _one_minus_dot(name):
    """-> (1 - |dot| per hit, dot per hit, instance per hit) of the spec's normals of the scene's closest hits"""
    s = traced(name)
    res, rinst = s["hits"][False]
    out, normals = nf.hit_attributes(res, rinst, s["inst"], s["blas_tris"], s["tri"], s["pos"])
    # copied verbatim but for the id
    for k in ("t", "padA", "padB"):
        assert out[k].tobytes() == res[k].tobytes()
    hit = res["id"] >= 0
    assert np.array_equal(out["id"] >= 0, hit) and hit.sum() > res.shape[0] // 8
    assert (normals[~hit] == 0).all() and (normals[hit, 3] == 1).all()
    # the resolved ids name the (instance, triangle) isc.flatten lists
    verts, who = isc.flatten(s["sc"])
    counts = np.array([isc.blas(s["sc"]["names"][int(b)])[0].shape[0] for b in s["sc"]["blas"]])
    first_flat = np.concatenate([[0], np.cumsum(counts)[:-1]])
    i, lid = rinst[hit].astype(np.int64), res["id"][hit].astype(np.int64)
    flat = first_flat[i] + lid
    assert np.array_equal(who[flat], np.stack([i, lid], axis=1))
    assert np.array_equal(out["id"][hit] - s["blas_tris"][s["sc"]["blas"][i], 0], who[flat][:, 1])
    v = verts[flat]
    n64 = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    n32 = normals[hit, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n32, axis=1) - 1.0).max() < 1e-6
    dot = (n32 * n64).sum(axis=1)
    return 1.0 - np.abs(dot), dot, i


@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_spec_against_binary64(name):
    """The spec's normal against the binary64 normal of the flattened world triangle.  Measured over the closest hits of the three
    scenes (isc.scene_rays(primary=(64, 32), random=2048)): the largest 1 - |dot| is MEASURED_ONE_MINUS_DOT = 1.45e-7 (three 1.22e-7, grid
    1.45e-7, mirror 1.13e-7); the test allows BOUND = 5.8e-7, 4 times the largest, because float32 cross products of the soups' slivers cancel."""
    err, dot, i = _one_minus_dot(name)
    print("%s: %d hits, largest 1 - |dot| = %.3g (bound %.3g)" % (name, err.size, float(err.max()), BOUND))
    assert err.max() <= BOUND, (name, float(err.max()), BOUND)
    det = np.array([np.linalg.det(m.reshape(3, 4)[:, :3].astype(np.float64)) for m in traced(name)["sc"]["transforms"]])
    if name == "mirror":
        assert (det < 0).any()
    # the normal follows the object's winding: against the world triangle's normal exactly under a mirroring instance
    assert np.array_equal(dot < 0, det[i] < 0)


def test_spec_any_hit_records_resolve_like_closest_hit_records():
    s = traced("three")
    res, rinst = s["hits"][True]
    out, normals = nf.hit_attributes(res, rinst, s["inst"], s["blas_tris"], s["tri"], s["pos"])
    hit = res["id"] >= 0
    assert hit.any() and np.array_equal(out["id"] >= 0, hit) and np.array_equal(normals[:, 3] == 1, hit)
    assert np.array_equal(out["id"][hit], s["blas_tris"][s["inst"]["blas"][rinst[hit]], 0] + res["id"][hit])


def test_argument_errors_and_no_device():
    """Pointers are never dereferenced by a refused call; the accepted call runs only where there is no device to run it on."""
    fake = 0x10000
    L = nt.lib()
    geom = nt.InstancedGeometry(5, 3, 100, 300, fake, fake, fake, fake)
    good = dict(num_rays=64, d_results=fake, d_instance_ids=fake, geom=geom, d_out_results=fake, d_normals=fake)

    def g(**kw):
        return nt.InstancedGeometry(**dict(dict(num_instances=5, num_blas=3, num_tris_total=100, num_verts=300, d_instances=fake, d_blas_tris=fake,
                                                d_tri=fake, d_pos=fake), **kw))

    cases = [dict(geom=None), dict(d_out_results=0, d_normals=0), dict(d_normals=fake + 4), dict(d_normals=fake + 8), dict(d_out_results=fake + 4),
             dict(num_rays=-1), dict(d_results=0), dict(d_instance_ids=0)]
    cases += [dict(geom=g(**{k: 0})) for k in ("num_instances", "num_blas", "num_tris_total", "num_verts", "d_instances", "d_blas_tris", "d_tri",
                                               "d_pos")]
    cases += [dict(geom=g(num_instances=-1)), dict(geom=g(d_instances=fake + 8))]
    for change in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.instanced_hit_attributes(**dict(good, **change))
        assert e.value.code == -1 and "ntr_instanced_hit_attributes" in str(e.value), (change, str(e.value))
    # numRays == 0 is no work, with or without a device, whatever else is passed
    assert L.ntr_instanced_hit_attributes(0, None, None, None, None, None, None) == 0
    assert nt.instanced_hit_attributes(**dict(good, num_rays=0)) is None
    # the AO generator over per-ray normals: ntr_raygen_ao's table, and the alignment of the normals
    ao = dict(d_out_rays=fake, d_out_id_to_slot=fake, d_out_slot_to_id=fake, d_in_rays=fake, d_in_results=fake, d_ray_normals=fake,
              first_input_slot=0, num_input_rays=64, num_samples=4, max_dist=1.0)
    for change in (dict(num_input_rays=-1), dict(num_samples=-1), dict(first_input_slot=-1), dict(d_ray_normals=0), dict(d_out_rays=0),
                   dict(d_in_results=0), dict(d_ray_normals=fake + 4)):
        with pytest.raises(nt.NtrError) as e:
            nt.raygen_ao_normals(**dict(ao, **change))
        assert e.value.code == -1 and "ntr_raygen_ao_normals" in str(e.value), (change, str(e.value))
    assert nt.raygen_ao_normals(**dict(ao, num_input_rays=0, d_ray_normals=0)) is None
    assert nt.raygen_ao_normals(**dict(ao, num_samples=0)) is None
    if not _has_device():
        with pytest.raises(nt.NtrError) as e:
            nt.instanced_hit_attributes(**good)
        assert e.value.code in (-2, -3), str(e.value)


def test_struct_layouts():
    assert C.sizeof(nt.BlasTris) == 8 and nt.BLAS_TRIS_DTYPE.itemsize == 8
    assert C.sizeof(nt.InstancedGeometry) == 48 and nt.InstancedGeometry.d_instances.offset == 16
    assert nt.INSTANCE_DTYPE.itemsize == 112 and nt.INSTANCE_DTYPE.fields["worldToObject"][1] == 48
