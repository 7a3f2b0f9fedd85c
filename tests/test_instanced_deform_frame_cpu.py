"""Motion-blurred frames over deforming BLASes without a device: the numpy rule (tests/np_instanced_deform_frame.py) against the older
specs it is written over (np_instanced_motion_frame.hit_attributes_motion at the shutter's two ends and with no flag set,
np_instanced_frame.hit_attributes over the scene posed at an interior time), against binary64 over the triangle posed at the ray's
time, over a BLAS that collapses to a point, on the self-occlusion demonstration, and the argument table of
ntr_instanced_hit_attributes_deform on fake pointers."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_deform_cases as dc
import instanced_deform_frame_cases as dfc
import np_bvh_motion as bm
import np_instanced_frame as nf
import np_instanced_motion as mo
import np_instanced_motion_frame as mf
from np_instanced_deform_frame import hit_attributes_deform

F = np.float32
U = np.uint32

# The largest 1 - |dot| of the spec's normal with the binary64 normal of the world-space triangle posed at the ray's time (vertices by the
# rule's binary32 deform_lerp, M(t_r) by the rule's binary32 lerp, then everything in binary64) over the hits of three, mirror and grid,
# as measured on the CPU against binary64 (never against the device), and the bound the test allows: 4 times that, the convention of
# test_instanced_motion_frame_cpu.py (the float32 cross products of the soups' slivers cancel).
MEASURED_ONE_MINUS_DOT = 1.42e-7
BOUND = 4.0 * MEASURED_ONE_MINUS_DOT


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _words(out, normals):
    return out.tobytes(), normals.view(U).tobytes()


def _attr(s, pos1=None, deforming=None, **kw):
    return hit_attributes_deform(s["res"], s["ids"], s["s"].inst0, s["blas_tris"], s["tri"], s["pos0"], s["pos1"] if pos1 is None else pos1,
                                 s["deforming"] if deforming is None else deforming, s["keys"], **kw)


def _motion(s, pos, **kw):
    return mf.hit_attributes_motion(s["res"], s["ids"], s["s"].inst0, s["blas_tris"], s["tri"], pos, s["keys"], **kw)


# ---- 1. ties to the older specs ---------------------------------------------------------------------------------------------------------------
def test_no_flag_set_is_the_motion_rule_over_key_0():
    for name, flags in (("three_static", None), ("three", np.zeros(3, U))):
        s = dfc.traced(name)
        assert (s["res"]["id"] >= 0).sum() > s["res"].shape[0] // 8
        poison = np.full_like(s["pos1"], np.nan)
        for kw in (dict(times=s["times"]), dict(time=0.5), dict(time=1.0)):
            assert _words(*_attr(s, pos1=poison, deforming=flags, **kw)) == _words(*_motion(s, s["pos0"], **kw)), (name, kw)
    assert not dfc.traced("three_static")["deforming"].any() and dfc.traced("three")["deforming"].tolist() == [0, 1, 0]


@pytest.mark.parametrize("name", dc.SCENES)
def test_ties_to_the_older_specs(name):
    """The records are the deform trace's at the hashed times; the attributes are a function of the records, the ids and the time alone,
    so one set of records serves every time."""
    s = dfc.traced(name)
    sc = s["s"]
    hit = s["res"]["id"] >= 0
    on_deforming = hit & (s["deforming"][sc.inst0["blas"][np.where(hit, s["ids"], 0)]] != 0)
    assert hit.sum() > hit.size // 8 and on_deforming.any()
    n = hit.size
    # the two ends are the keys: the motion rule over key 0's vertices and over key 1's
    at0, at1 = _words(*_motion(s, s["pos0"], time=0.0)), _words(*_motion(s, s["pos1"], time=1.0))
    assert _words(*_attr(s, time=0.0)) == at0 and _words(*_attr(s, times=np.zeros(n, F))) == at0
    assert _words(*_attr(s, time=1.0)) == at1 and _words(*_attr(s, times=np.ones(n, F))) == at1
    assert at0[0] == at1[0] and at0[1] != at1[1]
    # in between: the static scene that this one IS at tau, instances and meshes posed
    at = {}
    for tau in dfc.INTERIOR:
        _, inst, meshes = dc.posed_scene(sc, tau)
        pos = np.concatenate([m[1] for m in meshes]).astype(F)
        at[tau] = _words(*_attr(s, time=tau))
        assert at[tau] == _words(*nf.hit_attributes(s["res"], s["ids"], inst, s["blas_tris"], s["tri"], pos)), tau
    assert len(set(at.values())) == len(dfc.INTERIOR)
    # per-ray times: each ray takes its own pose
    pick = np.resize(np.array(dfc.INTERIOR, F), n)
    out, nrm = _attr(s, times=pick)
    for tau in dfc.INTERIOR:
        sel = pick == F(tau)
        assert nrm[sel].view(U).tobytes() == np.frombuffer(at[tau][1], U).reshape(-1, 4)[sel].tobytes()
    assert out.tobytes() == at0[0]
    # the corner times go through the clamp
    clamped = mo.clamp_time(dc.CORNER_TIMES)
    assert clamped.view(U).tolist() == [0, 0x3F800000, 0, 1, 0x3F7FFFFF]
    assert _words(*_attr(s, time=-1.0)) == at0 and _words(*_attr(s, time=2.0)) == at1 and _words(*_attr(s, time=float("nan"))) == at0
    nrm = _attr(s, times=np.resize(dc.CORNER_TIMES, n))[1]
    for j, k in enumerate(clamped):
        sel = np.arange(n) % clamped.size == j
        assert nrm[sel].view(U).tobytes() == _attr(s, time=float(k))[1][sel].view(U).tobytes(), j


@pytest.mark.parametrize("name", ["three", "collapse", "big"])
def test_key_1_of_a_static_blas_is_never_read(name):
    s = dfc.traced(name)
    tri, pos0, poisoned, _ = dfc.geometry_of(s["s"], poison=True)
    assert np.isnan(poisoned).any() and pos0.tobytes() == s["pos0"].tobytes()
    for kw in (dict(times=s["times"]), dict(time=1.0)):
        assert _words(*_attr(s, pos1=poisoned, **kw)) == _words(*_attr(s, **kw)), (name, kw)


# ---- 2. against binary64 ----------------------------------------------------------------------------------------------------------------------
def _one_minus_dot(name):
    s = dfc.traced(name)
    sc, res, ids = s["s"], s["res"], s["ids"]
    out, normals = _attr(s, times=s["times"])
    hit = res["id"] >= 0
    assert np.array_equal(out["id"] >= 0, hit) and (normals[~hit] == 0).all() and (normals[hit, 3] == 1).all()
    i, lid = ids[hit].astype(np.int64), res["id"][hit].astype(np.int64)
    b = sc.inst0["blas"][i]
    g = s["blas_tris"][b, 0] + lid
    assert np.array_equal(out["id"][hit], g)
    # the triangle posed at t_r under M(t_r): the rule's binary32 lerps of the two pairs of keys, then everything in binary64
    t = mo.clamp_time(s["times"])[hit]
    m = mo.lerp(sc.inst0["objectToWorld"].reshape(-1, 12)[i], sc.inst1["objectToWorld"].reshape(-1, 12)[i], t).astype(np.float64).reshape(-1, 3, 4)
    v = s["tri"][g]
    deforming = s["deforming"][b] != 0
    p = np.where(deforming[:, None, None], bm.deform_lerp(s["pos0"][v], s["pos1"][v], t[:, None, None]), s["pos0"][v]).astype(np.float64)
    w = np.einsum("nij,nkj->nki", m[:, :, :3], p) + m[:, None, :, 3]
    n64 = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    n32 = normals[hit, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n32, axis=1) - 1.0).max() < 1e-6
    dot = (n32 * n64).sum(axis=1)
    return 1.0 - np.abs(dot), dot, np.linalg.det(m[:, :, :3]), deforming


@pytest.mark.parametrize("name", dc.SCENES)
def test_spec_against_binary64_at_the_rays_time(name):
    """The spec's normal at the ray's hashed time against the binary64 normal of the hit triangle posed at t_r under M(t_r), over the
    closest hits of the three scenes (instanced_deform_cases.rays_of("cpu"), bvh_motion_cases.hashed_times) with
    test_instanced_motion_frame_cpu.py's exclusions and no others: the hits alone.  Measured: the largest 1 - |dot| is
    MEASURED_ONE_MINUS_DOT = 1.42e-7 (three 1.28e-7, mirror 1.42e-7, grid 1.17e-7); the test allows BOUND = 5.68e-7, 4 times the largest."""
    err, dot, det, deforming = _one_minus_dot(name)
    print("%s: %d hits (%d on deforming BLASes), largest 1 - |dot| = %.3g (bound %.3g)" % (name, err.size, int(deforming.sum()), float(err.max()), BOUND))
    assert deforming.any() and err.max() <= BOUND, (name, float(err.max()), BOUND)
    if name == "mirror":
        assert (det < 0).any()
    # the normal follows the object's winding: against the posed triangle's normal exactly where M(t) mirrors
    assert (det != 0).all() and np.array_equal(dot < 0, det < 0)


# ---- 3. a BLAS that collapses to a point ------------------------------------------------------------------------------------------------------
def test_a_collapsed_triangle_resolves_the_id_and_gives_no_normal():
    s = dfc.traced("collapse")
    sc = s["s"]
    assert s["deforming"].tolist() == [0, 0, 1]
    hit = s["res"]["id"] >= 0
    on2 = hit & (sc.inst0["blas"][np.where(hit, s["ids"], 0)] == 2)
    assert on2.sum() > 16 and (hit & ~on2).sum() > 16
    out, nrm = _attr(s, time=1.0)
    assert (out["id"][on2] >= 0).all() and (nrm[on2].view(U) == 0).all()              # resolved, and no normal
    assert (nrm[hit & ~on2, 3] == 1).all()                                            # the static BLASes beside it are untouched
    out, nrm = _attr(s, time=0.5)
    assert (nrm[hit, 3] == 1).all()
    # per-ray times: only the rays at exactly 1 lose their normal
    t = np.where(np.arange(hit.size) % 2 == 0, F(1.0), F(0.5)).astype(F)
    out, nrm = _attr(s, times=t)
    assert np.array_equal(nrm[on2, 3] == 0, (t == F(1.0))[on2]) and (out["id"][on2] >= 0).all()


# ---- 4. the demonstration: a convex cube that deforms inside the shutter ----------------------------------------------------------------------
def test_a_secondary_ray_must_start_from_the_triangle_its_primary_ray_hit():
    """instanced_deform_frame_cases.demo(): 64 x 32 primary rays with one hashed time per pixel, 8 AO rays of radius 3 per hit.  The
    deforming cube stays convex, so no AO ray may hit the instance it started from.  Measured on the spec alone: 240 primary hits (120 on
    the deforming cube), 1920 live AO rays; self hits 0 (52 AO rays occluded in all) with the normals of the posed triangle and the primary
    ray's time inherited, 275 (of 314) with key-0 normals, 717 (of 902) with the secondary times all 0."""
    d = dfc.demo()
    s, rays = d["s"], d["rays"]
    n = rays.shape[0]
    times = mf.ray_times_primary(n, d["s2i"], 0)
    rid, rt, ru, rv, rinst, _ = s.trace(rays, False, times=times)
    res, ids = dfc.records(rid, rt, ru, rv), rinst.astype(np.int32)
    assert ((rid >= 0) & (ids == 0)).sum() > 64 and ((rid >= 0) & (ids == 1)).sum() > 64
    keys = s.refit["motion_keys"]
    assert not mo.moving(s.inst0, s.inst1).any()          # only the deformation moves anything
    src = np.repeat(ids, dfc.DEMO_NS)

    def self_hits(attributes, sec_times):
        srays = dfc.ao_batch(rays, *attributes)
        assert (srays["tmax"] > 0).sum() == dfc.DEMO_NS * (rid >= 0).sum()
        sid, _, _, _, sinst, _ = s.trace(srays, True, times=sec_times)
        return int(((sid >= 0) & (sinst == src) & (src == 0)).sum()), int((sid >= 0).sum())
    at_time = hit_attributes_deform(res, ids, s.inst0, d["blas_tris"], d["tri"], d["pos0"], d["pos1"], d["deforming"], keys, times=times)
    at_key0 = mf.hit_attributes_motion(res, ids, s.inst0, d["blas_tris"], d["tri"], d["pos0"], keys, times=times)
    inherited = mf.ray_times_secondary(times, 0, n, dfc.DEMO_NS)
    rows = (self_hits(at_time, inherited), self_hits(at_key0, inherited), self_hits(at_time, np.zeros(n * dfc.DEMO_NS, F)))
    print("self hits (occluded): %d (%d) posed with inherited times, %d (%d) with key-0 normals, %d (%d) with secondary times 0"
          % tuple(x for r in rows for x in r))
    assert rows[0][0] == 0 and rows[0][1] > 0 and rows[1][0] > 0 and rows[2][0] > 0, rows


# ---- 5. refusals, before any device work --------------------------------------------------------------------------------------------------------
FAKE = 0x10000
NAME = "ntr_instanced_hit_attributes_deform"


def _geom(**kw):
    return nt.InstancedGeometry(**dict(dict(num_instances=5, num_blas=3, num_tris_total=100, num_verts=300, d_instances=FAKE, d_blas_tris=FAKE,
                                            d_tri=FAKE, d_pos=FAKE), **kw))


def test_argument_errors_and_no_device():
    """The shared refusals come in ntr_instanced_hit_attributes_motion's words and order under the new name: every case is put to both
    entry points, and the two messages differ in the name alone; the new call's own refusals come after them."""
    g = _geom
    motion = nt.InstanceMotion(FAKE, 128 * 5, FAKE, 0.5)
    deform = nt.InstancedDeformGeometry(FAKE, FAKE)
    bad_deform = nt.InstancedDeformGeometry(0, FAKE + 2)
    good = dict(num_rays=64, d_results=FAKE, d_instance_ids=FAKE, geom=g(), d_out_results=FAKE, d_normals=FAKE)
    shared = [dict(geom=None), dict(d_out_results=0, d_normals=0), dict(d_normals=FAKE + 4), dict(d_normals=FAKE + 8), dict(d_out_results=FAKE + 4),
              dict(num_rays=-1), dict(d_results=0), dict(d_instance_ids=0), dict(d_results=FAKE + 8)]
    shared += [dict(geom=g(**{k: 0})) for k in ("num_instances", "num_blas", "num_tris_total", "num_verts", "d_instances", "d_blas_tris", "d_tri",
                                                "d_pos")]
    shared += [dict(geom=g(num_instances=-1)), dict(geom=g(d_instances=FAKE + 8)), dict(geom=g(d_blas_tris=FAKE + 4))]
    # order: a call wrong in several ways names the first
    shared += [dict(num_rays=-1, geom=None), dict(geom=g(d_pos=0, num_blas=0)), dict(geom=g(num_verts=0), d_results=0),
               dict(d_instance_ids=0, d_out_results=0, d_normals=0), dict(d_out_results=0, d_normals=0, geom=g(d_instances=FAKE + 8)),
               dict(d_normals=FAKE + 4, geom=g(d_blas_tris=FAKE + 4))]
    # motion's refusals, before the new call's own
    shared += [dict(motion=nt.InstanceMotion(FAKE, 640, FAKE + 2, 0.5)), dict(motion=nt.InstanceMotion(0, 640, 0, 0.5)),
               dict(motion=nt.InstanceMotion(FAKE + 8, 640, FAKE, 0.5)), dict(motion=nt.InstanceMotion(FAKE, 639, FAKE, 0.5)),
               dict(motion=nt.InstanceMotion(0, 0, FAKE + 2, 0.5)), dict(motion=nt.InstanceMotion(FAKE, 639, FAKE, 0.5), d_results=0)]
    for change in shared:
        texts = []
        for fn, kw, name in ((nt.instanced_hit_attributes_motion, {}, "ntr_instanced_hit_attributes_motion"),
                             (nt.instanced_hit_attributes_deform, dict(deform=bad_deform), NAME)):
            with pytest.raises(nt.NtrError) as e:
                fn(**dict(dict(good, motion=motion), **change), **kw)
            assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: %s: " % name), (change, str(e.value))
            texts.append(str(e.value).split(name + ": ", 1)[1])
        assert texts[0] == texts[1], (change, texts)
    # the refusals of its own, in this order
    D = nt.InstancedDeformGeometry
    for change, text in [(dict(motion=None), "null motion"), (dict(motion=None, deform=bad_deform), "null motion"),
                         (dict(deform=D(0, FAKE)), "null d_vtxPos1"), (dict(deform=D(0, 0)), "null d_vtxPos1"),
                         (dict(deform=D(FAKE, 0)), "null d_blasDeforming"), (dict(deform=D(FAKE + 2, 0)), "null d_blasDeforming"),
                         (dict(deform=D(FAKE + 2, FAKE)), "d_vtxPos1 and d_blasDeforming must be 4-byte aligned"),
                         (dict(deform=D(FAKE, FAKE + 1)), "d_vtxPos1 and d_blasDeforming must be 4-byte aligned"),
                         (dict(motion=None, geom=None), "geom is null")]:
        with pytest.raises(nt.NtrError) as e:
            nt.instanced_hit_attributes_deform(**dict(dict(good, motion=motion, deform=deform), **change))
        assert e.value.code == -1 and str(e.value) == "ntrace_amd error -1: %s: %s" % (NAME, text), (change, str(e.value))
    # numRays == 0 is no work, with or without a device, whatever else is passed
    assert nt.lib().ntr_instanced_hit_attributes_deform(0, None, None, None, None, None, None, None, None) == 0
    assert nt.instanced_hit_attributes_deform(**dict(good, num_rays=0), motion=None, deform=bad_deform) is None
    if not _has_device():
        for m, d in ((motion, deform), (nt.InstanceMotion(FAKE, 640, 0, 0.5), deform), (motion, None), (None, None)):
            with pytest.raises(nt.NtrError) as e:
                nt.instanced_hit_attributes_deform(**good, motion=m, deform=d)
            assert e.value.code in (-2, -3), str(e.value)


def test_deform_null_is_the_motion_call():
    """deform == NULL delegates: a refusal names ntr_instanced_hit_attributes_motion, and with motion == NULL too the plain call."""
    good = dict(num_rays=64, d_results=FAKE, d_instance_ids=FAKE, geom=_geom(), d_out_results=FAKE, d_normals=FAKE)
    with pytest.raises(nt.NtrError) as e:
        nt.instanced_hit_attributes_deform(**dict(good, geom=None), motion=nt.InstanceMotion(FAKE, 640, FAKE, 0.5), deform=None)
    assert str(e.value) == "ntrace_amd error -1: ntr_instanced_hit_attributes_motion: geom is null"
    with pytest.raises(nt.NtrError) as e:
        nt.instanced_hit_attributes_deform(**good, motion=nt.InstanceMotion(FAKE, 639, FAKE, 0.5), deform=None)
    assert str(e.value).startswith("ntrace_amd error -1: ntr_instanced_hit_attributes_motion: ") and "motionKeysBytes below 128 * numInstances" in str(e.value)
    with pytest.raises(nt.NtrError) as e:
        nt.instanced_hit_attributes_deform(**dict(good, geom=None), motion=None, deform=None)
    assert str(e.value) == "ntrace_amd error -1: ntr_instanced_hit_attributes: geom is null"


def test_struct_layout():
    assert C.sizeof(nt.InstancedDeformGeometry) == 16 and nt.InstancedDeformGeometry.d_vtxPos1.offset == 0
    assert nt.InstancedDeformGeometry.d_blasDeforming.offset == 8
    assert hasattr(nt.lib(), NAME)
