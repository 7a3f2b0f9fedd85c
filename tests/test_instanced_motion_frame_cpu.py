"""Motion-blurred instanced frames without a device: the numpy rule (tests/np_instanced_motion_frame.py) against known answers, against
the older specs it is written over (np_instanced_frame.hit_attributes, np_instanced_motion's clamp, lerp and inverse), against binary64
over the triangles posed at the ray's time, on the self-occlusion demonstration, and the argument tables of ntr_ray_times_primary,
ntr_ray_times_secondary and ntr_instanced_hit_attributes_motion on fake pointers."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_motion_cases as mc
import instanced_motion_frame_cases as fc
import instanced_scenes as isc
import np_instanced as ni
import np_instanced_frame as nf
import np_instanced_motion as mo
import np_instanced_motion_frame as mf
from test_instanced_frame_cpu import geometry

F = np.float32
U = np.uint32

# (id, seed, hash x, time bits with open 0 and close 1), computed with plain Python integers apart from the spec and the kernel: both
# must meet them, so that a single misreading of the rule cannot satisfy both (tests/test_instanced_motion_frame_gpu.py: the kernel)
KNOWN = [(0, 0, 0x01FCE552, 0x3BFE7280), (1, 0, 0x9F505634, 0x3F1F5056), (2047, 0, 0xCD761963, 0x3F4D7619), (0, 1, 0x04F8D29E, 0x3C9F1A40),
         (5, 7, 0xA319CBB3, 0x3F2319CB), (0x7FFFFFFF, 0xFFFFFFFF, 0x8D29FFB8, 0x3F0D29FF)]
SHUTTERS = [(0.0, 1.0), (0.25, 0.75), (0.5, 0.5)]

# The largest 1 - |dot| of the spec's normal with the binary64 normal of the triangle posed at M(t_r) over the hits of the three scenes,
# as measured on the CPU against binary64 (never against the device), and the bound the test allows: 4 times that, for
# test_instanced_frame_cpu.py's reason (the float32 cross products of the soups' slivers cancel).
MEASURED_ONE_MINUS_DOT = 1.45e-7
BOUND = 4.0 * MEASURED_ONE_MINUS_DOT


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _words(out, normals):
    return out.tobytes(), normals.view(U).tobytes()


# ---- 1. ray times -----------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    for i, seed, x, bits in KNOWN:
        # plain Python integers, once more
        y = (i + (seed + 1) * 0x9E3779B9) & 0xFFFFFFFF
        y ^= y >> 16; y = (y * 0x7FEB352D) & 0xFFFFFFFF; y ^= y >> 15; y = (y * 0x846CA68B) & 0xFFFFFFFF; y ^= y >> 16
        assert y == x, (i, seed, hex(y))
        assert int(mf.hash_u32([i], seed)[0]) == x, (i, seed)
        assert int(mf.ray_times_primary(1, [i], seed)[0].view(U)) == bits, (i, seed)
    # as a table of int32 ids and without one
    assert int(mf.ray_times_primary(1, np.array([0x7FFFFFFF], np.int32), 0xFFFFFFFF)[0].view(U)) == 0x3F0D29FF
    assert [int(t.view(U)) for t in mf.ray_times_primary(2, None, 0)] == [0x3BFE7280, 0x3F1F5056]
    assert int(mf.ray_times_primary(2048, None, 0)[2047].view(U)) == 0x3F4D7619


def test_shutters_and_permutations():
    n = 4096
    rng = np.random.default_rng(2)
    ids = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    for seed in (0, 1, 0xFFFFFFFF):
        u = (mf.hash_u32(ids, seed) >> U(8)).astype(np.float64) * 2.0 ** -24
        assert u.min() >= 0 and u.max() <= 1 - 2.0 ** -24
        assert mf.ray_times_primary(n, ids, seed, 0.0, 1.0).tobytes() == u.astype(F).tobytes()     # u exactly
        for lo, hi in SHUTTERS[1:]:
            t = mf.ray_times_primary(n, ids, seed, lo, hi)
            assert (t >= F(lo)).all() and (t <= F(hi)).all()
        assert np.unique(mf.ray_times_primary(n, ids, seed, 0.25, 0.75)).size > n // 2
        assert (mf.ray_times_primary(n, ids, seed, 0.5, 0.5) == F(0.5)).all()
        # the time belongs to the pixel, not to the slot
        perm = rng.permutation(n)
        assert np.array_equal(mf.ray_times_primary(n, ids[perm], seed, 0.25, 0.75), mf.ray_times_primary(n, ids, seed, 0.25, 0.75)[perm])
    assert not np.array_equal(mf.ray_times_primary(n, ids, 0), mf.ray_times_primary(n, ids, 1))
    # a time past close after rounding is close: open + u * span rounds up to 1 at the top of [0.999, 1]
    top = mf.ray_times_primary(1 << 16, None, 3, 0.999, 1.0)
    assert top.max() <= F(1.0) and top.min() >= F(0.999)


def test_secondary_times_repeat_the_words():
    t = mf.ray_times_primary(64, None, 9)
    t[3], t[4] = np.array([0x7FC12345], U).view(F)[0], F(-0.0)
    for first, count, ns in ((0, 64, 1), (0, 1, 3), (5, 37, 8), (3, 2, 4)):
        got = mf.ray_times_secondary(t, first, count, ns)
        assert got.shape == (count * ns,) and got.view(U).tobytes() == np.repeat(t.view(U)[first:first + count], ns).tobytes()
    assert mf.ray_times_secondary(t, 3, 2, 4).view(U).tolist() == [0x7FC12345] * 4 + [0x80000000] * 4


# ---- 2. ties to the older specs ---------------------------------------------------------------------------------------------------------------
def _attr(s, inst1=None, **kw):
    ms = s["ms"]
    keys = mo.motion_keys(ms.inst0, ms.inst1 if inst1 is None else inst1)
    return mf.hit_attributes_motion(s["res"], s["ids"], ms.inst0, s["blas_tris"], s["tri"], s["pos"], keys, **kw)


def _plain(s, inst):
    return nf.hit_attributes(s["res"], s["ids"], inst, s["blas_tris"], s["tri"], s["pos"])


@pytest.mark.parametrize("name", mc.SCENES)
def test_ties_to_the_older_specs(name):
    """The records are the motion trace's at the hashed times; the attributes are a function of the records, the ids and the time alone,
    so one set of records serves every time."""
    s = fc.traced(name)
    ms = s["ms"]
    hit = s["res"]["id"] >= 0
    mv = mo.moving(ms.inst0, ms.inst1)
    assert hit.sum() > hit.size // 8 and mv[s["ids"][hit]].any() and (mv.all() or not mv[s["ids"][hit]].all())   # (mirror's two both move)
    today = _words(*_plain(s, ms.inst0))
    # key 1 == key 0: nothing moves, at any time
    assert _words(*_attr(s, inst1=ms.inst0, times=s["times"])) == today
    assert _words(*_attr(s, inst1=ms.inst0, time=0.5)) == today
    # the two ends are the keys
    assert _words(*_attr(s, time=0.0)) == today
    assert _words(*_attr(s, time=1.0)) == _words(*_plain(s, ms.inst1))
    assert _words(*_attr(s, time=1.0)) != today
    # in between: the instances posed at tau
    at = {}
    for tau in mc.INTERIOR:
        at[tau] = _words(*_attr(s, time=tau))
        assert at[tau] == _words(*_plain(s, fc.posed(ms.inst0, ms.inst1, tau)))
    assert len(set(at.values())) == len(mc.INTERIOR)
    # per-ray times: each ray takes its own pose
    n = hit.size
    pick = np.resize(np.array(mc.INTERIOR, F), n)
    out, nrm = _attr(s, times=pick)
    for tau in mc.INTERIOR:
        sel = pick == F(tau)
        assert nrm[sel].view(U).tobytes() == np.frombuffer(at[tau][1], U).reshape(-1, 4)[sel].tobytes()
    assert out.tobytes() == today[0]
    # the corner times go through the clamp: -1, 2, NaN, a denormal, 1 - 2^-24
    clamped = mo.clamp_time(mc.CORNER_TIMES)
    assert clamped.view(U).tolist() == [0, 0x3F800000, 0, 1, 0x3F7FFFFF]
    per_corner = []
    for c, k in zip(mc.CORNER_TIMES, clamped):
        per_corner.append(_attr(s, time=c)[1])
        assert per_corner[-1].view(U).tobytes() == _words(*_plain(s, fc.posed(ms.inst0, ms.inst1, k)))[1]
    pick = np.resize(mc.CORNER_TIMES, n)
    nrm = _attr(s, times=pick)[1]
    for j in range(mc.CORNER_TIMES.size):
        sel = np.arange(n) % mc.CORNER_TIMES.size == j
        assert nrm[sel].view(U).tobytes() == per_corner[j][sel].view(U).tobytes()


# ---- 3. against binary64 ----------------------------------------------------------------------------------------------------------------------
def _one_minus_dot(name):
    s = fc.traced(name)
    ms, res, ids = s["ms"], s["res"], s["ids"]
    out, normals = _attr(s, times=s["times"])
    hit = res["id"] >= 0
    assert np.array_equal(out["id"] >= 0, hit) and (normals[~hit] == 0).all() and (normals[hit, 3] == 1).all()
    i, lid = ids[hit].astype(np.int64), res["id"][hit].astype(np.int64)
    g = s["blas_tris"][ms.inst0["blas"][i], 0] + lid
    assert np.array_equal(out["id"][hit], g)
    # the triangle posed at M(t_r): the rule's binary32 lerp of the keys, then everything in binary64
    t = mo.clamp_time(s["times"])[hit]
    m = mo.lerp(ms.inst0["objectToWorld"].reshape(-1, 12)[i], ms.inst1["objectToWorld"].reshape(-1, 12)[i], t).astype(np.float64).reshape(-1, 3, 4)
    v = np.einsum("nij,nkj->nki", m[:, :, :3], s["pos"][s["tri"][g]].astype(np.float64)) + m[:, None, :, 3]
    n64 = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    n32 = normals[hit, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n32, axis=1) - 1.0).max() < 1e-6
    dot = (n32 * n64).sum(axis=1)
    return 1.0 - np.abs(dot), dot, np.linalg.det(m[:, :, :3]), mo.moving(ms.inst0, ms.inst1)[i]


@pytest.mark.parametrize("name", mc.SCENES)
def test_spec_against_binary64_at_the_rays_time(name):
    """The spec's normal at the ray's hashed time against the binary64 normal of the hit triangle posed at M(t_r).  Measured over the
    closest hits of the three scenes (isc.scene_rays((64, 32), 2048), times of seed 5): the largest 1 - |dot| is
    MEASURED_ONE_MINUS_DOT = 1.45e-7 (three 1.22e-7, grid 1.45e-7, mirror 1.25e-7); the test allows BOUND = 5.8e-7, 4 times the largest."""
    err, dot, det, moving = _one_minus_dot(name)
    print("%s: %d hits (%d on moving instances), largest 1 - |dot| = %.3g (bound %.3g)" % (name, err.size, int(moving.sum()), float(err.max()), BOUND))
    assert moving.any() and err.max() <= BOUND, (name, float(err.max()), BOUND)
    if name == "mirror":
        assert (det < 0).any()
    # the normal follows the object's winding: against the posed triangle's normal exactly where M(t) mirrors
    assert (det != 0).all() and np.array_equal(dot < 0, det < 0)


# ---- 4. a pose without an inverse -------------------------------------------------------------------------------------------------------------
def test_singular_pose_resolves_the_id_and_gives_no_normal():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    ms = mc.two_of_one(a, b.reshape(12))
    rays = mc.one_rays()
    rid, rt, ru, rv, rinst, _ = ms.trace(rays, False, time=0.25)
    res, ids = fc.records(rid, rt, ru, rv), rinst.astype(np.int32)
    on0, on1 = (rid >= 0) & (ids == 0), (rid >= 0) & (ids == 1)
    assert on0.any() and on1.any()
    tri, pos, blas_tris = geometry(["one"])
    keys = ms.refit["motion_keys"]
    out, nrm = mf.hit_attributes_motion(res, ids, ms.inst0, blas_tris, tri, pos, keys, time=0.5)
    assert (out["id"][on0] == 0).all() and (nrm[on0].view(U) == 0).all()            # resolved, and no normal
    assert (out["id"][on1] == 0).all() and (nrm[on1, 3] == 1).all()                 # the static instance beside it is untouched
    out, nrm = mf.hit_attributes_motion(res, ids, ms.inst0, blas_tris, tri, pos, keys, time=0.25)
    assert (nrm[on0 | on1, 3] == 1).all()
    # per-ray times: only the rays at exactly 0.5 lose their normal
    t = np.where(np.arange(rays.shape[0]) % 2 == 0, F(0.5), F(0.25)).astype(F)
    out, nrm = mf.hit_attributes_motion(res, ids, ms.inst0, blas_tris, tri, pos, keys, times=t)
    assert np.array_equal(nrm[on0, 3] == 0, (t == F(0.5))[on0]) and (out["id"][on0] == 0).all()


# ---- 5. the demonstration: a convex cube that turns inside the shutter --------------------------------------------------------------------------
def test_a_secondary_ray_must_see_its_instance_where_its_primary_ray_saw_it():
    """instanced_motion_frame_cases.demo(): 64 x 32 primary rays with one hashed time per pixel, 8 AO rays of radius 3 per hit.  The
    moving cube is convex, so no AO ray may hit the instance it started from.  Measured on the spec alone: 220 primary hits (100 on the
    moving cube), 1760 live AO rays; self hits 0 with the normals at the ray's time and the primary ray's time inherited, 290 with the
    secondary times all 0, 45 with today's key-0 normals."""
    d = fc.demo()
    ms, rays = d["ms"], d["rays"]
    n = rays.shape[0]
    times = mf.ray_times_primary(n, d["s2i"], 0)
    rid, rt, ru, rv, rinst, _ = ms.trace(rays, False, times=times)
    res, ids = fc.records(rid, rt, ru, rv), rinst.astype(np.int32)
    assert ((rid >= 0) & (ids == 0)).sum() > 64 and ((rid >= 0) & (ids == 1)).sum() > 64
    keys = ms.refit["motion_keys"]
    src = np.repeat(ids, fc.DEMO_NS)

    def self_hits(attributes, sec_times):
        srays = fc.ao_batch(rays, *attributes)
        assert (srays["tmax"] > 0).sum() == fc.DEMO_NS * (rid >= 0).sum()
        sid, _, _, _, sinst, _ = ms.trace(srays, True, times=sec_times)
        return int(((sid >= 0) & (sinst == src) & (src == 0)).sum())
    at_time = mf.hit_attributes_motion(res, ids, ms.inst0, d["blas_tris"], d["tri"], d["pos"], keys, times=times)
    at_key0 = nf.hit_attributes(res, ids, ms.inst0, d["blas_tris"], d["tri"], d["pos"])
    inherited = mf.ray_times_secondary(times, 0, n, fc.DEMO_NS)
    rows = (self_hits(at_time, inherited), self_hits(at_time, np.zeros(n * fc.DEMO_NS, F)), self_hits(at_key0, inherited))
    print("self hits: %d at the ray's time with inherited times, %d with secondary times 0, %d with key-0 normals" % rows)
    assert rows[0] == 0 and rows[1] > 0 and rows[2] > 0, rows


# ---- 6. refusals, before any device work --------------------------------------------------------------------------------------------------------
FAKE = 0x10000


def _refused(fn, name, good, cases):
    for change, text in cases:
        with pytest.raises(nt.NtrError) as e:
            fn(**dict(good, **change))
        assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: %s: " % name) and text in str(e.value), (change, str(e.value))


def test_ray_times_argument_errors_and_no_device():
    good = dict(num_rays=64, d_slot_to_id=FAKE, seed=0, open=0.0, close=1.0, d_times=FAKE)
    nan, inf = float("nan"), float("inf")
    _refused(nt.ray_times_primary, "ntr_ray_times_primary", good,
             [(dict(num_rays=-1), "numRays < 0"), (dict(d_times=0), "d_times is null"), (dict(d_times=FAKE + 2), "4-byte aligned"),
              (dict(open=nan), "0 <= open <= close <= 1"), (dict(close=nan), "0 <= open"), (dict(close=inf), "0 <= open"),
              (dict(open=-inf), "0 <= open"), (dict(open=-0.25), "0 <= open"), (dict(open=0.75, close=0.5), "0 <= open"),
              (dict(close=1.5), "0 <= open"), (dict(num_rays=0, close=2.0), "0 <= open")])
    assert nt.ray_times_primary(**dict(good, num_rays=0, d_times=0)) is None
    assert nt.ray_times_primary(**dict(good, d_slot_to_id=0, num_rays=0)) is None
    good2 = dict(d_in_times=FAKE, first_input_slot=0, num_input_rays=64, num_samples=4, d_out_times=FAKE)
    _refused(nt.ray_times_secondary, "ntr_ray_times_secondary", good2,
             [(dict(num_input_rays=-1), "negative count or slot"), (dict(first_input_slot=-1), "negative count or slot"),
              (dict(num_samples=0), "numSamples < 1"), (dict(num_samples=-3), "numSamples < 1"), (dict(num_input_rays=0, num_samples=0), "numSamples < 1"),
              (dict(num_input_rays=1 << 20, num_samples=1 << 11), "below 2^31"), (dict(num_input_rays=2 ** 31 - 1, num_samples=2 ** 31 - 1), "below 2^31"),
              (dict(d_in_times=0), "null buffer"), (dict(d_out_times=0), "null buffer"), (dict(d_in_times=FAKE + 1), "4-byte aligned"),
              (dict(d_out_times=FAKE + 2), "4-byte aligned")])
    assert nt.ray_times_secondary(**dict(good2, num_input_rays=0, d_in_times=0, d_out_times=0)) is None
    if not _has_device():
        for fn, args in ((nt.ray_times_primary, good), (nt.ray_times_primary, dict(good, d_slot_to_id=0)), (nt.ray_times_secondary, good2),
                         (nt.ray_times_secondary, dict(good2, num_input_rays=(1 << 20) - 1, num_samples=1 << 11))):
            with pytest.raises(nt.NtrError) as e:
                fn(**args)
            assert e.value.code in (-2, -3), str(e.value)


def test_attributes_argument_errors_and_no_device():
    """The shared refusals come in ntr_instanced_hit_attributes' words and order under the new name: every case is put to both entry
    points, and the two messages differ in the name alone."""
    def g(**kw):
        return nt.InstancedGeometry(**dict(dict(num_instances=5, num_blas=3, num_tris_total=100, num_verts=300, d_instances=FAKE, d_blas_tris=FAKE,
                                                d_tri=FAKE, d_pos=FAKE), **kw))
    motion = nt.InstanceMotion(FAKE, 128 * 5, FAKE, 0.5)
    good = dict(num_rays=64, d_results=FAKE, d_instance_ids=FAKE, geom=g(), d_out_results=FAKE, d_normals=FAKE)
    shared = [dict(geom=None), dict(d_out_results=0, d_normals=0), dict(d_normals=FAKE + 4), dict(d_normals=FAKE + 8), dict(d_out_results=FAKE + 4),
              dict(num_rays=-1), dict(d_results=0), dict(d_instance_ids=0), dict(d_results=FAKE + 8)]
    shared += [dict(geom=g(**{k: 0})) for k in ("num_instances", "num_blas", "num_tris_total", "num_verts", "d_instances", "d_blas_tris", "d_tri",
                                                "d_pos")]
    shared += [dict(geom=g(num_instances=-1)), dict(geom=g(d_instances=FAKE + 8)), dict(geom=g(d_blas_tris=FAKE + 4))]
    # order: a call wrong in several ways names the first; motion's own refusals come last
    shared += [dict(num_rays=-1, geom=None), dict(geom=g(d_pos=0, num_blas=0)), dict(geom=g(num_verts=0), d_results=0),
               dict(d_instance_ids=0, d_out_results=0, d_normals=0), dict(d_out_results=0, d_normals=0, geom=g(d_instances=FAKE + 8)),
               dict(d_normals=FAKE + 4, geom=g(d_blas_tris=FAKE + 4))]
    bad_motion = nt.InstanceMotion(0, 0, FAKE + 2, 0.5)
    for change in shared:
        texts = []
        for fn, kw, name in ((nt.instanced_hit_attributes, {}, "ntr_instanced_hit_attributes"),
                             (nt.instanced_hit_attributes_motion, dict(motion=bad_motion), "ntr_instanced_hit_attributes_motion")):
            with pytest.raises(nt.NtrError) as e:
                fn(**dict(good, **change), **kw)
            assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: %s: " % name), (change, str(e.value))
            texts.append(str(e.value).split(name + ": ", 1)[1])
        assert texts[0] == texts[1], (change, texts)
    # the refusals of its own, in the motion trace's words and order
    _refused(nt.instanced_hit_attributes_motion, "ntr_instanced_hit_attributes_motion", good,
             [(dict(motion=nt.InstanceMotion(FAKE, 640, FAKE + 2, 0.5)), "the ray times must be 4-byte aligned"),
              (dict(motion=nt.InstanceMotion(0, 640, 0, 0.5)), "the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
              (dict(motion=nt.InstanceMotion(FAKE + 8, 640, FAKE, 0.5)), "the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
              (dict(motion=nt.InstanceMotion(FAKE, 639, FAKE, 0.5)), "motionKeysBytes below 128 * numInstances"),
              (dict(motion=bad_motion), "the ray times must be 4-byte aligned"),
              (dict(motion=nt.InstanceMotion(FAKE + 8, 0, 0, 0.5)), "the motion keys")])
    # motion == NULL is ntr_instanced_hit_attributes, and its refusals name that function
    with pytest.raises(nt.NtrError) as e:
        nt.instanced_hit_attributes_motion(**dict(good, geom=None), motion=None)
    assert str(e.value).startswith("ntrace_amd error -1: ntr_instanced_hit_attributes: geom is null")
    # numRays == 0 is no work, with or without a device, whatever else is passed
    assert nt.lib().ntr_instanced_hit_attributes_motion(0, None, None, None, None, None, None, None) == 0
    assert nt.instanced_hit_attributes_motion(**dict(good, num_rays=0), motion=bad_motion) is None
    assert nt.lib().ntr_ray_times_primary(0, None, 0, 0.0, 1.0, None, None) == 0
    assert nt.lib().ntr_ray_times_secondary(None, 0, 0, 1, None, None) == 0
    if not _has_device():
        for m in (motion, nt.InstanceMotion(FAKE, 640, 0, 0.5), None):
            with pytest.raises(nt.NtrError) as e:
                nt.instanced_hit_attributes_motion(**good, motion=m)
            assert e.value.code in (-2, -3), str(e.value)


def test_struct_layouts():
    assert C.sizeof(nt.InstanceMotion) == 32 and nt.InstanceMotion.d_rayTimes.offset == 16 and nt.InstanceMotion.time.offset == 24
    assert C.sizeof(nt.InstancedGeometry) == 48 and nt.InstancedGeometry.d_instances.offset == 16
    assert mo.KEY_BYTES == 128 and mo.KEY_WORDS == 32
    for name in ("ntr_ray_times_primary", "ntr_ray_times_secondary", "ntr_instanced_hit_attributes_motion"):
        assert hasattr(nt.lib(), name)
