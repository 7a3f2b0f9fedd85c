"""Motion-blurred instanced frames on the device against the numpy rule (tests/np_instanced_motion_frame.py): ntr_ray_times_primary and
ntr_ray_times_secondary equal the rule bit for bit (and the primary kernel the known answers); ntr_instanced_hit_attributes_motion
equals hit_attributes_motion() in every word over records ntr_trace_instanced_motion wrote at hashed times, at the ray counts around a
workgroup, with per-ray times and the scalar, in place and with either output alone, over a pose without an inverse and over hand-made
records whose every index is out of range once; a whole frame at the C-ABI has no self hits on the demonstration's convex cube, step by
step equal to the specs; the frame with its motion refit replays as one linear graph.  Output buffers are prefilled with 0xAB and
nothing beyond the extents may change."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_motion_cases as mc
import instanced_motion_frame_cases as fc
import instanced_scenes as isc
import np_instanced as ni
import np_instanced_frame as nf
import np_instanced_motion as mo
import np_instanced_motion_frame as mf
import np_raygen
from gpu_util import up
from test_instanced_frame_cpu import geometry
from test_instanced_motion_frame_cpu import KNOWN, SHUTTERS
from test_instanced_motion_gpu import _Dev, _Traced

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
SLACK = 64
INT_MAX = 2 ** 31 - 1
TOL = 1e-5           # tests/test_raygen_gpu.py's bound on a generated direction
_cache = {}


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


def _down(buf, nbytes, what=""):
    raw = buf.cpu().numpy()
    assert (raw[nbytes:] == 0xAB).all(), "bytes beyond the extents were written: " + what
    return raw[:nbytes].copy()


# ---- 1. ray times -----------------------------------------------------------------------------------------------------------------------------
def _primary_times(n, table, seed, lo, hi):
    d_t = _filled(4 * n)
    d_tab = up(table) if table is not None else None
    nt.ray_times_primary(n, d_tab.data_ptr() if d_tab is not None else 0, seed, lo, hi, d_t.data_ptr())
    torch.cuda.synchronize()
    return _down(d_t, 4 * n, "ray times").view(U)


def test_primary_times_meet_the_known_answers():
    for i, seed, _, bits in KNOWN:
        assert int(_primary_times(1, np.array([i], np.int32), seed, 0.0, 1.0)[0]) == bits, (i, seed)
    got = _primary_times(2048, None, 0, 0.0, 1.0)
    assert [int(got[0]), int(got[1]), int(got[2047])] == [0x3BFE7280, 0x3F1F5056, 0x3F4D7619]


@pytest.mark.parametrize("n", [1, 63, 65, 2048])
def test_primary_times_equal_spec(n):
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.int32)
    wild = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)          # any word is an id
    for table in (None, perm, wild):
        for seed in (0, 1, 0xFFFFFFFF):
            for lo, hi in SHUTTERS:
                got = _primary_times(n, table, seed, lo, hi)
                want = mf.ray_times_primary(n, table, seed, lo, hi).view(U)
                assert np.array_equal(got, want), (n, seed, lo, hi, int(np.flatnonzero(got != want)[0]))
    # the time belongs to the pixel: permuted slots, permuted times
    assert np.array_equal(_primary_times(n, perm, 1, 0.25, 0.75), _primary_times(n, None, 1, 0.25, 0.75)[perm])


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("count", [1, 37])
def test_secondary_times_equal_spec(first, count):
    t = mf.ray_times_primary(64, None, 9)
    t[first], t[first + count - 1] = np.array([0x7FC12345], U).view(F)[0], F(-0.0)
    if count == 1:
        t[first] = np.array([0xFFC00001], U).view(F)[0]
    d_in = up(t)
    for ns in (1, 3, 8):
        m = count * ns
        d_out = torch.full((64 + 4 * m + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")      # guard words on both sides
        nt.ray_times_secondary(d_in.data_ptr(), first, count, ns, d_out.data_ptr() + 64)
        torch.cuda.synchronize()
        raw = d_out.cpu().numpy()
        assert (raw[:64] == 0xAB).all() and (raw[64 + 4 * m:] == 0xAB).all(), "a word outside the window was written"
        got = raw[64:64 + 4 * m].view(U)
        assert np.array_equal(got, mf.ray_times_secondary(t, first, count, ns).view(U)), (first, count, ns)
        assert np.array_equal(got, np.repeat(t.view(U)[first:first + count], ns))
    assert d_in.cpu().numpy().tobytes() == t.tobytes()


# ---- 2. the attributes at the ray's time ------------------------------------------------------------------------------------------------------
class _Attr:
    """A motion scene on the device (tests/test_instanced_motion_gpu.py's _Traced: pool, two keys, the motion-refitted tree) with its
    meshes: the NtrInstancedGeometry over key 0 and the NtrInstanceMotion over the key buffer the refit wrote."""

    def __init__(self, ms, tri, pos, blas_tris):
        self.t = _Traced(ms)
        self.ms, self.d = ms, self.t.d
        self.tri, self.pos, self.blas_tris = tri, pos, np.asarray(blas_tris, np.int32).reshape(-1, 2)
        self.d_tri, self.d_pos, self.d_bt = up(tri), up(pos), up(self.blas_tris)
        self.geom = nt.InstancedGeometry(self.d.n, self.blas_tris.shape[0], tri.shape[0], pos.shape[0], self.d.d_inst0.data_ptr(), self.d_bt.data_ptr(),
                                         self.d_tri.data_ptr(), self.d_pos.data_ptr())
        self.keep = []

    def motion(self, times=None, time=0.0):
        d_t = up(np.asarray(times, F)) if times is not None else None
        self.keep = [d_t]
        return nt.InstanceMotion(self.d.d_keys.data_ptr(), self.d.keys_bytes, d_t.data_ptr() if d_t is not None else 0, time)

    def trace(self, rays, any_hit=False, times=None, time=0.0, stream=0):
        """ntr_trace_instanced_motion -> (d_res, d_ids, host records, host ids)"""
        n = rays.shape[0]
        d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
        nt.trace_instanced_motion(*self.t.args(n, any_hit, d_rays, d_res, d_ids), vis=None, motion=self.motion(times, time), stream=stream, timed=False)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        return d_res, d_ids, _down(d_res, 16 * n, "records").view(nt.RESULT_DTYPE), _down(d_ids, 4 * n, "instance ids").view(np.int32)

    def spec(self, res, ids, times=None, time=0.0):
        return mf.hit_attributes_motion(res, ids, self.ms.inst0, self.blas_tris, self.tri, self.pos, self.t.keys, times=times, time=time)

    def attributes(self, n, d_res, d_ids, motion, out=True, normals=True, in_place=False, stream=0):
        d_out = d_res if in_place else (_filled(16 * n) if out else None)
        d_nrm = _filled(16 * n) if normals else None
        nt.instanced_hit_attributes_motion(n, d_res.data_ptr(), d_ids.data_ptr(), self.geom, motion, d_out.data_ptr() if d_out is not None else 0,
                                           d_nrm.data_ptr() if d_nrm is not None else 0, stream)
        return d_out, d_nrm

    def assert_equal(self, n, want, d_out, d_nrm, what):
        torch.cuda.synchronize()
        want_out, want_nrm = want
        if d_out is not None:
            got = _down(d_out, 16 * n, str(what)).view(U).reshape(-1, 4)
            bad = np.flatnonzero((got != want_out[:n].view(U).reshape(-1, 4)).any(axis=1))
            assert bad.size == 0, ("records differ", what, int(bad[0]), got[bad[0]], want_out[bad[0]])
        if d_nrm is not None:
            got = _down(d_nrm, 16 * n, str(what)).view(U).reshape(-1, 4)
            bad = np.flatnonzero((got != want_nrm[:n].view(U).reshape(-1, 4)).any(axis=1))
            assert bad.size == 0, ("normals differ", what, bad.size, int(bad[0]), got[bad[0]].view(F), want_nrm[bad[0]])

    def check(self, res, ids, d_res, d_ids, what, times=None, time=0.0, forms=False):
        """The device against the rule, for per-ray times or the scalar -> the rule's outputs"""
        n = res.shape[0]
        want = self.spec(res, ids, times, time)
        self.assert_equal(n, want, *self.attributes(n, d_res, d_ids, self.motion(times, time)), what)
        if forms:      # each output alone, then in place over a copy of the records
            self.assert_equal(n, want, *self.attributes(n, d_res, d_ids, self.motion(times, time), normals=False), (what, "records alone"))
            self.assert_equal(n, want, *self.attributes(n, d_res, d_ids, self.motion(times, time), out=False), (what, "normals alone"))
            d_copy = _filled(16 * n)
            d_copy[:16 * n] = d_res[:16 * n]
            d_out, d_nrm = self.attributes(n, d_copy, d_ids, self.motion(times, time), in_place=True)
            assert d_out is d_copy
            self.assert_equal(n, want, d_out, d_nrm, (what, "in place"))
            assert _down(d_res, 16 * n).tobytes() == res.tobytes(), "the input records changed"
        return want


def _scene(name):
    if name not in _cache:
        _cache[name] = _Attr(fc.motion_scene(name), *geometry(fc.names_of(name)))
    return _cache[name]


@pytest.mark.parametrize("name", mc.SCENES + ["big"])
def test_attributes_equal_spec_on_the_scenes(name):
    s = _scene(name)
    rays, times = fc.rays_and_times()
    n = rays.shape[0]
    d_res, d_ids, res, ids = s.trace(rays, False, times=times)
    hit = res["id"] >= 0
    mv = mo.moving(s.ms.inst0, s.ms.inst1)
    assert hit.sum() > n // 16 and mv[ids[hit]].any()
    if name != "big":          # the trace's records are the rule's: the CPU tier's inputs are these
        assert res.tobytes() == fc.traced(name)["res"].tobytes() and ids.tobytes() == fc.traced(name)["ids"].tobytes()
    want = s.check(res, ids, d_res, d_ids, name + " hashed times", times=times, forms=True)
    assert np.array_equal(want[0]["id"] >= 0, hit) and np.array_equal(want[1][:, 3] == 1, hit)
    today = nf.hit_attributes(res, ids, s.ms.inst0, s.blas_tris, s.tri, s.pos)
    assert want[0].tobytes() == today[0].tobytes() and want[1].tobytes() != today[1].tobytes()      # the ids are today's, the normals are not
    # the scalar: the ends, the middle, the corner times; then the corner times per ray
    s.check(res, ids, d_res, d_ids, name + " t = 0", time=0.0)
    s.check(res, ids, d_res, d_ids, name + " t = 1", time=1.0)
    s.check(res, ids, d_res, d_ids, name + " t = 0.5", time=0.5)
    for t in mc.CORNER_TIMES:
        s.check(res, ids, d_res, d_ids, "%s scalar time %r" % (name, t), time=float(t) if t == t else float("nan"))
    s.check(res, ids, d_res, d_ids, name + " corner times per ray", times=np.resize(mc.CORNER_TIMES, n))
    # t = 0 is key 0, and motion == NULL is ntr_instanced_hit_attributes: the bytes of today's call
    d_o0, d_n0 = _filled(16 * n), _filled(16 * n)
    nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), s.geom, d_o0.data_ptr(), d_n0.data_ptr())
    s.assert_equal(n, today, d_o0, d_n0, "today's call")
    s.assert_equal(n, today, *s.attributes(n, d_res, d_ids, None), "motion == NULL")
    s.assert_equal(n, today, *s.attributes(n, d_res, d_ids, s.motion(time=0.0)), "t = 0")
    # any-hit records resolve alike
    d_res, d_ids, res, ids = s.trace(rays, True, times=times)
    s.check(res, ids, d_res, d_ids, name + " any hit", times=times)


@pytest.mark.parametrize("n", [1, 255, 257, 4096])
def test_ray_counts(n):
    s = _scene("three")
    rays, times = fc.rays_and_times()
    assert rays.shape[0] == 4096
    if "first hit" not in _cache:
        _cache["first hit"] = int(np.flatnonzero(fc.traced("three")["res"]["id"] >= 0)[0])
    k = _cache["first hit"]                       # a single ray is a hit
    rays, times = np.roll(rays, -k)[:n], np.roll(times, -k)[:n].copy()
    d_res, d_ids, res, ids = s.trace(rays, False, times=times)
    want = s.check(res, ids, d_res, d_ids, "%d rays" % n, times=times, forms=True)
    assert want[0]["id"][0] >= 0 and want[1][0, 3] == 1
    s.check(res, ids, d_res, d_ids, "%d rays, scalar" % n, time=0.3)


def test_singular_pose_resolves_the_id_and_gives_no_normal():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    s = _Attr(mc.two_of_one(a, b.reshape(12)), *geometry(["one"]))
    rays = mc.one_rays()
    d_res, d_ids, res, ids = s.trace(rays, False, time=0.25)
    on0, on1 = (res["id"] >= 0) & (ids == 0), (res["id"] >= 0) & (ids == 1)
    assert on0.any() and on1.any()
    out, nrm = s.check(res, ids, d_res, d_ids, "singular at 0.5", time=0.5, forms=True)
    assert (out["id"][on0] == 0).all() and (nrm[on0].view(U) == 0).all() and (nrm[on1, 3] == 1).all()
    out, nrm = s.check(res, ids, d_res, d_ids, "not singular at 0.25", time=0.25)
    assert (nrm[on0 | on1, 3] == 1).all()
    t = np.where(np.arange(rays.shape[0]) % 2 == 0, F(0.5), F(0.25)).astype(F)
    out, nrm = s.check(res, ids, d_res, d_ids, "every other ray singular", times=t)
    assert np.array_equal(nrm[on0, 3] == 0, (t == F(0.5))[on0])


def test_synthetic_records_never_read_outside_the_buffers():
    """tests/test_instanced_frame_gpu.py's hand-made batch over a scene with two keys: one ray per way an index can be out of range,
    between good rays on moving and on static instances; every outcome is the rule's."""
    tri, pos, bt = geometry(["cornell", "soup1000", "one"])
    nv0, nt0 = pos.shape[0], tri.shape[0]
    tiny = np.array([(0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0)], F)
    pos = np.concatenate([pos, tiny]).astype(F)
    nv = pos.shape[0]
    special = np.array([(nv, 0, 1), (0, -1, 1), (nv0, nv0 + 1, nv0 + 2)], np.int32)
    tri = np.concatenate([tri, special]).astype(np.int32)
    bt = np.concatenate([bt, [(nt0, 3), (0, 0)]]).astype(np.int32)            # BLAS 3: the special triangles; BLAS 4: numTris 0
    num_blas = bt.shape[0]
    tf = isc.seeded_transforms(8, 77, mirrored=2)
    which = [0, 1, 2, 3, 4, 0, 0, 1]
    inst0, inst1 = ni.instances(tf, which), ni.instances(mc.key1_transforms(tf), which)      # 2 and 5 stand still
    for inst in (inst0, inst1):
        inst["blas"][5], inst["blas"][6] = -1, num_blas
    assert mo.moving(inst0, inst1).tolist() == [True, True, False, True, True, False, True, True]
    num_inst = inst0.shape[0]
    keys = mo.motion_keys(inst0, inst1)
    d_inst, d_keys, d_tri, d_pos, d_bt = up(inst0), _filled(128 * num_inst), up(tri), up(pos), up(bt)
    d_keys[:128 * num_inst] = up(keys)
    geom = nt.InstancedGeometry(num_inst, num_blas, tri.shape[0], pos.shape[0], d_inst.data_ptr(), d_bt.data_ptr(), d_tri.data_ptr(), d_pos.data_ptr())
    cases = [                                  # (what, id, instance)
        ("a good ray", 3, 0), ("a miss", -1, -1), ("a miss with an instance", -1, 1), ("instance -1 with id >= 0", 5, -1),
        ("instance == numInstances", 5, num_inst), ("instance INT_MAX", 5, INT_MAX), ("instance INT_MIN", 5, -INT_MAX - 1),
        ("blas -1", 0, 5), ("blas == numBlas", 0, 6), ("id == numTris", int(bt[0, 1]), 0), ("id == numTris - 1", int(bt[0, 1]) - 1, 0),
        ("id == numTris of the soup", int(bt[1, 1]), 7), ("id -2", -2, 0), ("id INT_MAX", INT_MAX, 1), ("id INT_MIN", -INT_MAX - 1, 1),
        ("a vertex index == numVerts", 0, 3), ("a vertex index -1", 1, 3), ("edges of 1e-20", 2, 3), ("a BLAS of no triangles", 0, 4),
        ("the single triangle, static", 0, 2), ("a good ray of the soup", 999, 7)]
    n = len(cases)
    res = np.zeros(n, nt.RESULT_DTYPE)
    res["id"] = [c[1] for c in cases]
    res["t"] = np.linspace(0.5, 9.5, n).astype(F)
    res["padA"], res["padB"] = np.arange(n) + 0x3e000000, np.arange(n) + 0x3f000000
    ids = np.array([c[2] for c in cases], np.int32)
    times = mf.ray_times_primary(n, None, 4)
    want_out, want_nrm = mf.hit_attributes_motion(res, ids, inst0, bt, tri, pos, keys, times=times)
    what = [c[0] for c in cases]
    resolved = {"a good ray", "id == numTris - 1", "edges of 1e-20", "the single triangle, static", "a good ray of the soup"}
    assert {w for w, o in zip(what, want_out["id"]) if o >= 0} == resolved
    assert {w for w, m in zip(what, want_nrm[:, 3]) if m == 1} == resolved - {"edges of 1e-20"}
    today = nf.hit_attributes(res, ids, inst0, bt, tri, pos)[1]
    k = what.index("the single triangle, static")
    assert want_nrm[k].tobytes() == today[k].tobytes() and want_nrm[0].tobytes() != today[0].tobytes()
    d_res, d_ids, d_t = _filled(16 * n), _filled(4 * n), up(times)
    d_res[:16 * n] = up(res)
    d_ids[:4 * n] = up(ids)
    motion = nt.InstanceMotion(d_keys.data_ptr(), 128 * num_inst, d_t.data_ptr(), 0.0)
    for in_place in (False, True):
        d_out, d_nrm = (d_res if in_place else _filled(16 * n)), _filled(16 * n)
        nt.instanced_hit_attributes_motion(n, d_res.data_ptr(), d_ids.data_ptr(), geom, motion, d_out.data_ptr(), d_nrm.data_ptr())
        torch.cuda.synchronize()
        assert _down(d_out, 16 * n).tobytes() == want_out.tobytes(), in_place
        assert _down(d_nrm, 16 * n).tobytes() == want_nrm.tobytes(), in_place
    assert _down(d_keys, 128 * num_inst).tobytes() == keys.tobytes()
    assert nt.trace_status() == 0


def test_a_wave_of_static_and_moving_hits_and_a_wave_of_static_hits():
    """64 consecutive rays alternate hits on a static and on a moving instance, another 64 are all on static instances, then a third
    wave all moving: both sides of the vote, and a wave in which the lanes part."""
    s = _scene("three")
    mv = mo.moving(s.ms.inst0, s.ms.inst1)
    still, moves = int(np.flatnonzero(~mv)[0]), int(np.flatnonzero(mv)[0])
    n = 192
    ids = np.concatenate([np.where(np.arange(64) % 2 == 0, still, moves), np.full(64, still), np.full(64, moves)]).astype(np.int32)
    num_tris = s.blas_tris[s.ms.inst0["blas"][ids], 1]
    res = np.zeros(n, nt.RESULT_DTYPE)
    res["id"] = (np.arange(n) * 7) % num_tris
    res["t"] = F(1.0)
    times = mf.ray_times_primary(n, None, 6, 0.125, 0.875)
    d_res, d_ids = _filled(16 * n), _filled(4 * n)
    d_res[:16 * n] = up(res)
    d_ids[:4 * n] = up(ids)
    out, nrm = s.check(res, ids, d_res, d_ids, "wave mix", times=times, forms=True)
    assert (out["id"] >= 0).all() and (nrm[:, 3] == 1).all()
    today = nf.hit_attributes(res, ids, s.ms.inst0, s.blas_tris, s.tri, s.pos)[1]
    same = (nrm.view(U) == today.view(U)).all(axis=1)
    assert same[ids == still].all() and not same[ids == moves].any()


# ---- 3. the frame at the C-ABI ----------------------------------------------------------------------------------------------------------------
class _Frame:
    """The demonstration's frame: times -> motion trace -> attributes at the ray's time -> ntr_raygen_ao_normals -> secondary times ->
    any-hit motion trace, over one _Attr; every call on `stream`."""

    def __init__(self, s, rays, s2i, ns, radius, ao_seed):
        self.s, self.rays, self.n, self.ns, self.radius, self.ao_seed = s, rays, rays.shape[0], ns, radius, ao_seed
        n, m = self.n, self.n * ns
        self.m = m
        self.d_rays, self.d_s2i = up(rays), up(s2i)
        self.bufs = dict(times=_filled(4 * n), res=_filled(16 * n), ids=_filled(4 * n), out=_filled(16 * n), nrm=_filled(16 * n), srays=_filled(32 * m),
                         si2s=_filled(4 * m), ss2i=_filled(4 * m), stimes=_filled(4 * m), sres=_filled(16 * m), sids=_filled(4 * m))

    def run(self, seed, stream=0):
        s, b, n, m = self.s, self.bufs, self.n, self.m
        p = {k: v.data_ptr() for k, v in b.items()}
        nt.ray_times_primary(n, self.d_s2i.data_ptr(), seed, 0.0, 1.0, p["times"], stream)
        pm = nt.InstanceMotion(s.d.d_keys.data_ptr(), s.d.keys_bytes, p["times"], 0.0)
        nt.trace_instanced_motion(*s.t.args(n, False, self.d_rays, b["res"], b["ids"]), vis=None, motion=pm, stream=stream, timed=False)
        nt.instanced_hit_attributes_motion(n, p["res"], p["ids"], s.geom, pm, p["out"], p["nrm"], stream)
        nt.raygen_ao_normals(p["srays"], p["si2s"], p["ss2i"], self.d_rays.data_ptr(), p["out"], p["nrm"], 0, n, self.ns, self.radius, self.ao_seed, stream)
        nt.ray_times_secondary(p["times"], 0, n, self.ns, p["stimes"], stream)
        sm = nt.InstanceMotion(s.d.d_keys.data_ptr(), s.d.keys_bytes, p["stimes"], 0.0)
        nt.trace_instanced_motion(*s.t.args(m, True, b["srays"], b["sres"], b["sids"]), vis=None, motion=sm, stream=stream, timed=False)

    def download(self):
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        sizes = dict(times=4, res=16, ids=4, out=16, nrm=16)
        return {k: _down(v, (sizes[k] * self.n) if k in sizes else {"srays": 32, "si2s": 4, "ss2i": 4, "stimes": 4, "sres": 16, "sids": 4}[k] * self.m, k)
                for k, v in self.bufs.items()}

    def assert_equals_specs(self, got, ms, keys, s2i, seed, what):
        """Each device step against its spec, fed with the device's own inputs of that step -> self hits on instance 0"""
        s, n, m = self.s, self.n, self.m
        times = got["times"].view(F)
        assert times.tobytes() == mf.ray_times_primary(n, s2i, seed).tobytes(), (what, "times")
        rid, rt, ru, rv, rinst, _ = ms.trace(self.rays, False, times=times)
        res, ids = fc.records(rid, rt, ru, rv), rinst.astype(np.int32)
        assert got["res"].tobytes() == res.tobytes() and got["ids"].tobytes() == ids.tobytes(), (what, "primary records")
        out, nrm = mf.hit_attributes_motion(res, ids, ms.inst0, s.blas_tris, s.tri, s.pos, keys, times=times)
        assert got["out"].tobytes() == out.tobytes() and got["nrm"].tobytes() == nrm.tobytes(), (what, "attributes")
        # the generator against its restatement, to that restatement's tolerance (tests/test_instanced_frame_gpu.py)
        srays = got["srays"].view(nt.RAY_DTYPE)
        sf = got["srays"].view(F).reshape(-1, 8)
        by_slot = out.copy()
        by_slot["id"] = np.where((out["id"] == -1) | (nrm[:, 3] == 0), -1, np.arange(n))
        ro, rd, rt2 = np_raygen.ao_rays(self.rays, by_slot, nrm[:, :3].copy(), self.ns, self.radius, self.ao_seed)
        live = rt2 > 0
        assert np.array_equal(sf[:, 7], rt2.astype(F)) and live.sum() == self.ns * (out["id"] >= 0).sum()
        assert np.abs(sf[live, :3] - ro[live]).max() < 1e-4 * max(1.0, np.abs(ro).max()) and np.abs(sf[live, 4:7] - rd[live]).max() < TOL
        assert np.array_equal(got["si2s"].view(np.int32), np.arange(m)) and np.array_equal(got["ss2i"].view(np.int32), np.arange(m))
        stimes = got["stimes"].view(F)
        assert stimes.tobytes() == mf.ray_times_secondary(times, 0, n, self.ns).tobytes(), (what, "secondary times")
        sid, st, su, sv, sinst, _ = ms.trace(srays, True, times=stimes)
        assert got["sres"].tobytes() == fc.records(sid, st, su, sv).tobytes() and got["sids"].tobytes() == sinst.astype(np.int32).tobytes(), (what, "secondary")
        src = np.repeat(ids, self.ns)
        return int(((sid >= 0) & (sinst == src) & (src == 0)).sum()), int((sid >= 0).sum())


def test_the_frame_has_no_self_hits_on_the_convex_cube():
    d = fc.demo()
    s = _Attr(d["ms"], d["tri"], d["pos"], d["blas_tris"])
    f = _Frame(s, d["rays"], d["s2i"], fc.DEMO_NS, fc.DEMO_RADIUS, fc.DEMO_AO_SEED)
    f.run(0)
    got = f.download()
    self_hits, occluded = f.assert_equals_specs(got, d["ms"], s.t.keys, d["s2i"], 0, "demonstration")
    print("%d of %d AO rays occluded, %d by the cube they started from" % (occluded, f.m, self_hits))
    assert self_hits == 0 and occluded > 0
    # today's pieces on the same records do hit the cube itself: key-0 normals, and secondary times all 0
    n, m = f.n, f.m
    for what, key0_normals, zero_times in (("key-0 normals", True, False), ("secondary times 0", False, True)):
        d_nrm, d_out = (_filled(16 * n), _filled(16 * n)) if key0_normals else (f.bufs["nrm"], f.bufs["out"])
        if key0_normals:
            nt.instanced_hit_attributes(n, f.bufs["res"].data_ptr(), f.bufs["ids"].data_ptr(), s.geom, d_out.data_ptr(), d_nrm.data_ptr())
        d_srays, d_a, d_b = _filled(32 * m), _filled(4 * m), _filled(4 * m)
        nt.raygen_ao_normals(d_srays.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), f.d_rays.data_ptr(), d_out.data_ptr(), d_nrm.data_ptr(), 0, n, f.ns,
                             f.radius, f.ao_seed)
        d_st = torch.zeros(m, dtype=torch.float32, device="cuda:0") if zero_times else f.bufs["stimes"]
        d_sres, d_sids = _filled(16 * m), _filled(4 * m)
        nt.trace_instanced_motion(*s.t.args(m, True, d_srays, d_sres, d_sids), vis=None,
                                  motion=nt.InstanceMotion(s.d.d_keys.data_ptr(), s.d.keys_bytes, d_st.data_ptr(), 0.0), timed=False)
        torch.cuda.synchronize()
        sid = _down(d_sres, 16 * m).view(nt.RESULT_DTYPE)["id"]
        sinst = _down(d_sids, 4 * m).view(np.int32)
        src = np.repeat(got["ids"].view(np.int32), f.ns)
        wrong = int(((sid >= 0) & (sinst == src) & (src == 0)).sum())
        print("%s: %d self hits" % (what, wrong))
        assert wrong > 0, what


def test_motion_refit_and_the_frame_as_one_graph():
    """ntr_tlas_motion_refit (asynchronous) and the six steps on one stream, a linear graph: an uncaptured pass first (it uploads the
    refit's table and reserves its scratch), then the capture, then replays after key 1 and the slot table were rewritten on the device;
    a replay equals the specs, and so the same calls made uncaptured."""
    d = fc.demo()
    ms0 = d["ms"]
    s = _Attr(ms0, d["tri"], d["pos"], d["blas_tris"])
    n = d["rays"].shape[0]
    f = _Frame(s, d["rays"], d["s2i"], 4, fc.DEMO_RADIUS, fc.DEMO_AO_SEED)
    rng = np.random.default_rng(8)
    other = ms0.inst1.copy()
    other["objectToWorld"][0] = isc.transform(isc.rotation(rng), 4.0, (1.0, -1.0, 1.0)).reshape(other["objectToWorld"][0].shape)
    tables = [d["s2i"], rng.permutation(n).astype(np.int32), d["s2i"]]
    keys1 = [ms0.inst1, other, ms0.inst0]          # the last: nothing moves
    st = torch.cuda.Stream()

    def frame(stream):
        s.d.refit(blocking=False, stream=stream)
        f.run(3, stream)

    def check(k, what):
        torch.cuda.synchronize()
        ms = mc.MotionScene(ms0.pool, ms0.inst0, keys1[k])
        s.d.assert_equals(s.d.spec(), None, what)
        got = f.download()
        f.assert_equals_specs(got, ms, ms.refit["motion_keys"], tables[k], 3, what)
        return got["nrm"].tobytes() + got["sres"].tobytes()

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)
    seen = [check(0, "uncaptured")]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    for rep, k in enumerate((1, 2, 0)):
        s.d.set_keys(ms0.inst0, keys1[k])
        f.d_s2i.copy_(up(tables[k]))
        s.d.reset()
        for b in f.bufs.values():
            b.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        seen.append(check(k, "graph replay %d" % rep))
    assert len(set(seen[:3])) == 3 and seen[3] == seen[0]
    del g
