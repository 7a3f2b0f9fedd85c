"""Motion-blurred frames over deforming BLASes on the device against the numpy rule (tests/np_instanced_deform_frame.py):
ntr_instanced_hit_attributes_deform equals hit_attributes_deform() in every word over records ntr_trace_instanced_deform wrote at
hashed times, at the ray counts around a wave and a workgroup, with per-ray times and the scalar, in place and with either output alone,
over waves made of the four lane classes and over hand-made records whose every index is out of range once; a whole frame at the C-ABI
has no self hits on the demonstration's deforming cube, step by step equal to the specs; the frame with the pool's batched motion refit
and the top-level refit replays as one linear graph.  Output buffers are prefilled with 0xAB and nothing beyond the extents may change."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_deform_cases as dc
import instanced_deform_frame_cases as dfc
import instanced_motion_cases as mc
import instanced_scenes as isc
import np_instanced as ni
import np_instanced_deform as nd
import np_instanced_frame as nf
import np_instanced_motion as mo
import np_instanced_motion_frame as mf
import np_raygen
from gpu_util import up
from np_instanced_deform_frame import hit_attributes_deform
from test_instanced_deform_gpu import _Dev, _dev
from test_motion_refit_batch_cpu import _shared

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


class _Attr:
    """A deforming scene on the device (tests/test_instanced_deform_gpu.py's _Dev: the pool with its key 1, two keys of the instances, the
    deform-refitted tree) with its meshes: the NtrInstancedGeometry over key 0's vertices, the NtrInstancedDeformGeometry over key 1's
    and the flag array the refit read, and the NtrInstanceMotion over the key buffer the refit wrote."""

    def __init__(self, d, poison=True):
        self.d, self.s = d, d.s
        self.tri, self.pos0, self.pos1, self.blas_tris = dfc.geometry_of(self.s, poison=poison)    # (a static BLAS's key 1: NaN)
        self.d_tri, self.d_pos0, self.d_pos1, self.d_bt = up(self.tri), up(self.pos0), up(self.pos1), up(self.blas_tris)
        self.geom = nt.InstancedGeometry(d.n, self.blas_tris.shape[0], self.tri.shape[0], self.pos0.shape[0], d.d_inst0.data_ptr(), self.d_bt.data_ptr(),
                                         self.d_tri.data_ptr(), self.d_pos0.data_ptr())
        self.deform = nt.InstancedDeformGeometry(self.d_pos1.data_ptr(), d.d_flags.data_ptr())
        self.keep = []

    def keys(self):
        return self.d.download()[2]

    def motion(self, times=None, time=0.0):
        d_t = up(np.asarray(times, F)) if times is not None else None
        self.keep = [d_t]
        return nt.InstanceMotion(self.d.d_keys.data_ptr(), self.d.keys_bytes, d_t.data_ptr() if d_t is not None else 0, time)

    def trace(self, rays, any_hit=False, times=None, time=0.0):
        """ntr_trace_instanced_deform -> (d_res, d_ids, host records, host ids)"""
        n = rays.shape[0]
        d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
        nt.trace_instanced_deform(*self.d.args(n, any_hit, d_rays, d_res, d_ids), vis=None, motion=self.motion(times, time), deform=self.d.deform,
                                  timed=False)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        return d_res, d_ids, _down(d_res, 16 * n, "records").view(nt.RESULT_DTYPE), _down(d_ids, 4 * n, "instance ids").view(np.int32)

    def spec(self, res, ids, times=None, time=0.0):
        return hit_attributes_deform(res, ids, self.s.inst0, self.blas_tris, self.tri, self.pos0, self.pos1, self.s.pool["deforming"],
                                     self.s.refit["motion_keys"], times=times, time=time)

    def attributes(self, n, d_res, d_ids, motion, out=True, normals=True, in_place=False, deform=True):
        d_out = d_res if in_place else (_filled(16 * n) if out else None)
        d_nrm = _filled(16 * n) if normals else None
        nt.instanced_hit_attributes_deform(n, d_res.data_ptr(), d_ids.data_ptr(), self.geom, motion, self.deform if deform else None,
                                           d_out.data_ptr() if d_out is not None else 0, d_nrm.data_ptr() if d_nrm is not None else 0)
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
        _cache[name] = _Attr(_dev(name))
    return _cache[name]


# ---- 1. the attributes of the posed triangle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dfc.SCENES)
def test_attributes_equal_spec_on_the_scenes(name):
    s = _scene(name)
    rays, times = dfc.rays_and_times()
    n = rays.shape[0]
    d_res, d_ids, res, ids = s.trace(rays, False, times=times)
    hit = res["id"] >= 0
    assert hit.sum() > n // 16
    assert s.keys().tobytes() == s.s.refit["motion_keys"].tobytes()
    want = s.check(res, ids, d_res, d_ids, name + " hashed times", times=times, forms=True)
    assert np.array_equal(want[0]["id"] >= 0, hit)
    at_key0 = mf.hit_attributes_motion(res, ids, s.s.inst0, s.blas_tris, s.tri, s.pos0, s.s.refit["motion_keys"], times=times)
    assert want[0].tobytes() == at_key0[0].tobytes()                                   # the ids are the motion call's
    on_deforming = hit & (s.s.pool["deforming"][s.s.inst0["blas"][np.where(hit, ids, 0)]] != 0)
    assert on_deforming.any() or name in ("three_static", "big")                       # (big's instances are small: its rays meet few)
    assert (want[1].tobytes() != at_key0[1].tobytes()) == bool(on_deforming.any())     # the normals are not, where something deforms
    # the scalar: the ends, the middle, the corner times; then the corner times per ray
    for t in (0.0, 1.0, 0.5):
        s.check(res, ids, d_res, d_ids, "%s t = %g" % (name, t), time=t)
    for t in dc.CORNER_TIMES:
        s.check(res, ids, d_res, d_ids, "%s scalar time %r" % (name, t), time=float(t) if t == t else float("nan"))
    s.check(res, ids, d_res, d_ids, name + " corner times per ray", times=np.resize(dc.CORNER_TIMES, n))
    # deform == NULL is ntr_instanced_hit_attributes_motion: the bytes of that call
    d_o0, d_n0 = _filled(16 * n), _filled(16 * n)
    nt.instanced_hit_attributes_motion(n, d_res.data_ptr(), d_ids.data_ptr(), s.geom, s.motion(times), d_o0.data_ptr(), d_n0.data_ptr())
    s.assert_equal(n, at_key0, d_o0, d_n0, "the motion call")
    s.assert_equal(n, at_key0, *s.attributes(n, d_res, d_ids, s.motion(times), deform=False), "deform == NULL")
    # any-hit records resolve alike
    d_res, d_ids, res, ids = s.trace(rays, True, times=times)
    s.check(res, ids, d_res, d_ids, name + " any hit", times=times)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_ray_counts(n):
    s = _scene("three")
    rays, times = dfc.rays_and_times()
    if "first" not in _cache:      # a single ray is a hit on the deforming BLAS
        _, _, res, ids = s.trace(rays, False, times=times)
        _cache["first"] = int(np.flatnonzero((res["id"] >= 0) & (ids == 1) & (times > 0.1) & (times < 0.9))[0])
    k = _cache["first"]
    rays, times = np.roll(rays, -k)[:n], np.roll(times, -k)[:n].copy()
    d_res, d_ids, res, ids = s.trace(rays, False, times=times)
    want = s.check(res, ids, d_res, d_ids, "%d rays" % n, times=times, forms=True)
    assert want[0]["id"][0] >= 0 and want[1][0, 3] == 1 and s.s.pool["deforming"][s.s.inst0["blas"][ids[0]]] != 0
    s.check(res, ids, d_res, d_ids, "%d rays, scalar" % n, time=0.3)


# ---- 2. hand-made records -------------------------------------------------------------------------------------------------------------------------
class _Synthetic:
    """Instances of its own over `three`'s meshes (BLAS 1 deforms), uploaded without a tree: the call takes records, not a trace.  Every
    buffer the kernel reads stands between guard bytes; the flag array's neighbours say "deforming", and key 1 of every static BLAS is
    NaN, so a flag or a vertex read outside the rule would change a normal."""

    def __init__(self, inst0, inst1, flags, tri=None, pos0=None, pos1=None, bt=None):
        g = dfc.geometry_of(dc.named("three"), poison=True)
        self.tri, self.pos0, self.pos1, self.bt = (tri if tri is not None else g[0]), (pos0 if pos0 is not None else g[1]), \
            (pos1 if pos1 is not None else g[2]), (bt if bt is not None else g[3])
        self.inst0, self.flags = inst0, np.asarray(flags, U)
        self.keys = mo.motion_keys(inst0, inst1)
        self.num_inst = inst0.shape[0]
        assert self.flags.shape[0] == self.bt.shape[0]
        self.d_inst, self.d_keys, self.d_tri, self.d_pos0, self.d_pos1, self.d_bt = (up(a) for a in (inst0, self.keys, self.tri, self.pos0, self.pos1, self.bt))
        self.d_flags = up(np.concatenate([np.ones(4, U), self.flags, np.ones(4, U)]))
        self.geom = nt.InstancedGeometry(self.num_inst, self.bt.shape[0], self.tri.shape[0], self.pos0.shape[0], self.d_inst.data_ptr(), self.d_bt.data_ptr(),
                                         self.d_tri.data_ptr(), self.d_pos0.data_ptr())
        self.deform = nt.InstancedDeformGeometry(self.d_pos1.data_ptr(), self.d_flags.data_ptr() + 16)

    def spec(self, res, ids, times):
        return hit_attributes_deform(res, ids, self.inst0, self.bt, self.tri, self.pos0, self.pos1, self.flags, self.keys, times=times)

    def run(self, res, ids, times, in_place=False):
        """-> (records, normals) as bytes; the outputs stand between 64 guard bytes on either side"""
        n = res.shape[0]
        d_res, d_ids, d_t = torch.full((64 + 16 * n + 64,), 0xAB, dtype=torch.uint8, device="cuda:0"), up(ids), up(times)
        d_res[64:64 + 16 * n] = up(res)
        d_out = d_res if in_place else torch.full((64 + 16 * n + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_nrm = torch.full((64 + 16 * n + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
        motion = nt.InstanceMotion(self.d_keys.data_ptr(), 128 * self.num_inst, d_t.data_ptr(), 0.0)
        nt.instanced_hit_attributes_deform(n, d_res.data_ptr() + 64, d_ids.data_ptr(), self.geom, motion, self.deform, d_out.data_ptr() + 64,
                                           d_nrm.data_ptr() + 64)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        got = []
        for b in (d_out, d_nrm):
            raw = b.cpu().numpy()
            assert (raw[:64] == 0xAB).all() and (raw[64 + 16 * n:] == 0xAB).all(), "a word outside the outputs was written"
            got.append(raw[64:64 + 16 * n].tobytes())
        if not in_place:
            assert d_res.cpu().numpy()[64:64 + 16 * n].tobytes() == res.tobytes(), "the input records changed"
        for buf, a in ((self.d_inst, self.inst0), (self.d_keys, self.keys), (self.d_tri, self.tri), (self.d_pos0, self.pos0), (self.d_bt, self.bt)):
            assert buf.cpu().numpy().tobytes() == a.tobytes(), "an input changed"
        return got


def test_waves_of_the_four_lane_classes():
    """Static instance / static BLAS, moving / static, static / deforming, moving / deforming: one wave of 64 uniform in each class, then
    one that mixes all four: both sides of both votes, and a wave in which the lanes part twice."""
    sc = isc.scene("three")
    tf0 = np.stack([sc["transforms"][0], sc["transforms"][0], sc["transforms"][1], sc["transforms"][1]])
    tf1 = tf0.copy()
    rng = np.random.default_rng(21)
    tf1[1] = isc.transform(isc.rotation(rng), 0.03, (-7.0, -8.5, -6.0))
    tf1[3] = isc.transform(isc.rotation(rng), (1.0, 0.8, 1.1), (1.0, 0.5, 0.0))
    which = [0, 0, 1, 1]
    inst0, inst1 = ni.instances(tf0, which), ni.instances(tf1, which)
    assert mo.moving(inst0, inst1).tolist() == [False, True, False, True]
    s = _Synthetic(inst0, inst1, [0, 1, 0])
    n = 320
    ids = np.concatenate([np.full(64, c) for c in range(4)] + [np.arange(64) % 4]).astype(np.int32)       # the instance is the class
    res = np.zeros(n, nt.RESULT_DTYPE)
    res["id"] = (np.arange(n) * 7) % s.bt[inst0["blas"][ids], 1]
    res["t"] = F(1.0)
    times = mf.ray_times_primary(n, None, 6, 0.125, 0.875)
    want = s.spec(res, ids, times)
    assert (want[0]["id"] >= 0).all() and (want[1][:, 3] == 1).all()
    for in_place in (False, True):
        got = s.run(res, ids, times, in_place)
        assert got[0] == want[0].tobytes() and got[1] == want[1].view(U).tobytes(), in_place
    # ntr_instanced_hit_attributes' own bytes on the static / static lanes, and on no other
    d_res, d_ids, d_n0 = up(res), up(ids), _filled(16 * n)
    nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), s.geom, 0, d_n0.data_ptr())
    torch.cuda.synchronize()
    today = _down(d_n0, 16 * n).view(U).reshape(-1, 4)
    assert today.tobytes() == nf.hit_attributes(res, ids, inst0, s.bt, s.tri, s.pos0)[1].view(U).tobytes()
    same = (np.frombuffer(got[1], U).reshape(-1, 4) == today).all(axis=1)
    assert same[ids == 0].all() and not same[ids != 0].any(), [int(same[ids == c].sum()) for c in range(4)]


def test_hostile_records_never_read_outside_the_buffers():
    """tests/test_instanced_motion_frame_gpu.py's hand-made batch over a pool in which BLAS 1 deforms: one ray per way an index can be out
    of range, between good rays of the four classes; every outcome is the rule's, and nothing but the outputs changes."""
    tri, pos0, pos1, bt = dfc.geometry_of(dc.named("three"), poison=True)
    nv0, nt0 = pos0.shape[0], tri.shape[0]
    tiny = np.array([(0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0)], F)
    pos0 = np.concatenate([pos0, tiny]).astype(F)
    pos1 = np.concatenate([pos1, tiny[::-1]]).astype(F)
    nv = pos0.shape[0]
    special = np.array([(nv, 0, 1), (0, -1, 1), (nv0, nv0 + 1, nv0 + 2)], np.int32)
    tri = np.concatenate([tri, special]).astype(np.int32)
    bt = np.concatenate([bt, [(nt0, 3), (0, 0)]]).astype(np.int32)            # BLAS 3: the special triangles (deforming); BLAS 4: numTris 0
    num_blas = bt.shape[0]
    flags = [0, 1, 0, 1, 1]
    tf = isc.seeded_transforms(8, 77, mirrored=2)
    which = [0, 1, 2, 3, 4, 0, 0, 1]
    inst0, inst1 = ni.instances(tf, which), ni.instances(mc.key1_transforms(tf), which)      # 2 and 5 stand still
    for inst in (inst0, inst1):
        inst["blas"][5], inst["blas"][6] = -1, num_blas
    inst1["objectToWorld"][7] = inst0["objectToWorld"][7]                                    # 7: a static instance of the deforming BLAS
    assert mo.moving(inst0, inst1).tolist() == [True, True, False, True, True, False, True, False]
    num_inst = inst0.shape[0]
    s = _Synthetic(inst0, inst1, flags, tri, pos0, pos1, bt)
    cases = [                                  # (what, id, instance)
        ("a good ray", 3, 0), ("a miss", -1, -1), ("a miss with an instance", -1, 1), ("instance -1 with id >= 0", 5, -1),
        ("instance == numInstances", 5, num_inst), ("instance INT_MAX", 5, INT_MAX), ("instance INT_MIN", 5, -INT_MAX - 1),
        ("blas -1", 0, 5), ("blas == numBlas", 0, 6), ("id == numTris", int(bt[0, 1]), 0), ("id == numTris - 1", int(bt[0, 1]) - 1, 0),
        ("id == numTris of the soup", int(bt[1, 1]), 7), ("id -2", -2, 0), ("id INT_MAX", INT_MAX, 1), ("id INT_MIN", -INT_MAX - 1, 1),
        ("a vertex index == numVerts", 0, 3), ("a vertex index -1", 1, 3), ("edges of 1e-20", 2, 3), ("a BLAS of no triangles", 0, 4),
        ("the single triangle, static", 0, 2), ("a good ray of the soup, static instance", 999, 7), ("a good ray of the soup, moving instance", 7, 1)]
    n = len(cases)
    res = np.zeros(n, nt.RESULT_DTYPE)
    res["id"] = [c[1] for c in cases]
    res["t"] = np.linspace(0.5, 9.5, n).astype(F)
    res["padA"], res["padB"] = np.arange(n) + 0x3e000000, np.arange(n) + 0x3f000000
    ids = np.array([c[2] for c in cases], np.int32)
    times = mf.ray_times_primary(n, None, 4)
    want_out, want_nrm = s.spec(res, ids, times)
    what = [c[0] for c in cases]
    resolved = {"a good ray", "id == numTris - 1", "edges of 1e-20", "the single triangle, static", "a good ray of the soup, static instance",
                "a good ray of the soup, moving instance"}
    assert {w for w, o in zip(what, want_out["id"]) if o >= 0} == resolved
    assert {w for w, m in zip(what, want_nrm[:, 3]) if m == 1} == resolved - {"edges of 1e-20"}
    assert not np.isnan(want_nrm).any()
    today = mf.hit_attributes_motion(res, ids, inst0, bt, tri, pos0, s.keys, times=times)[1]
    differs = {w for w, a, b in zip(what, want_nrm, today) if a.tobytes() != b.tobytes()}
    assert differs == {"a good ray of the soup, static instance", "a good ray of the soup, moving instance"}
    for in_place in (False, True):
        got = s.run(res, ids, times, in_place)
        assert got[0] == want_out.tobytes() and got[1] == want_nrm.view(U).tobytes(), in_place
    assert nt.trace_status() == 0


# ---- 3. the frame at the C-ABI ----------------------------------------------------------------------------------------------------------------
class _Frame:
    """The demonstration's frame: times -> deform trace -> attributes of the posed triangle -> ntr_raygen_ao_normals -> secondary times ->
    any-hit deform trace, over one _Attr; every call on `stream`."""

    def __init__(self, s, rays, s2i, ns, radius, ao_seed):
        self.s, self.rays, self.n, self.ns, self.radius, self.ao_seed = s, rays, rays.shape[0], ns, radius, ao_seed
        n, m = self.n, self.n * ns
        self.m = m
        self.d_rays, self.d_s2i = up(rays), up(s2i)
        self.bufs = dict(times=_filled(4 * n), res=_filled(16 * n), ids=_filled(4 * n), out=_filled(16 * n), nrm=_filled(16 * n), srays=_filled(32 * m),
                         si2s=_filled(4 * m), ss2i=_filled(4 * m), stimes=_filled(4 * m), sres=_filled(16 * m), sids=_filled(4 * m))

    def run(self, seed, stream=0):
        s, d, b, n, m = self.s, self.s.d, self.bufs, self.n, self.m
        p = {k: v.data_ptr() for k, v in b.items()}
        nt.ray_times_primary(n, self.d_s2i.data_ptr(), seed, 0.0, 1.0, p["times"], stream)
        pm = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, p["times"], 0.0)
        nt.trace_instanced_deform(*d.args(n, False, self.d_rays, b["res"], b["ids"]), vis=None, motion=pm, deform=d.deform, stream=stream, timed=False)
        nt.instanced_hit_attributes_deform(n, p["res"], p["ids"], s.geom, pm, s.deform, p["out"], p["nrm"], stream)
        nt.raygen_ao_normals(p["srays"], p["si2s"], p["ss2i"], self.d_rays.data_ptr(), p["out"], p["nrm"], 0, n, self.ns, self.radius, self.ao_seed, stream)
        nt.ray_times_secondary(p["times"], 0, n, self.ns, p["stimes"], stream)
        sm = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, p["stimes"], 0.0)
        nt.trace_instanced_deform(*d.args(m, True, b["srays"], b["sres"], b["sids"]), vis=None, motion=sm, deform=d.deform, stream=stream, timed=False)

    def download(self):
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        sizes = dict(times=4, res=16, ids=4, out=16, nrm=16)
        return {k: _down(v, (sizes[k] * self.n) if k in sizes else {"srays": 32, "si2s": 4, "ss2i": 4, "stimes": 4, "sres": 16, "sids": 4}[k] * self.m, k)
                for k, v in self.bufs.items()}

    def assert_equals_specs(self, got, trace, attributes, s2i, seed, what):
        """Each device step against its spec, fed with the device's own inputs of that step; trace(rays, any_hit, times) and
        attributes(res, ids, times) are the rule over the scene's current state -> (self hits on instance 0, occluded AO rays)"""
        n, m = self.n, self.m
        times = got["times"].view(F)
        assert times.tobytes() == mf.ray_times_primary(n, s2i, seed).tobytes(), (what, "times")
        rid, rt, ru, rv, rinst, _ = trace(self.rays, False, times)
        res, ids = dfc.records(rid, rt, ru, rv), rinst.astype(np.int32)
        assert got["res"].tobytes() == res.tobytes() and got["ids"].tobytes() == ids.tobytes(), (what, "primary records")
        out, nrm = attributes(res, ids, times)
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
        sid, st, su, sv, sinst, _ = trace(srays, True, stimes)
        assert got["sres"].tobytes() == dfc.records(sid, st, su, sv).tobytes() and got["sids"].tobytes() == sinst.astype(np.int32).tobytes(), (what, "secondary")
        src = np.repeat(ids, self.ns)
        return int(((sid >= 0) & (sinst == src) & (src == 0)).sum()), int((sid >= 0).sum())


def _rules(scene, d, a, flags, pos1):
    """The two rules over a scene's state: the pool's flags replaced by `flags`, the top-level tree the device's own build, refitted by
    the rule -> (the refit's outputs, trace(rays, any_hit, times), attributes(res, ids, times))"""
    pool = dict(scene.pool, deforming=np.asarray(flags, U))
    want = nd.deform_refit(d.built_nodes, d.root, d.built_records, pool["nodes"], pool["nodes1"], scene.ranges, pool["deforming"], scene.inst0,
                           scene.inst1)

    def trace(rays, any_hit, times):
        return nd.trace(want["nodes"], d.root, want["records"], want["motion_keys"], pool, rays, any_hit, times=times)

    def attributes(res, ids, times):
        return hit_attributes_deform(res, ids, scene.inst0, a.blas_tris, a.tri, a.pos0, pos1, pool["deforming"], want["motion_keys"], times=times)
    return want, trace, attributes


def test_the_frame_has_no_self_hits_on_the_deforming_cube():
    demo = dfc.demo()
    d = _Dev(demo["s"])
    d.refit()
    a = _Attr(d)
    f = _Frame(a, demo["rays"], demo["s2i"], dfc.DEMO_NS, dfc.DEMO_RADIUS, dfc.DEMO_AO_SEED)
    f.run(0)
    got = f.download()
    _, trace, attributes = _rules(demo["s"], d, a, demo["deforming"], demo["pos1"])
    self_hits, occluded = f.assert_equals_specs(got, trace, attributes, demo["s2i"], 0, "demonstration")
    print("%d of %d AO rays occluded, %d by the cube they started from" % (occluded, f.m, self_hits))
    assert self_hits == 0 and occluded > 0
    # today's pieces on the same records do hit the cube itself: key-0 normals, and secondary times all 0
    n, m = f.n, f.m
    pm = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, f.bufs["times"].data_ptr(), 0.0)
    for what, key0_normals, zero_times in (("key-0 normals", True, False), ("secondary times 0", False, True)):
        d_nrm, d_out = (_filled(16 * n), _filled(16 * n)) if key0_normals else (f.bufs["nrm"], f.bufs["out"])
        if key0_normals:
            nt.instanced_hit_attributes_motion(n, f.bufs["res"].data_ptr(), f.bufs["ids"].data_ptr(), a.geom, pm, d_out.data_ptr(), d_nrm.data_ptr())
        d_srays, d_a, d_b = _filled(32 * m), _filled(4 * m), _filled(4 * m)
        nt.raygen_ao_normals(d_srays.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), f.d_rays.data_ptr(), d_out.data_ptr(), d_nrm.data_ptr(), 0, n, f.ns,
                             f.radius, f.ao_seed)
        d_st = torch.zeros(m, dtype=torch.float32, device="cuda:0") if zero_times else f.bufs["stimes"]
        d_sres, d_sids = _filled(16 * m), _filled(4 * m)
        nt.trace_instanced_deform(*d.args(m, True, d_srays, d_sres, d_sids), vis=None,
                                  motion=nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, d_st.data_ptr(), 0.0), deform=d.deform, timed=False)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        sid = _down(d_sres, 16 * m).view(nt.RESULT_DTYPE)["id"]
        sinst = _down(d_sids, 4 * m).view(np.int32)
        src = np.repeat(got["ids"].view(np.int32), f.ns)
        wrong = int(((sid >= 0) & (sinst == src) & (src == 0)).sum())
        print("%s: %d self hits" % (what, wrong))
        assert wrong > 0, what


def test_pool_refit_top_level_refit_and_the_frame_as_one_graph():
    """ntr_bvh_motion_refit_batch and ntr_tlas_deform_refit (both asynchronous) and the six steps on one stream, a linear graph: an
    uncaptured pass first (it uploads the refits' tables and reserves their scratch), then the capture, then replays after key 1 of the
    vertices, the flag array and the slot table were rewritten on the device; a replay equals the specs, and so the same calls made
    uncaptured."""
    demo = dfc.demo()
    s0 = demo["s"]
    d = _Dev(s0)
    a = _Attr(d, poison=False)          # the batch refit reads both vertex arrays whole: the attributes call shares them
    tri, pos0, pos1, entries = _shared(s0)
    assert tri.tobytes() == a.tri.tobytes() and pos0.tobytes() == a.pos0.tobytes() and pos1.tobytes() == a.pos1.tobytes()
    n = demo["rays"].shape[0]
    f = _Frame(a, demo["rays"], demo["s2i"], 4, dfc.DEMO_RADIUS, dfc.DEMO_AO_SEED)
    rng = np.random.default_rng(8)
    other = pos1.copy()
    nv = dfc.CUBE_POS.shape[0]
    other[:nv] = (dfc.CUBE_POS.astype(np.float64) @ (isc.rotation(rng) @ np.diag([1.3, 0.8, 1.1])).T + np.array([-0.2, 0.0, 0.2])).astype(F)
    # (the state a replay sees: key 1 of the vertices, the flags, the slot table)
    states = [(pos1, [1, 0], demo["s2i"]), (other, [1, 0], rng.permutation(n).astype(np.int32)), (other, [0, 0], demo["s2i"])]
    st = torch.cuda.Stream()

    def frame(stream):
        assert nt.bvh_motion_refit_batch(entries, d.d_nodes.data_ptr(), d.nb, d.d_nodes1.data_ptr(), d.d_woop.data_ptr(), d.wb, d.d_idx.data_ptr(),
                                         d.d_v0.data_ptr(), d.d_v1.data_ptr(), tri.shape[0], a.d_tri.data_ptr(), pos0.shape[0], a.d_pos0.data_ptr(),
                                         a.d_pos1.data_ptr(), 0, stream=stream, blocking=False) is None
        d.refit(blocking=False, stream=stream)
        f.run(3, stream)

    def check(k, what):
        torch.cuda.synchronize()
        p1, flags, table = states[k]
        scene = dc.DeformScene(s0.names, s0.inst0, s0.inst1, {0: (pos0[:nv], p1[:nv])})
        for name, buf in (("nodes", d.d_nodes), ("woop", d.d_woop), ("nodes1", d.d_nodes1), ("vrows0", d.d_v0), ("vrows1", d.d_v1)):
            assert buf.cpu().numpy()[:scene.pool[name].size].tobytes() == scene.pool[name].tobytes(), ("the pool's " + name, what)
        want, trace, attributes = _rules(scene, d, a, flags, p1)
        d.assert_equals(want, None, what)
        got = f.download()
        f.assert_equals_specs(got, trace, attributes, table, 3, what)
        return got["nrm"].tobytes() + got["sres"].tobytes()

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)
    seen = [check(0, "uncaptured")]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    for rep, k in enumerate((1, 2, 0)):
        p1, flags, table = states[k]
        a.d_pos1.copy_(up(p1))
        d.d_flags.copy_(up(np.asarray(flags, U)))
        f.d_s2i.copy_(up(table))
        d.reset()
        for b in f.bufs.values():
            b.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        seen.append(check(k, "graph replay %d" % rep))
    assert len(set(seen[:3])) == 3 and seen[3] == seen[0]
    del g
