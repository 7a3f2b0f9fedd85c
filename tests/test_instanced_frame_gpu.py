"""Instanced frames on the device: ntr_instanced_hit_attributes equals the numpy rule (tests/np_instanced_frame.py) in every word --
ids, t, pads and the four normal words as uint32 -- over traced scenes, at the ray counts around a workgroup, in place and with either
output alone, and over hand-made records whose every index is out of range once; ntr_raygen_ao_normals equals ntr_raygen_ao bit for
bit when handed the table's normals per ray; a whole frame (primary -> two-level trace -> attributes -> AO / diffuse rays -> two-level
trace -> ntr_reconstruct) equals the specs with no tolerance reaching a hit; the frame replays as one graph.  Output buffers are
prefilled with 0xAB and nothing beyond the extents may change."""
import types

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_frame as nf
import np_raygen
import np_rayops
from gpu_util import DeviceBvh, gpu_trace, up
from test_instanced_frame_cpu import geometry

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 64
TOL = 1e-5
INT_MAX = 2 ** 31 - 1
_cache = {}


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


def _down(buf, nbytes, what=""):
    raw = buf.cpu().numpy()
    assert (raw[nbytes:] == 0xAB).all(), "bytes beyond the extents were written: " + what
    return raw[:nbytes].copy()


class _Geom:
    """The meshes of a pool and its instances on the device, and the NtrInstancedGeometry over them."""

    def __init__(self, tri, pos, blas_tris, inst):
        self.tri, self.pos, self.blas_tris, self.inst = tri, pos, np.asarray(blas_tris, np.int32).reshape(-1, 2), inst
        self.d_tri, self.d_pos, self.d_bt, self.d_inst = up(tri), up(pos), up(self.blas_tris), up(inst)
        self.geom = nt.InstancedGeometry(inst.shape[0], self.blas_tris.shape[0], tri.shape[0], pos.shape[0], self.d_inst.data_ptr(),
                                         self.d_bt.data_ptr(), self.d_tri.data_ptr(), self.d_pos.data_ptr())

    def set_instances(self, inst):
        self.inst = inst
        self.d_inst.copy_(up(inst))

    def spec(self, res, ids):
        return nf.hit_attributes(res, ids, self.inst, self.blas_tris, self.tri, self.pos)

    def attributes(self, n, d_res, d_ids, out=True, normals=True, in_place=False, stream=0):
        """-> (d_out or None, d_nrm or None), 0xAB-bordered; in_place writes the records over d_res"""
        d_out = d_res if in_place else (_filled(16 * n) if out else None)
        d_nrm = _filled(16 * n) if normals else None
        nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), self.geom, d_out.data_ptr() if d_out is not None else 0,
                                    d_nrm.data_ptr() if d_nrm is not None else 0, stream)
        return d_out, d_nrm

    def assert_equals_spec(self, n, res, ids, d_out, d_nrm, what):
        """res, ids: the host copies of the input records; the device outputs equal the rule in every word"""
        torch.cuda.synchronize()
        want_out, want_nrm = self.spec(res[:n], ids[:n])
        if d_out is not None:
            got = _down(d_out, 16 * n, str(what)).view(np.uint32).reshape(-1, 4)
            bad = np.flatnonzero((got != want_out.view(np.uint32).reshape(-1, 4)).any(axis=1))
            assert bad.size == 0, ("records differ", what, int(bad[0]), got[bad[0]], want_out[bad[0]])
        if d_nrm is not None:
            got = _down(d_nrm, 16 * n, str(what)).view(np.uint32).reshape(-1, 4)
            bad = np.flatnonzero((got != want_nrm.view(np.uint32).reshape(-1, 4)).any(axis=1))
            assert bad.size == 0, ("normals differ", what, int(bad[0]), got[bad[0]].view(F), want_nrm[bad[0]])
        return want_out, want_nrm


class _Scene:
    """A named scene of instanced_scenes on the device: pool, device-built top-level tree, geometry."""

    def __init__(self, name):
        sc = isc.scene(name)
        self.pool = isc.pool_of(sc["names"])
        self.inst = ni.instances(sc["transforms"], sc["blas"])
        self.n = self.inst.shape[0]
        self.d_nodes, self.d_woop, self.d_idx = up(self.pool["nodes"]), up(self.pool["woop"]), up(self.pool["tri_index"])
        self.g = _Geom(*geometry(sc["names"]), self.inst)
        caps = nt.tlas_capacity(self.n)
        self.d_tlas, self.d_rec = _filled(caps[0]), _filled(caps[1])
        self.res = nt.tlas_build(self.n, self.g.d_inst.data_ptr(), self.pool["ranges"], self.d_nodes.data_ptr(), self.pool["nodes"].size,
                                 self.d_tlas.data_ptr(), caps[0], self.d_rec.data_ptr(), caps[1])
        torch.cuda.synchronize()
        self.tlas = self.d_tlas.cpu().numpy()[:self.res.nodesBytes].view(np.int32).reshape(-1, 16).copy()
        self.records = self.d_rec.cpu().numpy()[:self.res.recordsBytes].view(np.uint32).reshape(-1, 16).copy()

    def trace(self, n, d_rays, any_hit, stream=0):
        d_res, d_ids = _filled(16 * n), _filled(4 * n)
        nt.trace_instanced(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), self.d_tlas.data_ptr(), self.res.nodesBytes,
                           self.res.rootLink, self.d_rec.data_ptr(), self.n, self.d_nodes.data_ptr(), self.pool["nodes"].size,
                           self.d_woop.data_ptr(), self.pool["woop"].size, self.d_idx.data_ptr(), stream=stream, timed=False)
        return d_res, d_ids

    def spec_trace(self, rays, any_hit):
        return _spec_records(ni.trace(self.tlas, self.res.rootLink, self.records, self.pool, rays, any_hit))


def _spec_records(traced):
    rid, rt, ru, rv, rinst = traced
    res = np.zeros(rid.shape[0], nt.RESULT_DTYPE)
    res["id"], res["t"], res["padA"], res["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return res, rinst.astype(np.int32)


def _named(name):
    if name not in _cache:
        _cache[name] = _Scene(name)
    return _cache[name]


def _host(d_res, d_ids, n):
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    return _down(d_res, 16 * n, "trace records").view(nt.RESULT_DTYPE), _down(d_ids, 4 * n, "trace instance ids").view(np.int32)


# ---- 1. attributes equal the spec in every word ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_attributes_equal_spec_on_the_scenes(name):
    s = _named(name)
    rays = isc.scene_rays(primary=(64, 32), random=2048)
    n = rays.shape[0]
    d_rays = up(rays)
    for any_hit in (False, True):
        d_res, d_ids = s.trace(n, d_rays, any_hit)
        res, ids = _host(d_res, d_ids, n)
        assert (res["id"] >= 0).sum() > n // 8
        d_out, d_nrm = s.g.attributes(n, d_res, d_ids)
        want_out, want_nrm = s.g.assert_equals_spec(n, res, ids, d_out, d_nrm, (name, any_hit))
        assert np.array_equal(want_out["id"] >= 0, res["id"] >= 0) and np.array_equal(want_nrm[:, 3] == 1, res["id"] >= 0)
        assert _down(d_res, 16 * n).tobytes() == res.tobytes(), "the input records changed"
        # each output alone, then in place
        d_out, _ = s.g.attributes(n, d_res, d_ids, normals=False)
        s.g.assert_equals_spec(n, res, ids, d_out, None, (name, any_hit, "records alone"))
        _, d_nrm = s.g.attributes(n, d_res, d_ids, out=False)
        s.g.assert_equals_spec(n, res, ids, None, d_nrm, (name, any_hit, "normals alone"))
        d_out, d_nrm = s.g.attributes(n, d_res, d_ids, in_place=True)
        assert d_out is d_res
        s.g.assert_equals_spec(n, res, ids, d_out, d_nrm, (name, any_hit, "in place"))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 + 2048])
def test_ray_counts(n):
    s = _named("three")
    rays = isc.scene_rays(primary=(64, 32), random=4096)
    assert rays.shape[0] == 4096 + 2048
    if "first hit" not in _cache:
        d_res, d_ids = s.trace(rays.shape[0], up(rays), False)
        _cache["first hit"] = int(np.flatnonzero(_host(d_res, d_ids, rays.shape[0])[0]["id"] >= 0)[0])
    rays = np.roll(rays, -_cache["first hit"])[:n]        # a single ray is a hit
    d_rays = up(rays)
    d_res, d_ids = s.trace(n, d_rays, False)
    res, ids = _host(d_res, d_ids, n)
    d_out, d_nrm = s.g.attributes(n, d_res, d_ids)
    want_out, _ = s.g.assert_equals_spec(n, res, ids, d_out, d_nrm, n)
    assert want_out["id"][0] >= 0
    d_out, d_nrm = s.g.attributes(n, d_res, d_ids, in_place=True)
    s.g.assert_equals_spec(n, res, ids, d_out, d_nrm, (n, "in place"))


# ---- 2. synthetic records -----------------------------------------------------------------------------------------------------------------
def test_synthetic_records_never_read_outside_the_buffers():
    """Records made by hand over the meshes of ["cornell", "soup1000", "one"] plus a fourth BLAS of three special triangles and a fifth
    of none; no trace.  One ray per way an index can be out of range, between good rays; every outcome is the rule's."""
    tri, pos, bt = geometry(["cornell", "soup1000", "one"])
    nv0, nt0 = pos.shape[0], tri.shape[0]
    # three vertices whose edges are 1e-20 long: the cross product is subnormal and l2 underflows to 0
    tiny = np.array([(0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0)], F)
    pos = np.concatenate([pos, tiny]).astype(F)
    nv = pos.shape[0]
    special = np.array([(nv, 0, 1), (0, -1, 1), (nv0, nv0 + 1, nv0 + 2)], np.int32)
    tri = np.concatenate([tri, special]).astype(np.int32)
    bt = np.concatenate([bt, [(nt0, 3), (0, 0)]]).astype(np.int32)            # BLAS 3: the special triangles; BLAS 4: numTris 0
    num_blas = bt.shape[0]
    tf = isc.seeded_transforms(8, 77, mirrored=2)
    inst = ni.instances(tf, [0, 1, 2, 3, 4, 0, 0, 1])
    inst["blas"][5], inst["blas"][6] = -1, num_blas
    g = _Geom(tri, pos, bt, inst)
    num_inst = inst.shape[0]
    cases = [                                  # (what, id, instance)
        ("a good ray", 3, 0), ("a miss", -1, -1), ("a miss with an instance", -1, 1), ("instance -1 with id >= 0", 5, -1),
        ("instance == numInstances", 5, num_inst), ("instance INT_MAX", 5, INT_MAX), ("instance INT_MIN", 5, -INT_MAX - 1),
        ("blas -1", 0, 5), ("blas == numBlas", 0, 6), ("id == numTris", int(bt[0, 1]), 0), ("id == numTris - 1", int(bt[0, 1]) - 1, 0),
        ("id == numTris of the soup", int(bt[1, 1]), 7), ("id -2", -2, 0), ("id INT_MAX", INT_MAX, 1), ("id INT_MIN", -INT_MAX - 1, 1),
        ("a vertex index == numVerts", 0, 3), ("a vertex index -1", 1, 3), ("edges of 1e-20", 2, 3), ("a BLAS of no triangles", 0, 4),
        ("the single triangle", 0, 2), ("a good ray of the soup", 999, 7)]
    n = len(cases)
    res = np.zeros(n, nt.RESULT_DTYPE)
    res["id"] = [c[1] for c in cases]
    res["t"] = np.linspace(0.5, 9.5, n).astype(F)
    res["padA"], res["padB"] = np.arange(n) + 0x3e000000, np.arange(n) + 0x3f000000
    ids = np.array([c[2] for c in cases], np.int32)
    want_out, want_nrm = g.spec(res, ids)
    what = [c[0] for c in cases]
    resolved = {"a good ray", "id == numTris - 1", "edges of 1e-20", "the single triangle", "a good ray of the soup"}
    assert {w for w, o in zip(what, want_out["id"]) if o >= 0} == resolved
    assert {w for w, m in zip(what, want_nrm[:, 3]) if m == 1} == resolved - {"edges of 1e-20"}
    assert want_out["id"][what.index("edges of 1e-20")] == nt0 + 2 and want_out["id"][what.index("a good ray of the soup")] == bt[1, 0] + 999
    d_res, d_ids = _filled(16 * n), _filled(4 * n)
    d_res[:16 * n] = up(res)
    d_ids[:4 * n] = up(ids)
    d_out, d_nrm = g.attributes(n, d_res, d_ids)
    g.assert_equals_spec(n, res, ids, d_out, d_nrm, "synthetic")
    d_out, d_nrm = g.attributes(n, d_res, d_ids, in_place=True)
    g.assert_equals_spec(n, res, ids, d_out, d_nrm, "synthetic, in place")
    assert nt.trace_status() == 0


# ---- 3. ntr_raygen_ao_normals against the existing generator ------------------------------------------------------------------------------------
def _cornell_batch():
    """Primary rays and closest-hit records of the Cornell box (some inputs made misses), its triangle normals and those per ray"""
    if "cornell" not in _cache:
        tri, pos, cam = scenes.cornell_box()
        dbvh = DeviceBvh(nt.sah_build(tri, pos))
        rays, _ = scenes.primary_rays(cam, 64, 48)
        res, _ = gpu_trace("fermi_speculative_while_while", dbvh, rays, False)
        res = res.copy()
        res["id"][7::11] = -1
        assert (res["id"] >= 0).sum() > rays.shape[0] // 2
        tn = scenes.tri_normals(tri, pos)
        per_ray = np.zeros((rays.shape[0], 4), F)
        per_ray[:, :3] = tn[np.maximum(res["id"], 0)]
        per_ray[:, 3] = 1.0
        _cache["cornell"] = (rays, res, tn, per_ray, cam)
    return _cache["cornell"]


def _ao(fn, d_rays, d_res, d_nrm, first, count, ns, max_dist, seed):
    n = count * ns
    bufs = _filled(32 * n), _filled(4 * n), _filled(4 * n)
    fn(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), first, count, ns,
       max_dist, seed)
    torch.cuda.synchronize()
    return [_down(b, e * n, fn.__name__) for b, e in zip(bufs, (32, 4, 4))]


def test_ao_normals_equal_raygen_ao_bit_for_bit():
    rays, res, tn, per_ray, cam = _cornell_batch()
    n = rays.shape[0]
    d_rays, d_res, d_tn, d_pr = up(rays), up(res), up(tn), up(per_ray)
    hits = 0
    for first, count in ((0, n), (100, 333), (n - 1, 1)):
        for ns in (1, 4, 32):
            for seed in (0, 12345):
                a = _ao(nt.raygen_ao, d_rays, d_res, d_tn, first, count, ns, 150.0, seed)
                b = _ao(nt.raygen_ao_normals, d_rays, d_res, d_pr, first, count, ns, 150.0, seed)
                for x, y, what in zip(a, b, ("rays", "idToSlot", "slotToID")):
                    assert x.tobytes() == y.tobytes(), (what, first, count, ns, seed)
                hits += int((b[0].view(F).reshape(-1, 8)[:, 7] == F(150.0)).sum())
    assert hits > 0


def test_ao_normals_a_zero_fourth_word_is_a_missed_input():
    rays, res, tn, per_ray, cam = _cornell_batch()
    n = rays.shape[0]
    gone = np.zeros(n, bool)
    gone[3::5] = True
    gone &= res["id"] >= 0
    assert gone.sum() > n // 8
    zeroed = per_ray.copy()
    zeroed[gone, 3] = 0.0
    zeroed[np.flatnonzero(gone)[::2], 3] = -0.0          # (-0 is zero too)
    missed = res.copy()
    missed["id"][gone] = -1
    d_rays = up(rays)
    ns = 4
    a = _ao(nt.raygen_ao, d_rays, up(missed), up(tn), 0, n, ns, 150.0, 99)
    b = _ao(nt.raygen_ao_normals, d_rays, up(res), up(zeroed), 0, n, ns, 150.0, 99)
    assert a[0].tobytes() == b[0].tobytes()
    tmax = b[0].view(F).reshape(-1, 8)[:, 7].reshape(n, ns)
    assert (tmax[gone] == -1).all() and (tmax[res["id"] == -1] == -1).all() and (tmax[~gone & (res["id"] >= 0)] == F(150.0)).all()


def test_ao_normals_match_numpy_restatement():
    """np_raygen.ao_rays with the per-ray normals as its table and ids arange; TOL and the origin bound of tests/test_raygen_gpu.py"""
    rays, res, tn, per_ray, cam = _cornell_batch()
    n = rays.shape[0]
    ns, first, count, seed, maxd = 8, 128, 2500, 0x12345678, 5.0
    got = _ao(nt.raygen_ao_normals, up(rays), up(res), up(per_ray), first, count, ns, maxd, seed)[0].view(F).reshape(-1, 8)
    by_slot = res.copy()
    by_slot["id"] = np.where(res["id"] == -1, -1, np.arange(n))
    ro, rd, rt = np_raygen.ao_rays(rays, by_slot, per_ray[:, :3].copy(), ns, maxd, seed, first, count)
    err_o, err_d = np.abs(got[:, :3] - ro).max(), np.abs(got[:, 4:7] - rd).max()
    print("origins: %.3g (bound %.3g); directions: %.3g (bound %.3g)" % (err_o, 1e-4 * max(1.0, np.abs(ro).max()), err_d, TOL))
    assert err_o < 1e-4 * max(1.0, np.abs(ro).max())
    assert err_d < TOL
    assert np.array_equal(got[:, 7], rt.astype(F)) and (got[:, 3] == 0).all()


# ---- 4. a whole frame, and 5. one graph -------------------------------------------------------------------------------------------------------
W, H, NS, RADIUS = 64, 32, 4, 2.0


class _Frame:
    """The buffers of a frame of W x H primary rays with NS secondary rays each over a scene-like object (trace(n, d_rays, any_hit,
    stream) and .g, a _Geom), and the device passes; primary rays are generated once, on the device."""

    def __init__(self, s):
        self.s, self.n, self.m = s, W * H, W * H * NS
        cam = isc.CAMERA
        self.d_tab = torch.zeros(self.n, dtype=torch.int32, device="cuda:0")
        nt.pixel_table(W, H, self.d_tab.data_ptr())
        self.d_rays, self.d_i2s, self.d_s2i = _filled(32 * self.n), _filled(4 * self.n), _filled(4 * self.n)
        nt.raygen_primary(self.d_rays.data_ptr(), self.d_i2s.data_ptr(), self.d_s2i.data_ptr(), self.d_tab.data_ptr(), cam["eye"],
                          scenes.nscreen_to_world(cam, W, H), W, H, cam["far"])
        torch.cuda.synchronize()
        self.rays = _down(self.d_rays, 32 * self.n).view(nt.RAY_DTYPE)
        self.s2i = _down(self.d_s2i, 4 * self.n).view(np.int32)
        self.d_srays, self.d_si2s, self.d_ss2i = _filled(32 * self.m), _filled(4 * self.m), _filled(4 * self.m)
        rng = np.random.default_rng(4)
        ntri = s.g.tri.shape[0]
        self.mat = rng.integers(0, 2 ** 32, ntri, dtype=np.uint64).astype(np.uint32)
        self.shaded = rng.integers(0, 2 ** 32, ntri, dtype=np.uint64).astype(np.uint32)
        self.d_mat, self.d_shaded = up(self.mat), up(self.shaded)

    def primary(self, stream=0):
        """two-level closest-hit trace of the primary rays and their attributes -> the four device buffers"""
        self.d_res, self.d_ids = self.s.trace(self.n, self.d_rays, False, stream)
        self.d_out, self.d_nrm = self.s.g.attributes(self.n, self.d_res, self.d_ids, stream=stream)

    def secondary(self, max_dist, any_hit, seed, stream=0):
        """the AO / diffuse batch from the primary hits' normals, its two-level trace and its resolved records"""
        nt.raygen_ao_normals(self.d_srays.data_ptr(), self.d_si2s.data_ptr(), self.d_ss2i.data_ptr(), self.d_rays.data_ptr(),
                             self.d_out.data_ptr(), self.d_nrm.data_ptr(), 0, self.n, NS, max_dist, seed, stream)
        self.d_sres, self.d_sids = self.s.trace(self.m, self.d_srays, any_hit, stream)
        self.d_sout, _ = self.s.g.attributes(self.m, self.d_sres, self.d_sids, normals=False, stream=stream)

    def pixels(self, ray_type):
        d_pix = torch.full((self.n + 16,), 0x11223344, dtype=torch.int32, device="cuda:0")
        nt.reconstruct(ray_type, NS, 0, self.n, self.d_s2i.data_ptr(), self.d_out.data_ptr(), self.d_si2s.data_ptr(), self.d_sout.data_ptr(),
                       self.d_mat.data_ptr(), self.d_shaded.data_ptr(), d_pix.data_ptr())
        torch.cuda.synchronize()
        raw = d_pix.cpu().numpy().view(np.uint32)
        assert (raw[self.n:] == 0x11223344).all()
        return raw[:self.n]

    def assert_primary(self, spec_trace, what):
        """the first level against the specs -> the spec's resolved primary records"""
        res, ids = _host(self.d_res, self.d_ids, self.n)
        want_res, want_ids = spec_trace(self.rays, False)
        assert res.tobytes() == want_res.tobytes() and ids.tobytes() == want_ids.tobytes(), ("primary records differ", what)
        want_out, _ = self.s.g.assert_equals_spec(self.n, want_res, want_ids, self.d_out, self.d_nrm, (what, "primary"))
        return want_out

    def assert_secondary(self, spec_trace, any_hit, max_dist, what):
        """the second level: the records equal the spec's trace of the DEVICE-generated rays in all words -> the spec's resolved records"""
        torch.cuda.synchronize()
        srays = _down(self.d_srays, 32 * self.m, "secondary rays").view(nt.RAY_DTYPE)
        si2s = _down(self.d_si2s, 4 * self.m).view(np.int32)
        assert np.array_equal(si2s, np.arange(self.m)) and np.array_equal(_down(self.d_ss2i, 4 * self.m).view(np.int32), np.arange(self.m))
        hit = np.repeat((_down(self.d_out, 16 * self.n).view(nt.RESULT_DTYPE)["id"] >= 0)
                        & (_down(self.d_nrm, 16 * self.n).view(F).reshape(-1, 4)[:, 3] != 0), NS)
        assert (srays["tmax"][hit] == F(max_dist)).all() and (srays["tmax"][~hit] == -1).all()
        res, ids = _host(self.d_sres, self.d_sids, self.m)
        want_res, want_ids = spec_trace(srays, any_hit)
        for k in ("id", "t", "padA", "padB"):
            bad = np.flatnonzero(res[k].view(np.uint32) != want_res[k].view(np.uint32))
            assert bad.size == 0, ("secondary records differ", what, k, int(bad[0]))
        assert ids.tobytes() == want_ids.tobytes(), ("secondary instance ids differ", what)
        want_out, _ = self.s.g.assert_equals_spec(self.m, want_res, want_ids, self.d_sout, None, (what, "secondary"))
        return want_out, si2s


def test_a_whole_frame_on_grid():
    s = _named("grid")
    f = _Frame(s)
    f.primary()
    p_out = f.assert_primary(s.spec_trace, "grid")
    assert (p_out["id"] >= 0).sum() > f.n // 8
    # ambient occlusion: any hit within RADIUS; then diffuse: closest hit up to the far plane
    for ray_type, max_dist, any_hit, seed in ((1, RADIUS, True, 0x51ed270b), (2, isc.CAMERA["far"], False, 0x2545f491)):
        f.secondary(max_dist, any_hit, seed)
        s_out, si2s = f.assert_secondary(s.spec_trace, any_hit, max_dist, ("grid", ray_type))
        occluded = int((s_out["id"] >= 0).sum())
        assert 0 < occluded < f.m
        want = np_rayops.np_reconstruct_vec(ray_type, NS, 0, f.n, f.s2i, p_out, si2s, s_out, f.mat, f.shaded, np.full(f.n, 0x11223344, np.uint32))
        got = f.pixels(ray_type)
        assert np.array_equal(got, want), (ray_type, int((got != want).sum()))
        assert np.unique(got).size > 4
        print("rayType %d: %d of %d secondary rays hit" % (ray_type, occluded, f.m))


def test_refit_trace_attributes_ao_and_trace_as_one_graph():
    """ntr_tlas_refit -> trace -> attributes -> ntr_raygen_ao_normals -> trace -> attributes on one stream, linear: an uncaptured pass
    first (it uploads the refit's table and reserves its scratch), then the capture, then two replays with moved instances, each equal
    to the specs as the whole frame above."""
    import np_tlas_refit as tr
    from test_tlas_refit_cpu import moved, placed, pool
    from test_tlas_refit_gpu import _Tlas
    p = pool()
    d_pool = up(p["nodes"]), up(p["woop"]), up(p["tri_index"])
    inst = placed(9, 41, blas=[0, 0, 1, 0, 2, 0, 0, 2, 0])
    t = _Tlas(p["ranges"], d_pool[0], p["nodes"].size, inst)
    g = _Geom(*geometry(["cornell", "soup1000", "one"]), inst)
    g.d_inst = t.d_inst                       # one instance array for the refit, the trace's records and the attributes
    g.geom.d_instances = t.d_inst.data_ptr()

    def trace(n, d_rays, any_hit, stream=0):
        d_res, d_ids = _filled(16 * n), _filled(4 * n)
        nt.trace_instanced(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), t.d_tlas.data_ptr(), t.nodes_bytes, t.root,
                           t.d_rec.data_ptr(), t.n, d_pool[0].data_ptr(), p["nodes"].size, d_pool[1].data_ptr(), p["woop"].size,
                           d_pool[2].data_ptr(), stream=stream, timed=False)
        return d_res, d_ids
    f = _Frame(types.SimpleNamespace(g=g, trace=trace))
    seed = 0x0badf00d

    def frame(stream):
        t.refit(blocking=False, stream=stream)
        f.primary(stream)
        f.secondary(RADIUS, True, seed, stream)

    def check(cur, what):
        torch.cuda.synchronize()
        want = tr.refit(t.built_nodes, t.root, t.built_records, p["nodes"], p["ranges"], cur)
        t.assert_equals(want, None, what)
        g.inst = cur

        def spec_trace(rays, any_hit):
            return _spec_records(ni.trace(want["nodes"], t.root, want["records"], p, rays, any_hit))
        f.assert_primary(spec_trace, what)
        s_out, _ = f.assert_secondary(spec_trace, True, RADIUS, what)
        return int((s_out["id"] >= 0).sum())

    insts = [moved(inst, 7), moved(inst, 8), moved(inst, 9)]
    st = torch.cuda.Stream()
    t.set_instances(insts[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)
    hits = check(insts[0], "uncaptured")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    for rep, cur in enumerate(insts[1:]):
        t.set_instances(cur)
        for b in (f.d_res, f.d_ids, f.d_out, f.d_nrm, f.d_srays, f.d_si2s, f.d_ss2i, f.d_sres, f.d_sids, f.d_sout, t.d_scene):
            b.fill_(0xAB)
        torch.cuda.synchronize()
        gr.replay()
        hits += check(cur, "graph replay %d" % rep)
    assert hits > 0
    del gr


# ---- 6. determinism and scratch ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_the_calls_hold_no_scratch():
    nt.lbvh_release_workspace()
    pools = (nt.tlas_scratch_bytes, nt.tlas_refit_scratch_bytes, nt.ploc_scratch_bytes, nt.ploc_batch_scratch_bytes, nt.bvh_refit_scratch_bytes,
             nt.bvh_refit_batch_scratch_bytes, nt.bvh_widen_scratch_bytes)
    s = _named("three")
    rays = isc.scene_rays(primary=(64, 32), random=2048)
    n = rays.shape[0]
    d_rays = up(rays)
    d_res, d_ids = s.trace(n, d_rays, False)
    torch.cuda.synchronize()
    nt.lbvh_release_workspace()
    assert [fn() for fn in pools] == [0] * len(pools)
    runs = []
    for _ in range(2):
        d_out, d_nrm = s.g.attributes(n, d_res, d_ids)
        bufs = _filled(32 * n * NS), _filled(4 * n * NS), _filled(4 * n * NS)
        nt.raygen_ao_normals(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), d_rays.data_ptr(), d_out.data_ptr(), d_nrm.data_ptr(),
                             0, n, NS, RADIUS, 17)
        torch.cuda.synchronize()
        runs.append([b.cpu().numpy().tobytes() for b in (d_out, d_nrm) + bufs])
    assert runs[0] == runs[1]
    assert [fn() for fn in pools] == [0] * len(pools), "the calls reserved scratch"
    assert nt.trace_status() == 0
