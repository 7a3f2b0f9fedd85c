"""Deforming BLASes in the motion-blurred two-level trace on the device against the numpy rule (tests/np_instanced_deform.py):
ntr_tlas_deform_refit equals deform_refit() byte for byte in nodes, records, motion keys and scene box, and in its counts;
ntr_trace_instanced_deform equals trace() in all four result words and the instance id, for closest hit and any hit, and its
instrumented form in the thirteen counters; the consequences a, b and c of the rule hold against the older entry points themselves; a
captured chain of per-BLAS motion refits, top-level refit and trace reads flags, keys and times at replay time.  The pool's key-1
buffers are made on the device by ntr_bvh_motion_refit at pool + offset; output buffers are prefilled with 0xAB and nothing beyond the
extents may be written; the status word stays clear."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import bvh_motion_cases as bc
import instanced_deform_cases as dc
import instanced_scenes as isc
import np_bvh_refit as rf
import np_instanced as ni
import np_instanced_deform as nd
import np_instanced_motion as mo
import np_tlas_refit as tr
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 64
FILL = 0xCD          # np_instanced_deform.pool_motion_refit's: the bytes of the key-1 buffers that belong to no deforming BLAS
_cache = {}


def _filled(nbytes, byte=0xAB):
    return torch.full((int(nbytes) + SLACK,), byte, dtype=torch.uint8, device="cuda:0")


def _records(rays, rid, rt, ru, rv):
    rec = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    rec["id"], rec["t"], rec["padA"], rec["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return rec.tobytes()


class _Dev:
    """A DeformScene on the device.  The pool starts as the builders left it; ntr_bvh_motion_refit at pool + offset makes key 1 of every
    deforming BLAS (pose()); the top-level tree is ntr_tlas_build's at key 0 over that pool, downloaded: those bytes are the rule's input."""

    def __init__(self, s):
        self.s, self.n = s, s.n
        base = isc.pool_of(s.names)
        self.nb, self.wb = base["nodes"].size, base["woop"].size
        self.d_nodes, self.d_woop, self.d_idx = up(base["nodes"]), up(base["woop"]), up(base["tri_index"])
        self.d_nodes1, self.d_v0, self.d_v1 = _filled(self.nb, FILL), _filled(self.wb, FILL), _filled(self.wb, FILL)
        self.d_flags = up(s.pool["deforming"])
        self.d_mesh = {b: (up(m[0]), up(m[1]), up(m[2])) for b, m in enumerate(s.meshes) if m is not None}
        self.pose()
        torch.cuda.synchronize()
        for name, buf in (("nodes", self.d_nodes), ("woop", self.d_woop), ("nodes1", self.d_nodes1), ("vrows0", self.d_v0), ("vrows1", self.d_v1)):
            got = buf.cpu().numpy()[:s.pool[name].size]
            assert got.tobytes() == s.pool[name].tobytes(), ("the pool's " + name + " differs from the spec's", s.names)
        self.d_inst0, self.d_inst1 = up(s.inst0), up(s.inst1)
        n = self.n
        self.nodes_bytes, self.rec_bytes, self.keys_bytes = 64 * (n - 1), 64 * n, 128 * n
        self.root = -1 if n == 1 else 0
        caps = nt.tlas_capacity(n)
        d_tlas, d_rec = _filled(caps[0]), _filled(caps[1])
        res = nt.tlas_build(n, self.d_inst0.data_ptr(), s.ranges, self.d_nodes.data_ptr(), self.nb, d_tlas.data_ptr(), caps[0], d_rec.data_ptr(),
                            caps[1])
        torch.cuda.synchronize()
        assert (res.nodesBytes, res.recordsBytes, res.rootLink) == (self.nodes_bytes, self.rec_bytes, self.root)
        self.built_nodes = d_tlas.cpu().numpy()[:self.nodes_bytes].view(np.int32).reshape(-1, 16).copy()
        self.built_records = d_rec.cpu().numpy()[:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy()
        self.d_tlas, self.d_rec, self.d_keys, self.d_scene = (_filled(b) for b in (self.nodes_bytes, self.rec_bytes, self.keys_bytes, 24))
        self.deform = nt.InstanceDeform(self.d_nodes1.data_ptr(), self.d_v0.data_ptr(), self.d_v1.data_ptr())
        self.reset()

    def pose(self, stream=0, blocking=True):
        """ntr_bvh_motion_refit at pool + offset for every BLAS that has a mesh with two keys, on `stream`"""
        for b, (d_tri, d_p0, d_p1) in self.d_mesh.items():
            n_off, n_bytes, w_off, w_bytes = self.s.ranges[b]
            tri, pos = self.s.meshes[b][0], self.s.meshes[b][1]
            nt.bvh_motion_refit(self.d_nodes.data_ptr() + n_off, n_bytes, self.d_nodes1.data_ptr() + n_off, self.d_woop.data_ptr() + w_off, w_bytes,
                                self.d_idx.data_ptr() + w_off // 4, w_bytes // 4, self.d_v0.data_ptr() + w_off, self.d_v1.data_ptr() + w_off,
                                tri.shape[0], d_tri.data_ptr(), pos.shape[0], d_p0.data_ptr(), d_p1.data_ptr(), 0.0, stream=stream,
                                blocking=blocking)

    def reset(self):
        """The top-level buffers as the build left them, keys and scene box 0xAB."""
        self.d_tlas[:self.nodes_bytes] = up(self.built_nodes)
        self.d_rec[:self.rec_bytes] = up(self.built_records)
        self.d_keys.fill_(0xAB)
        self.d_scene.fill_(0xAB)

    def refit(self, blocking=True, stream=0, how="deform"):
        a = (self.n, self.d_inst0.data_ptr(), self.d_inst1.data_ptr(), self.s.ranges, self.d_nodes.data_ptr())
        b = (self.d_tlas.data_ptr(), self.nodes_bytes, self.root, self.d_rec.data_ptr(), self.rec_bytes, self.d_keys.data_ptr(), self.keys_bytes,
             self.d_scene.data_ptr())
        if how == "motion":
            return nt.tlas_motion_refit(*a, self.nb, *b, stream=stream, blocking=blocking)
        return nt.tlas_deform_refit(*a, self.d_nodes1.data_ptr(), self.nb, self.d_flags.data_ptr(), *b, stream=stream, blocking=blocking)

    def spec(self, pool=None, inst1=None):
        pool = self.s.pool if pool is None else pool
        return nd.deform_refit(self.built_nodes, self.root, self.built_records, pool["nodes"], pool["nodes1"], self.s.ranges, pool["deforming"],
                               self.s.inst0, self.s.inst1 if inst1 is None else inst1)

    def download(self):
        torch.cuda.synchronize()
        raw = [b.cpu().numpy() for b in (self.d_tlas, self.d_rec, self.d_keys, self.d_scene)]
        for x, e in zip(raw, (self.nodes_bytes, self.rec_bytes, self.keys_bytes, 24)):
            assert (x[e:] == 0xAB).all(), "bytes beyond the extents were written"
        return (raw[0][:self.nodes_bytes].view(np.int32).reshape(-1, 16).copy(), raw[1][:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy(),
                raw[2][:self.keys_bytes].view(np.uint32).reshape(-1, 32).copy(), raw[3][:24].copy())

    def assert_equals(self, want, res=None, what=""):
        nodes, records, keys, sb = self.download()
        bad = np.flatnonzero((nodes != want["nodes"]).any(axis=1))
        assert bad.size == 0, ("nodes differ", what, int(bad[0]), nodes[bad[0]], want["nodes"][bad[0]])
        assert np.array_equal(records, want["records"]), ("records differ", what)
        assert np.array_equal(keys, want["motion_keys"]), ("motion keys differ", what)
        assert sb.tobytes() == want["scene_box"].tobytes(), ("d_sceneBox differs", what)
        if res is not None:
            r, st = res.motion.refit, want["stats"]
            assert (r.numNodes, r.numLeaves, r.errBits, res.motion.numMoving, res.numDeforming) == (st["numNodes"], st["numLeaves"], want["err_bits"],
                                                                                                  st["numMoving"], st["numDeforming"]), what
            got = np.concatenate([np.array(list(r.sceneMin), F), np.array(list(r.sceneMax), F)])
            assert got.tobytes() == want["scene_box"].tobytes(), ("sceneMin / sceneMax differ", what)

    # ---- the trace ------------------------------------------------------------------------------------------------------------------
    def args(self, n, any_hit, d_rays, d_res, d_ids, d_nodes=None, d_woop=None, d_rec=None):
        return (n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), self.d_tlas.data_ptr(), self.nodes_bytes, self.root,
                (self.d_rec if d_rec is None else d_rec).data_ptr(), self.n, (self.d_nodes if d_nodes is None else d_nodes).data_ptr(), self.nb,
                (self.d_woop if d_woop is None else d_woop).data_ptr(), self.wb, self.d_idx.data_ptr())

    def launch(self, rays, any_hit, times=None, time=0.0, how="deform", inst_masks=None, ray_mask=0xFFFFFFFF, **bufs):
        """-> (results as bytes, instance ids as bytes, the stats objects or None); how: deform, stats, motion (ntr_trace_instanced_motion),
        null (deform == NULL), masked (ntr_trace_instanced_masked)"""
        n = rays.shape[0]
        d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
        d_t = up(np.asarray(times, F)) if times is not None else None
        d_M = up(np.asarray(inst_masks, np.uint32)) if inst_masks is not None else None
        vis = nt.InstanceVisibility(d_M.data_ptr() if d_M is not None else 0, 0, ray_mask)
        motion = nt.InstanceMotion(self.d_keys.data_ptr(), self.keys_bytes, d_t.data_ptr() if d_t is not None else 0, time)
        args = self.args(n, any_hit, d_rays, d_res, d_ids, **bufs)
        st = None
        if how == "masked":
            nt.trace_instanced_masked(*args, vis=vis)
        elif how == "motion":
            nt.trace_instanced_motion(*args, vis=vis, motion=motion)
        elif how == "null":
            nt.trace_instanced_deform(*args, vis=vis, motion=motion, deform=None)
        elif how == "stats":
            st = nt.trace_instanced_deform_stats(*args, vis=vis, motion=motion, deform=self.deform)
        else:
            nt.trace_instanced_deform(*args, vis=vis, motion=motion, deform=self.deform)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        return res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st

    def spec_trace(self, rays, any_hit, **kw):
        rid, rt, ru, rv, rinst, c = self.s.trace(rays, any_hit, **kw)
        return _records(rays, rid, rt, ru, rv), rinst.astype(np.int32).tobytes(), c

    def assert_equals_spec(self, rays, what, counters=True, **kw):
        out = {}
        for any_hit in (False, True):
            want = self.spec_trace(rays, any_hit, **kw)
            got = self.launch(rays, any_hit, **kw)
            for name, g, e, dt in (("record", got[0], want[0], np.uint32), ("instance", got[1], want[1], np.int32)):
                if g != e:
                    g, e = np.frombuffer(g, dt), np.frombuffer(e, dt)
                    bad = np.flatnonzero(g != e)
                    raise AssertionError("%s anyHit=%d: %d %s words differ, first at word %d: %r != %r"
                                         % (what, any_hit, bad.size, name, bad[0], g[bad[0]], e[bad[0]]))
            if counters:
                res, ids, st = self.launch(rays, any_hit, how="stats", **kw)
                assert res == got[0] and ids == got[1], (what, any_hit, "the instrumented kernel's records differ")
                have = dict(st[0].as_dict(), **st[1].as_dict(), **st[2].as_dict())
                assert have == want[2], (what, any_hit, have, want[2])
            out[any_hit] = want
        return out


def _dev(name):
    """The scene on the device, refitted by ntr_tlas_deform_refit (whose bytes the refit tests pin to the spec's)."""
    if name not in _cache:
        d = _Dev(dc.big() if name == "big" else dc.named(name))
        d.refit()
        d.assert_equals(d.s.refit)
        _cache[name] = d
    return _cache[name]


# ---- the refit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES + ["three_static", "collapse", "big"])
def test_deform_refit_equals_spec(name):
    d = _Dev(dc.big() if name == "big" else dc.named(name))
    want = d.spec()
    assert want["records"].tobytes() == d.s.refit["records"].tobytes()          # the device-built tree is the spec's
    st = want["stats"]
    assert st["numDeforming"] == int((want["records"][:, 15] & 2 != 0).sum()) and st["numMoving"] == int((want["records"][:, 15] & 1 != 0).sum())
    assert (st["numDeforming"] > 0) == (name != "three_static")
    for blocking in (True, False):
        d.reset()
        res = d.refit(blocking=blocking)
        assert (res is None) == (not blocking)
        d.assert_equals(want, res, (name, blocking))
    # nothing moving: the instances' key 1 is key 0, the BLASes still deform (two boxes: K = {key 0})
    d.d_inst1.copy_(up(d.s.inst0))
    d.reset()
    d.assert_equals(d.spec(inst1=d.s.inst0), d.refit(), (name, "instances static"))
    assert nt.trace_status() == 0


@pytest.mark.parametrize("name", ["three", "big"])
def test_refit_with_no_flag_set_writes_the_motion_refits_bytes(name):
    d = _Dev(dc.big() if name == "big" else dc.named(name))
    d.d_flags.zero_()
    d.reset()
    res = d.refit()
    mine = d.download()
    assert res.numDeforming == 0 and not (mine[1][:, 15] & 2).any()
    d.reset()
    ref = d.refit(how="motion")
    theirs = d.download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, theirs))
    assert {k: v for k, v in res.motion.as_dict().items() if k != "seconds"} == {k: v for k, v in ref.as_dict().items() if k != "seconds"}
    want = mo.motion_refit(d.built_nodes, d.root, d.built_records, d.s.pool["nodes"], d.s.ranges, d.s.inst0, d.s.inst1)
    assert mine[0].tobytes() == want["nodes"].tobytes() and mine[1].tobytes() == want["records"].tobytes()


def test_scratch_is_reported_and_released():
    d = _Dev(dc.big())
    d.refit()
    held = nt.tlas_deform_refit_scratch_bytes()
    assert held >= 8 * 299 + 16 * 2
    d.reset()
    d.refit(blocking=False)
    torch.cuda.synchronize()
    assert nt.tlas_deform_refit_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.tlas_deform_refit_scratch_bytes() == 0


# ---- the trace ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES + ["collapse", "big"])
def test_deform_trace_equals_spec_on_the_scenes(name):
    d = _dev(name)
    rays = dc.rays_of("cpu")
    n = rays.shape[0]
    w0 = d.assert_equals_spec(rays, name + " t = 0", time=0.0)
    w1 = d.assert_equals_spec(rays, name + " t = 1", time=1.0)
    wi = [d.assert_equals_spec(rays, "%s t = %r" % (name, tau), counters=tau == 0.5, time=tau) for tau in dc.INTERIOR]
    wh = d.assert_equals_spec(rays, name + " hashed times", times=bc.hashed_times(n))
    # the middle of the shutter differs from both keys on at least one ray
    assert wi[1][False][0] != w0[False][0] and wi[1][False][0] != w1[False][0]
    c = wh[False][2]
    assert 0 < c["numDeformEntries"] <= c["numInstanceEntries"] and 0 < c["numDeformInnerVisits"] <= c["numInnerVisits"]
    assert 0 < c["numDeformTriTests"] <= c["numTriTests"] and c["numHits"] > 0
    if name == "three":                                                         # waves mix static and deforming lanes
        assert c["numDeformEntries"] < c["numInstanceEntries"] and c["numDeformTriTests"] < c["numTriTests"]
    st = d.launch(rays, False, times=bc.hashed_times(n), how="stats")[2]
    print("%s hashed: %r %r %r, %d algorithmic bytes" % (name, st[0].as_dict(), st[1].as_dict(), st[2].as_dict(),
                                                        st[2].algorithmic_bytes(st[0], st[1], ray_times=True)))
    assert st[2].algorithmic_bytes(st[0], st[1], ray_times=True) == nd.algorithmic_bytes(c, ray_times=True)
    assert nt.trace_status() == 0


@pytest.mark.parametrize("kind", ["tail", "single", "odd"])
def test_ray_sets_below_and_across_a_wave(kind):
    rays = dc.rays_of(kind)
    n = rays.shape[0]
    assert n == {"tail": 4097, "single": 1, "odd": 256}[kind]
    for name in ("three", "grid"):
        d = _dev(name)
        d.assert_equals_spec(rays, "%s %s hashed" % (name, kind), times=bc.hashed_times(n))
        d.assert_equals_spec(rays, "%s %s scalar" % (name, kind), counters=False, time=0.8125)


def test_corner_times_and_masks_with_deform():
    d = _dev("grid")
    rays = dc.rays_of("cpu")[:2048]
    for t in dc.CORNER_TIMES:
        d.assert_equals_spec(rays, "grid scalar time %r" % t, counters=False, time=float(t) if t == t else float("nan"))
    d.assert_equals_spec(rays, "grid corner times per ray", times=np.resize(dc.CORNER_TIMES, 2048))
    M = np.where(np.arange(d.n) % 2 == 0, 1, 2).astype(np.uint32)
    for ray_mask in (1, 2, 0x80000000):
        w = d.assert_equals_spec(rays, "grid parity, ray mask %#x" % ray_mask, times=bc.hashed_times(2048), inst_masks=M, ray_mask=ray_mask)
        c = w[False][2]
        assert c["numInstancesMasked"] > 0
        if ray_mask == 0x80000000:
            assert c["numInstanceEntries"] == c["numDeformEntries"] == c["numDeformInnerVisits"] == 0


# ---- the consequences, against the older entry points themselves ----------------------------------------------------------------------
def test_a_nothing_deforming_gives_the_motion_launchs_bytes():
    rays = dc.rays_of("cpu")
    n = rays.shape[0]
    d = _dev("three_static")
    assert not (d.s.refit["records"][:, 15] & 2).any()
    for any_hit in (False, True):
        for kw in (dict(time=0.5), dict(times=bc.hashed_times(n))):
            motion = d.launch(rays, any_hit, how="motion", **kw)[:2]
            assert d.launch(rays, any_hit, **kw)[:2] == motion
            assert d.launch(rays, any_hit, how="null", **kw)[:2] == motion               # deform == NULL
            res, ids, st = d.launch(rays, any_hit, how="stats", **kw)
            assert (res, ids) == motion and st[2].as_dict() == dict(numDeformEntries=0, numDeformInnerVisits=0, numDeformTriTests=0)
            assert st[1].numMovingEntries > 0


def test_b_one_identity_instance_is_the_single_level_motion_trace():
    tf = ni.IDENTITY[None]
    inst = ni.instances(tf, [0])
    s = dc.DeformScene(["soup1000"], inst, inst, {0: 0.3})
    d = _Dev(s)
    d.refit()
    d.assert_equals(s.refit)
    assert s.refit["records"][0, 15] == 2
    rays = isc.finite_edge_rays()
    rays = np.concatenate([dc.rays_of("cpu")[:2048], rays])
    n = rays.shape[0]
    times = bc.hashed_times(n)
    d_rays, d_t = up(rays), up(times)
    for any_hit in (False, True):
        got, ids, st = d.launch(rays, any_hit, times=times, how="stats")
        d_res = _filled(16 * n)
        bm_motion = nt.BvhMotion(d.d_nodes1.data_ptr(), d.d_v0.data_ptr(), d.d_v1.data_ptr(), d_t.data_ptr(), 0.0)
        ref = nt.trace_bvh_motion_stats(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d.d_nodes.data_ptr(), d.nb, d.wb, d.d_idx.data_ptr(), bm_motion)
        torch.cuda.synchronize()
        assert got == d_res.cpu().numpy()[:16 * n].tobytes(), any_hit
        assert (st[0].numInnerVisits, st[0].numTriTests, st[0].numLeafVisits, st[0].numHits) == (ref.numInnerVisits, ref.numTriTests,
                                                                                              ref.numLeafVisits, ref.numHits)
        assert (st[2].numDeformInnerVisits, st[2].numDeformTriTests) == (ref.numInnerVisits, ref.numTriTests)
        hit = np.frombuffer(got, nt.RESULT_DTYPE)["id"] != -1
        assert np.array_equal(np.frombuffer(ids, np.int32), np.where(hit, 0, -1))


@pytest.mark.parametrize("name", ["three", "grid"])
def test_c_at_the_shutters_ends_the_trace_is_the_masked_launch_over_that_keys_pool(name):
    d = _dev(name)
    s = d.s
    rays = dc.rays_of("cpu")
    # key 1's pool: nodes1's boxes with nodes' links, the Woop rows of np_bvh_refit.refit(pos1)
    nodes1, woop1 = s.pool["nodes"].copy(), s.pool["woop"].copy()
    for b, mesh in enumerate(s.meshes):
        if mesh is None:
            continue
        n_off, n_bytes, w_off, w_bytes = s.ranges[b]
        m, tidx = s.blas_slices(b)
        nodes1[n_off:n_off + n_bytes] = m["nodes1"].view(np.uint8).reshape(-1)
        woop1[w_off:w_off + w_bytes] = rf.refit(m["nodes0"], m["woop"], tidx, mesh[0], mesh[2], 0.0)["woop"]
    rec1 = np.stack([tr.record_of(s.inst1[i], s.ranges) for i in range(s.n)])
    rec0 = np.stack([tr.record_of(s.inst0[i], s.ranges) for i in range(s.n)])
    for t, bufs in ((0.0, dict(d_rec=up(rec0))), (1.0, dict(d_nodes=up(nodes1), d_woop=up(woop1), d_rec=up(rec1)))):
        for any_hit in (False, True):
            assert d.launch(rays, any_hit, time=t)[:2] == d.launch(rays, any_hit, how="masked", **bufs)[:2], (name, t, any_hit)


# ---- one stream, one graph --------------------------------------------------------------------------------------------------------------
def test_blas_refits_top_level_refit_and_trace_as_one_graph():
    """The per-BLAS motion refits, ntr_tlas_deform_refit and the trace, asynchronous on one stream and captured as one graph that is
    replayed after the ray times, the flag array and the meshes' key 1 were rewritten."""
    s = dc.named("three")
    d = _Dev(s)
    rays = dc.rays_of("cpu")[:4096]
    n = rays.shape[0]
    d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
    times = [bc.hashed_times(n), np.full(n, 0.75, F), bc.hashed_times(n, seed=4)]
    d_times = up(times[0])
    motion = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, d_times.data_ptr(), 0.0)
    st = torch.cuda.Stream()
    s3 = dc.DeformScene(s.names, s.inst0, s.inst1, {1: 0.1})                    # the second state: BLAS 1 deforms by another amount

    def frame(stream):
        d.pose(stream=stream, blocking=False)
        d.refit(blocking=False, stream=stream)
        nt.trace_instanced_deform(*d.args(n, False, d_rays, d_res, d_ids), vis=None, motion=motion, deform=d.deform, stream=stream, timed=False)

    def check(scene, flags, tm, what):
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        pool = dict(scene.pool, deforming=np.asarray(flags, np.uint32))
        want = nd.deform_refit(d.built_nodes, d.root, d.built_records, pool["nodes"], pool["nodes1"], scene.ranges, pool["deforming"], scene.inst0,
                               scene.inst1)
        d.assert_equals(want, None, what)
        rid, rt, ru, rv, rinst, _ = nd.trace(want["nodes"], d.root, want["records"], want["motion_keys"], pool, rays, False, times=tm)
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all()
        assert res[:16 * n].tobytes() == _records(rays, rid, rt, ru, rv) and ids[:4 * n].tobytes() == rinst.astype(np.int32).tobytes(), what
        return res[:16 * n].tobytes()

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)                       # uncaptured first: it uploads the range table and reserves the scratch
    seen = [check(s, s.pool["deforming"], times[0], "uncaptured")]
    held = nt.tlas_deform_refit_scratch_bytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    assert nt.tlas_deform_refit_scratch_bytes() == held
    # replay 1: the same inputs, other times.  replay 2: the mesh's key 1 rewritten in place, other times.  replay 3: the flag cleared
    d_times.copy_(up(times[1]))
    d.reset(); d_res.fill_(0xAB); d_ids.fill_(0xAB)
    torch.cuda.synchronize()
    g.replay()
    seen.append(check(s, s.pool["deforming"], times[1], "replay, other times"))
    d.d_mesh[1][2].copy_(up(s3.meshes[1][2]))
    flags = [0, 1, 0]
    d_times.copy_(up(times[2]))
    d.reset(); d_res.fill_(0xAB); d_ids.fill_(0xAB)
    torch.cuda.synchronize()
    g.replay()
    seen.append(check(s3, flags, times[2], "replay, key 1 and times rewritten"))
    d.d_flags.zero_()
    d.reset(); d_res.fill_(0xAB); d_ids.fill_(0xAB)
    torch.cuda.synchronize()
    g.replay()
    seen.append(check(s3, [0, 0, 0], times[2], "replay, no flag set"))
    assert len(set(seen)) == 4
    # the instrumented form is refused on a capturing stream
    errs = []
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        d_ids.fill_(0xAB)    # so that the graph is not empty
        try:
            nt.trace_instanced_deform_stats(*d.args(n, False, d_rays, d_res, d_ids), vis=None, motion=motion, deform=d.deform,
                                            stream=torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            errs.append((e.code, "cannot be captured" in str(e)))
    torch.cuda.synchronize()
    assert errs == [(-1, True)]
