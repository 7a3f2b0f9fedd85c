"""Motion blur over the 4-wide trees on the device against the numpy rule (tests/np_instanced_wide_motion.py):
ntr_tlas_wide_motion_refit equals wide_motion_refit() byte for byte in wide nodes, wide records, motion keys and scene box, and in its
counts; ntr_trace_instanced_wide_motion equals trace() in all four result words and the instance id, for closest hit and any hit, and
its instrumented form in the ten counters; a captured refit + trace reads keys and times at replay time.  Output buffers are prefilled
with 0xAB and nothing beyond the extents may be written; the status word stays clear.  The wide pool and the wide top-level tree at key 0
are the wide spec's bytes (np_instanced_wide.widen_pool / widen_tlas, which ntr_pool_widen and ntr_tlas_widen equal byte for byte:
test_instanced_wide_gpu.py), uploaded."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_motion_cases as mc
import instanced_scenes as isc
import instanced_wide_motion_cases as wc
import np_bvh_wide as bw
import np_instanced as ni
import np_instanced_wide as niw
import np_instanced_wide_motion as wm
import np_wide_refit as wr
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 64
_cache = {}


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


class _Dev:
    """A pool, its wide pool and two keys on the device, the wide top-level tree at key 0, and 0xAB-bordered buffers of exactly the
    extents for the wide motion refit."""

    def __init__(self, ms):
        self.ms, self.pool, self.n, self.root = ms, ms.pool, ms.n, ms.root
        pool, n = ms.pool, ms.n
        self.wp = niw.widen_pool(pool)
        self.wt = niw.widen_tlas(ms.built["nodes"], ms.root, ms.inst0, pool["ranges"], self.wp["ranges"])
        self.built_nodes = np.ascontiguousarray(self.wt["nodes"]).view(np.int32).reshape(-1, 32).copy()
        self.built_records = self.wt["records"].copy()
        self.d_wide, self.d_woop, self.d_idx = up(self.wp["nodes"]), up(pool["woop"]), up(pool["tri_index"])
        self.wide_bytes = int(self.wp["nodes"].size)
        self.d_inst0, self.d_inst1 = up(ms.inst0), up(ms.inst1)
        self.nodes_bytes, self.rec_bytes, self.keys_bytes = 128 * self.built_nodes.shape[0], 64 * n, 128 * n
        assert (self.nodes_bytes == 0) == (n == 1) and self.root == (-1 if n == 1 else 0)
        self.d_wt, self.d_rec, self.d_keys, self.d_scene = (_filled(b) for b in (self.nodes_bytes, self.rec_bytes, self.keys_bytes, 24))
        self.reset()
        self.set_keys(ms.inst0, ms.inst1)

    def set_keys(self, inst0, inst1):
        self.inst0, self.inst1 = inst0, inst1
        self.d_inst0.copy_(up(inst0))
        self.d_inst1.copy_(up(inst1))

    def reset(self, nodes=None, records=None):
        """The buffers as the widening left them (or the given tree), keys and scene box 0xAB."""
        if self.nodes_bytes:
            self.d_wt[:self.nodes_bytes] = up(self.built_nodes if nodes is None else nodes)
        self.d_rec[:self.rec_bytes] = up(self.built_records if records is None else records)
        self.d_keys.fill_(0xAB)
        self.d_scene.fill_(0xAB)

    def refit(self, blocking=True, stream=0):
        return nt.tlas_wide_motion_refit(self.n, self.d_inst0.data_ptr(), self.d_inst1.data_ptr(), self.pool["ranges"], self.wp["ranges"],
                                         self.d_wide.data_ptr(), self.wide_bytes, self.d_wt.data_ptr() if self.nodes_bytes else 0,
                                         self.nodes_bytes, self.root, self.d_rec.data_ptr(), self.rec_bytes, self.d_keys.data_ptr(),
                                         self.keys_bytes, self.d_scene.data_ptr(), stream=stream, blocking=blocking)

    def plain_refit(self):
        return nt.tlas_wide_refit(self.n, self.d_inst0.data_ptr(), self.pool["ranges"], self.wp["ranges"], self.d_wide.data_ptr(), self.wide_bytes,
                                  self.d_wt.data_ptr() if self.nodes_bytes else 0, self.nodes_bytes, self.root, self.d_rec.data_ptr(),
                                  self.rec_bytes, self.d_scene.data_ptr())

    def spec(self, nodes=None):
        return wm.wide_motion_refit(self.built_nodes if nodes is None else nodes, self.root, self.built_records, self.wp["nodes"],
                                    self.pool["ranges"], self.wp["ranges"], self.inst0, self.inst1)

    def download(self):
        torch.cuda.synchronize()
        raw = [b.cpu().numpy() for b in (self.d_wt, self.d_rec, self.d_keys, self.d_scene)]
        for x, e in zip(raw, (self.nodes_bytes, self.rec_bytes, self.keys_bytes, 24)):
            assert (x[e:] == 0xAB).all(), "bytes beyond the extents were written"
        return (raw[0][:self.nodes_bytes].view(np.int32).reshape(-1, 32).copy(), raw[1][:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy(),
                raw[2][:self.keys_bytes].view(np.uint32).reshape(-1, 32).copy(), raw[3][:24].copy())

    def assert_equals(self, want, res=None, what="", scene=True):
        nodes, records, keys, sb = self.download()
        bad = np.flatnonzero((nodes != want["nodes"]).any(axis=1))
        assert bad.size == 0, ("wide nodes differ", what, int(bad[0]), nodes[bad[0]], want["nodes"][bad[0]])
        assert np.array_equal(records, want["records"]), ("wide records differ", what)
        assert np.array_equal(keys, want["motion_keys"]), ("motion keys differ", what)
        if scene:
            assert sb.tobytes() == want["scene_box"].tobytes(), ("d_sceneBox differs", what)
        if res is not None:
            r = res.refit
            assert (r.numNodes, r.numLeaves, r.errBits, res.numMoving) == (want["stats"]["numNodes"], want["stats"]["numLeaves"], want["err_bits"],
                                                                            want["stats"]["numMoving"]), what
            got = np.concatenate([np.array(list(r.sceneMin), F), np.array(list(r.sceneMax), F)])
            assert got.tobytes() == want["scene_box"].tobytes(), ("sceneMin / sceneMax differ", what)


def _scene_of(n):
    """(pool, transforms, blas) of N instances: the first n of `three`, `grid` (64), or the 300 of instanced_motion_cases.big()."""
    if n <= 3:
        sc = isc.scene("three")
        return isc.pool_of(sc["names"]), sc["transforms"][:n], np.asarray(sc["blas"])[:n]
    if n == 64:
        sc = isc.scene("grid")
        return isc.pool_of(sc["names"]), sc["transforms"], np.asarray(sc["blas"])
    b = mc.big(n)
    return b.pool, b.inst0["objectToWorld"], b.inst0["blas"]


def _dev(n):
    if ("dev", n) not in _cache:
        pool, tf, blas = _scene_of(n)
        inst0 = ni.instances(tf, blas)
        _cache[("dev", n)] = (_Dev(mc.MotionScene(pool, inst0, inst0)), tf, blas)
    return _cache[("dev", n)]


# ---- the refit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 300])
def test_wide_motion_refit_equals_spec(n):
    d, tf, blas = _dev(n)
    inst0 = ni.instances(tf, blas)
    assert (d.built_nodes.shape[0] == 0) == (n == 1) and (n < 300 or 4 * d.built_nodes.shape[0] > 256)   # big(): more than one workgroup
    for what, inst1 in (("key 1 == key 0", inst0), ("every instance moving", ni.instances(mc.key1_transforms(tf, every=True), blas)),
                        ("mixed", ni.instances(mc.key1_transforms(tf), blas))):
        d.set_keys(inst0, inst1)
        want = d.spec()
        for blocking in (True, False):
            d.reset()
            res = d.refit(blocking=blocking)
            assert (res is None) == (not blocking)
            d.assert_equals(want, res, (n, what, blocking))
            if blocking:
                assert res.refit.seconds > 0
        moving = want["stats"]["numMoving"]
        assert moving == {"key 1 == key 0": 0, "every instance moving": n, "mixed": n - n // 3}[what]
        assert int((want["records"][:, 15] != 0).sum()) == moving
        if what == "key 1 == key 0":
            # a refit of a fresh widen changes no byte but the key buffer, and the bytes are ntr_tlas_wide_refit's
            nodes, records, keys, _ = d.download()
            assert nodes.tobytes() == d.built_nodes.tobytes() and records.tobytes() == d.built_records.tobytes()
            assert keys.tobytes() == want["motion_keys"].tobytes()
            d.reset()
            d.plain_refit()
            again = d.download()
            assert nodes.tobytes() == again[0].tobytes() and records.tobytes() == again[1].tobytes()
            assert again[3].tobytes() == want["scene_box"].tobytes()
    # a later plain ntr_tlas_wide_refit writes word 15 = 0: the scene is frozen at key 0
    d.plain_refit()
    assert not d.download()[1][:, 15].any()
    assert nt.trace_status() == 0


@pytest.mark.parametrize("which", [("blas",), ("link",), ("blas", "link", "leaf")])
def test_a_bad_part_is_never_followed(which):
    """5 instances: a link that names no wide node, a leaf link beyond the instances, an instance whose blas index is numBlas; the error
    code and bits, and every byte is the rule's.  The bad instance's record has the empty extent; its key entry is written."""
    pool = isc.pool_of(["cornell", "soup64"])
    tf = isc.seeded_transforms(5, 77, spread=8.0, size=0.02)
    blas = np.array([0, 1, 0, 1, 0], np.int32)
    inst0, inst1 = ni.instances(tf, blas), ni.instances(mc.key1_transforms(tf, every=True), blas)
    d = _Dev(mc.MotionScene(pool, inst0, inst1))
    nodes = d.built_nodes.copy()
    leaves = [(a, k) for a in range(nodes.shape[0]) for k in range(int(nodes[a, bw.WCOUNT])) if nodes[a, bw.WLINK + k] < 0]
    assert len(leaves) == 5
    if "link" in which:
        a, k = leaves[0]
        nodes[a, bw.WLINK + k] = 128 * 9
    if "leaf" in which:
        a, k = leaves[2]
        nodes[a, bw.WLINK + k] = ~7
    bad_i = -1
    if "blas" in which:
        a, k = leaves[4]
        bad_i = ~int(nodes[a, bw.WLINK + k])
        inst0, inst1 = inst0.copy(), inst1.copy()
        inst0["blas"][bad_i] = 2
        d.set_keys(inst0, inst1)
    want = d.spec(nodes)
    bits = sum(b for name, b in (("blas", 1), ("link", 2), ("leaf", 4)) if name in which)
    assert want["err_bits"] == bits
    d.reset(nodes)
    with pytest.raises(nt.NtrError) as e:
        d.refit()
    assert e.value.code == (-1 if "blas" in which else -4) and "ntr_tlas_wide_motion_refit" in str(e.value), str(e.value)
    d.assert_equals(want, e.value.result, which, scene=False)
    got = d.download()
    assert got[3].tobytes() == bytes([0xAB]) * 24                   # the root was not refitted
    if bad_i >= 0:
        assert not got[1][bad_i, 12:15].any() and np.array_equal(got[2][bad_i], want["motion_keys"][bad_i])
    d.reset(nodes)
    assert d.refit(blocking=False) is None                          # the asynchronous form skips the bad part silently
    d.assert_equals(want, None, (which, "asynchronous"), scene=False)
    assert nt.trace_status() == 0


def test_scratch_and_release():
    d, tf, blas = _dev(300)
    d.reset()
    d.refit()
    held = nt.tlas_wide_motion_refit_scratch_bytes()
    assert held >= 8 * d.built_nodes.shape[0] + 16 * 2
    d.reset()
    d.refit(blocking=False)
    torch.cuda.synchronize()
    assert nt.tlas_wide_motion_refit_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.tlas_wide_motion_refit_scratch_bytes() == 0


# ---- the trace ----------------------------------------------------------------------------------------------------------------------------
class _Traced:
    """A MotionScene on the device, refitted by ntr_tlas_wide_motion_refit (whose bytes the refit tests pin to the spec's)."""

    def __init__(self, ms):
        self.ms = ms
        self.d = _Dev(ms)
        self.d.refit()
        self.d.assert_equals(self.d.spec())
        nodes, records, keys, _ = self.d.download()
        self.nodes, self.records, self.keys = nodes, records, keys

    def args(self, n, any_hit, d_rays, d_res, d_ids):
        d = self.d
        return (n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d.d_wt.data_ptr() if d.nodes_bytes else 0, d.nodes_bytes, d.root,
                d.d_rec.data_ptr(), d.n, d.d_wide.data_ptr(), d.wide_bytes, d.d_woop.data_ptr(), d.pool["woop"].size, d.d_idx.data_ptr())

    def launch(self, rays, any_hit, times=None, time=0.0, how="motion", inst_masks=None, ray_mask=0xFFFFFFFF, keys_bytes=None):
        """-> (results as bytes, instance ids as bytes, (stats, motion stats) or None); how: motion, stats, null (motion == NULL), wide"""
        n = rays.shape[0]
        d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
        d_t = up(np.asarray(times, F)) if times is not None else None
        d_M = up(np.asarray(inst_masks, np.uint32)) if inst_masks is not None else None
        vis = nt.InstanceVisibility(d_M.data_ptr() if d_M is not None else 0, 0, ray_mask)
        motion = nt.InstanceMotion(self.d.d_keys.data_ptr(), self.d.keys_bytes if keys_bytes is None else keys_bytes,
                                   d_t.data_ptr() if d_t is not None else 0, time)
        args = self.args(n, any_hit, d_rays, d_res, d_ids)
        st = None
        if how == "wide":
            nt.trace_instanced_wide(*args, vis=vis)
        elif how == "null":
            nt.trace_instanced_wide_motion(*args, vis=vis, motion=None)
        elif how == "stats":
            st = nt.trace_instanced_wide_motion_stats(*args, vis=vis, motion=motion)
        else:
            nt.trace_instanced_wide_motion(*args, vis=vis, motion=motion)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        return res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st

    def spec(self, rays, any_hit, keys_bytes=None, **kw):
        keys = self.keys if keys_bytes is None else self.keys.reshape(-1).view(np.uint8)[:keys_bytes]
        rid, rt, ru, rv, rinst, c = wm.trace(self.nodes, self.d.root, self.records, keys, self.d.pool, self.d.wp, rays, any_hit, **kw)
        return _records(rays, rid, rt, ru, rv), rinst.astype(np.int32).tobytes(), c

    def assert_equals_spec(self, rays, what, counters=True, **kw):
        out = {}
        for any_hit in (False, True):
            want = self.spec(rays, any_hit, **kw)
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
                have = dict(st[0].as_dict(), **st[1].as_dict())
                assert have == want[2], (what, any_hit, have, want[2])
            out[any_hit] = want
        return out


def _records(rays, rid, rt, ru, rv):
    rec = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    rec["id"], rec["t"], rec["padA"], rec["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return rec.tobytes()


def _traced(name):
    if ("traced", name) not in _cache:
        _cache[("traced", name)] = _Traced(mc.big() if name == "big" else mc.named(name))
    return _cache[("traced", name)]


def _rays():
    """The CPU tier's rays (instanced_motion_cases.cpu_rays(): 8 192), so that the spec's side of a test stays within seconds."""
    return mc.cpu_rays()


def _ramp(n):
    """Per-ray times: a ramp over [0, 1] with the corner times among its first entries."""
    t = np.linspace(0.0, 1.0, n).astype(F)
    t[1:1 + min(n - 1, mc.CORNER_TIMES.size)] = mc.CORNER_TIMES[:max(0, min(n - 1, mc.CORNER_TIMES.size))]
    return t


@pytest.mark.parametrize("name", mc.SCENES + ["big"])
def test_wide_motion_trace_equals_spec_on_the_scenes(name):
    s = _traced(name)
    rays = _rays()
    n = rays.shape[0]
    w0 = s.assert_equals_spec(rays, name + " t = 0", time=0.0)
    w1 = s.assert_equals_spec(rays, name + " t = 1", time=1.0)
    wh = s.assert_equals_spec(rays, name + " t = 0.5", counters=False, time=0.5)
    wr_ = s.assert_equals_spec(rays, name + " ramp", times=_ramp(n))
    assert len({w[False][0] for w in (w0, w1, wh, wr_)}) == 4          # the four poses give four different answers
    c = wr_[False][2]
    assert 0 < c["numMovingEntries"] <= c["numInstanceEntries"] and c["numSingular"] == 0 and c["numHits"] > 0
    # the corner times as the launch's scalar, and repeated across the rays
    for t in mc.CORNER_TIMES:
        s.assert_equals_spec(rays[:1024], "%s scalar time %r" % (name, t), counters=False, time=float(t) if t == t else float("nan"))
    s.assert_equals_spec(rays[:1024], name + " corner times per ray", times=np.resize(mc.CORNER_TIMES, 1024))
    # the ends are the keys: t = 0 is the wide masked launch over the same buffers (key-0 records)
    for any_hit in (False, True):
        assert s.launch(rays, any_hit, how="wide")[:2] == w0[any_hit][:2]
    st = s.launch(rays, False, times=_ramp(n), how="stats")[2]
    assert st[1].algorithmic_bytes(st[0], ray_times=True) == wm.algorithmic_bytes(c, ray_times=True)
    print("%s ramp: %r %r, %d algorithmic bytes" % (name, st[0].as_dict(), st[1].as_dict(), st[1].algorithmic_bytes(st[0], ray_times=True)))


@pytest.mark.parametrize("n", [1, 65])
def test_ray_counts_below_and_across_a_wave(n):
    s = _traced("three")
    rays = isc.scene_rays((8, 8), 1000)[:n]
    s.assert_equals_spec(rays, "%d rays ramp" % n, times=_ramp(n))
    s.assert_equals_spec(rays, "%d rays scalar" % n, time=0.3)


def test_masks_with_motion():
    """A refused moving instance counts as masked only -- neither a moving entry nor a singular step -- and the visible ones are posed."""
    s = _traced("grid")
    rays = _rays()[:4096]
    M = np.where(np.arange(s.d.n) % 2 == 0, 1, 2).astype(np.uint32)
    for ray_mask in (1, 2, 0x80000000):
        w = s.assert_equals_spec(rays, "grid parity, ray mask %#x" % ray_mask, times=_ramp(4096), inst_masks=M, ray_mask=ray_mask)
        c = w[False][2]
        assert c["numInstancesMasked"] > 0
        if ray_mask == 0x80000000:
            assert c["numInstanceEntries"] == c["numMovingEntries"] == c["numSingular"] == 0


def test_exact_singular_pair_is_popped_and_counted():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    s = _Traced(mc.two_of_one(a, b.reshape(12)))
    rays = mc.one_rays()
    w = s.assert_equals_spec(rays, "singular at 0.5", time=0.5)
    c = w[False][2]
    assert c["numSingular"] > 0 and c["numMovingEntries"] == 0 and c["numHits"] > 0
    ids = np.frombuffer(w[False][1], np.int32)
    assert (ids == 1).any() and not (ids == 0).any()
    w = s.assert_equals_spec(rays, "not singular at 0.25", time=0.25)
    assert w[False][2]["numSingular"] == 0 and w[False][2]["numMovingEntries"] > 0
    # per-ray times: only the rays at exactly 0.5 are popped
    t = np.where(np.arange(rays.shape[0]) % 2 == 0, F(0.5), F(0.25)).astype(F)
    w = s.assert_equals_spec(rays, "every other ray singular", times=t)
    assert 0 < w[False][2]["numSingular"] and 0 < w[False][2]["numMovingEntries"]


def test_a_key_buffer_cut_to_the_minimum():
    """motionKeysBytes == 128 * numInstances is the least the call accepts, and the descriptor ends there: the last instance's entry is
    read in full.  (Below it the call is refused; the spec reads an entry beyond the extent as zeros.)"""
    s = _traced("grid")
    rays = _rays()[:2048]
    w = s.assert_equals_spec(rays, "keys cut to 128 N", times=_ramp(2048), keys_bytes=128 * s.d.n)
    assert w[False][2]["numSingular"] == 0 and w[False][2]["numMovingEntries"] > 0
    with pytest.raises(nt.NtrError) as e:
        s.launch(rays, False, time=0.5, keys_bytes=128 * s.d.n - 1)
    assert e.value.code == -1 and "motionKeysBytes below 128 * numInstances" in str(e.value)


@pytest.mark.parametrize("name", ["three", "grid"])
def test_motion_null_and_nothing_moving_give_the_wide_launchs_bytes(name):
    ms = mc.named(name)
    rays = _rays()
    n = rays.shape[0]
    s = _traced(name)
    for any_hit in (False, True):
        plain = s.launch(rays, any_hit, how="wide")[:2]
        assert s.launch(rays, any_hit, how="null")[:2] == plain                           # motion == NULL
    still = _Traced(mc.MotionScene(ms.pool, ms.inst0, ms.inst0))                          # nothing moves, but a times array
    assert not still.records[:, 15].any()
    for any_hit in (False, True):
        plain = still.launch(rays, any_hit, how="wide")[:2]
        assert still.launch(rays, any_hit, times=_ramp(n))[:2] == plain
        res, ids, st = still.launch(rays, any_hit, times=_ramp(n), how="stats")
        assert (res, ids) == plain and st[1].as_dict() == dict(numMovingEntries=0, numSingular=0)


# ---- one stream, one graph ----------------------------------------------------------------------------------------------------------------
def test_wide_motion_refit_and_trace_as_one_graph():
    ms = mc.named("grid")
    sc = isc.scene("grid")
    d = _Dev(ms)
    rays = _rays()[:4096]
    n = rays.shape[0]
    d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
    uploads = [(ms.inst1, _ramp(n)), (ni.instances(mc.key1_transforms(sc["transforms"], seed=9, every=True), sc["blas"]), np.full(n, 0.75, F)),
               (ms.inst0, _ramp(n)[::-1].copy())]
    d_times = up(uploads[0][1])
    motion = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, d_times.data_ptr(), 0.0)
    st = torch.cuda.Stream()

    def frame(stream):
        d.refit(blocking=False, stream=stream)
        nt.trace_instanced_wide_motion(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d.d_wt.data_ptr(), d.nodes_bytes, d.root,
                                       d.d_rec.data_ptr(), d.n, d.d_wide.data_ptr(), d.wide_bytes, d.d_woop.data_ptr(), d.pool["woop"].size,
                                       d.d_idx.data_ptr(), vis=None, motion=motion, stream=stream, timed=False)

    def check(k, what):
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        want = d.spec()
        d.assert_equals(want, None, what)
        rid, rt, ru, rv, rinst, _ = wm.trace(want["nodes"], d.root, want["records"], want["motion_keys"], d.pool, d.wp, rays, False,
                                             times=uploads[k][1])
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all()
        assert res[:16 * n].tobytes() == _records(rays, rid, rt, ru, rv) and ids[:4 * n].tobytes() == rinst.astype(np.int32).tobytes(), what
        return res[:16 * n].tobytes()

    # an identical uncaptured pass first: it uploads the range table and reserves the scratch
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)
    seen = [check(0, "uncaptured")]
    held = nt.tlas_wide_motion_refit_scratch_bytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    assert nt.tlas_wide_motion_refit_scratch_bytes() == held
    for rep, k in enumerate((1, 2, 0)):
        d.set_keys(ms.inst0, uploads[k][0])
        d_times.copy_(up(uploads[k][1]))
        d.reset()
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        seen.append(check(k, "graph replay %d" % rep))
    assert seen[1] != seen[2] and seen[3] == seen[0]
    # the blocking refit and the instrumented trace are refused on a capturing stream
    errs = []
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        d_ids.fill_(0xAB)    # so that the graph is not empty
        cur = torch.cuda.current_stream().cuda_stream
        for call in (lambda: d.refit(blocking=True, stream=cur),
                     lambda: nt.trace_instanced_wide_motion_stats(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d.d_wt.data_ptr(),
                                                                  d.nodes_bytes, d.root, d.d_rec.data_ptr(), d.n, d.d_wide.data_ptr(), d.wide_bytes,
                                                                  d.d_woop.data_ptr(), d.pool["woop"].size, d.d_idx.data_ptr(), vis=None,
                                                                  motion=motion, stream=cur)):
            try:
                call()
            except nt.NtrError as e:
                errs.append(e.code)
    torch.cuda.synchronize()
    assert errs == [-1, -1]
