"""The two-level trace over 4-wide trees on the device: ntr_pool_widen and ntr_tlas_widen equal the numpy spec
(tests/np_instanced_wide.py) byte for byte; ntr_trace_instanced_wide equals it in all four result words and the instance id, for closest
hit and any hit, with and without masks; ntr_trace_instanced_wide_stats gives the same bytes and the spec's eight counters.  Output
buffers are prefilled with 0xAB and nothing beyond the extents may be written; the status word stays clear."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_wide as nw
from gpu_util import up
from test_instanced_gpu import _Scene, _filled

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ["three", "grid", "mirror"]
ALL = 0xFFFFFFFF
_cache = {}


class _Wide:
    """A _Scene widened on the device into 0xAB-filled buffers, checked against the spec's bytes on the way."""

    def __init__(self, s):
        self.s = s
        pool = s.pool
        cap = nt.pool_widen_capacity(pool["ranges"])
        assert cap == sum(128 * (r[1] // 64) for r in pool["ranges"])
        self.d_wpool = _filled(cap + 128)
        self.wide_ranges, self.pool_res = nt.pool_widen(pool["ranges"], s.d_nodes.data_ptr(), pool["nodes"].size, self.d_wpool.data_ptr(), cap)
        self.wpool = nw.widen_pool(pool)
        raw = self.d_wpool.cpu().numpy()
        ext = self.pool_res.nodesBytes
        assert ext == self.wpool["stats"]["nodesBytes"] and (raw[ext:] == 0xAB).all(), "bytes beyond the wide pool's extent were written"
        assert raw[:ext].tobytes() == self.wpool["nodes"].tobytes()
        assert self.wide_ranges == self.wpool["ranges"]
        st = self.wpool["stats"]
        r = self.pool_res
        assert (r.numNodes, list(r.counts), r.numLeafLinks, r.height, r.stackBound) == \
            (st["numNodes"], st["counts"], st["numLeafLinks"], st["height"], st["stackBound"]) and r.seconds > 0
        self.wpool_bytes = ext
        self.widen_tlas()

    def widen_tlas(self):
        s = self.s
        tcap = nt.bvh_widen_capacity(s.res.nodesBytes) if s.res.rootLink == 0 else 0
        self.d_wtlas, self.d_wrec = _filled(tcap + 128), _filled(64 * s.n + 64)
        self.res = nt.tlas_widen(s.n, s.d_inst.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes, s.res.rootLink, s.pool["ranges"],
                                 self.wide_ranges, self.d_wtlas.data_ptr(), tcap, self.d_wrec.data_ptr(), 64 * s.n)
        self.wt = nw.widen_tlas(s.tlas, s.res.rootLink, s.inst, s.pool["ranges"], self.wpool["ranges"])
        raw_t, raw_r = self.d_wtlas.cpu().numpy(), self.d_wrec.cpu().numpy()
        r, st = self.res, self.wt["stats"]
        assert r.nodesBytes == 128 * st["numNodes"] and r.recordsBytes == 64 * s.n
        assert (raw_t[r.nodesBytes:] == 0xAB).all() and (raw_r[r.recordsBytes:] == 0xAB).all(), "bytes beyond the extents were written"
        assert raw_t[:r.nodesBytes].tobytes() == self.wt["nodes"].tobytes()
        assert raw_r[:r.recordsBytes].tobytes() == self.wt["records"].tobytes()
        assert (r.numNodes, list(r.counts), r.numLeafLinks, r.height, r.tlasStackBound, r.stackBound) == \
            (st["numNodes"], st["counts"], st["numLeafLinks"], st["height"], st["tlasStackBound"], st["stackBound"])
        return self

    def args(self, d_rays, d_res, d_ids, n, any_hit, tlas=None, rec=None):
        s = self.s
        return (n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), (self.d_wtlas if tlas is None else tlas).data_ptr(), self.res.nodesBytes,
                s.res.rootLink, (self.d_wrec if rec is None else rec).data_ptr(), s.n, self.d_wpool.data_ptr(), self.wpool_bytes, s.d_woop.data_ptr(),
                s.pool["woop"].size, s.d_idx.data_ptr())


def _named(name):
    if name not in _cache:
        sc = isc.scene(name)
        _cache[name] = _Wide(_Scene(isc.pool_of(sc["names"]), ni.instances(sc["transforms"], sc["blas"])))
    return _cache[name]


def _rays():
    if "rays" not in _cache:
        _cache["rays"] = isc.scene_rays()
    return _cache["rays"]


def _parity(n):
    return np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)


def _launch(w, rays, any_hit, inst_masks=None, ray_masks=None, ray_mask=ALL, how="wide", null_vis=False, tlas=None, rec=None):
    """-> (results as bytes, instance ids as bytes, stats or None); how: 'wide' or 'stats'."""
    n = rays.shape[0]
    d_rays = up(rays)
    d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
    d_M = up(np.asarray(inst_masks, np.uint32)) if inst_masks is not None else None
    d_m = up(np.asarray(ray_masks, np.uint32)) if ray_masks is not None else None
    vis = None if null_vis else nt.InstanceVisibility(d_M.data_ptr() if d_M is not None else 0, d_m.data_ptr() if d_m is not None else 0, ray_mask)
    args = w.args(d_rays, d_res, d_ids, n, any_hit, tlas, rec)
    st = nt.trace_instanced_wide_stats(*args, vis=vis) if how == "stats" else None
    if how != "stats":
        nt.trace_instanced_wide(*args, vis=vis)
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
    assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
    return res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st


def _spec(w, rays, any_hit, tlas=None, records=None, probe=None, **kw):
    rid, rt, ru, rv, rinst, c = nw.trace(w.wt["nodes"] if tlas is None else tlas, w.s.res.rootLink, w.wt["records"] if records is None else records,
                                         w.s.pool, w.wpool, rays, any_hit, probe=probe, **kw)
    rec = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    rec["id"], rec["t"], rec["padA"], rec["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return rec.tobytes(), rinst.astype(np.int32).tobytes(), c


def _assert_equals_spec(w, rays, what, counters=False, probe=None, **kw):
    """Both hit modes: the launch equals the spec in every byte; with counters, so does the instrumented launch, counters too."""
    out = {}
    for any_hit in (False, True):
        want = _spec(w, rays, any_hit, probe=probe, **kw)
        got = _launch(w, rays, any_hit, **kw)
        for name, g, e, dt in (("record", got[0], want[0], np.uint32), ("instance", got[1], want[1], np.int32)):
            if g != e:
                g, e = np.frombuffer(g, dt), np.frombuffer(e, dt)
                bad = np.flatnonzero(g != e)
                raise AssertionError("%s anyHit=%d: %d %s words differ, first at word %d: %r != %r" % (what, any_hit, bad.size, name, bad[0], g[bad[0]], e[bad[0]]))
        if counters:
            res, ids, st = _launch(w, rays, any_hit, how="stats", **kw)
            assert res == got[0] and ids == got[1], (what, any_hit, "the instrumented kernel's records differ")
            assert st.as_dict() == want[2], (what, any_hit, st.as_dict(), want[2])
            assert st.algorithmic_bytes(kw.get("inst_masks") is not None, kw.get("ray_masks") is not None) == \
                nw.algorithmic_bytes(want[2], kw.get("inst_masks") is not None, kw.get("ray_masks") is not None)
        out[any_hit] = want
    return out


# ---- widening ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_widening_equals_the_spec_on_the_scenes(name):
    w = _named(name)            # (_Wide compares every byte, extent and statistic)
    assert w.res.stackBound <= 104 and w.res.numNodes >= 1


def test_widening_a_pool_with_gaps():
    pool = isc.pool_of(["one", "nested90", "soup64"], gap_nodes=2, gap_rows=1)
    inst = ni.instances(isc.seeded_transforms(5, 3, spread=4.0), [0, 1, 2, 1, 0])
    w = _Wide(_Scene(pool, inst))
    assert [r[0] for r in w.wide_ranges] == [0, 128, 128 + w.wide_ranges[1][1]] and w.wide_ranges[1][3] == 89
    assert w.res.stackBound == w.res.tlasStackBound + 1 + 89
    # an instance of a BLAS that is not there: extent 0, byte for byte the spec's record
    inst2 = inst.copy()
    inst2["blas"][3] = 9
    w.s.inst = inst2
    w.s.d_inst = up(inst2)
    w.widen_tlas()
    assert tuple(w.wt["records"][3, 12:16]) == (0, 0, 0, 0)
    rays = isc.scene_rays((16, 16), 256)
    out = _assert_equals_spec(w, rays, "an instance without a BLAS", counters=True)
    assert not (np.frombuffer(out[False][1], np.int32) == 3).any()


@pytest.mark.parametrize("n", [1, 2, 3, 65, 1025])
def test_widening_n_instances_of_one_blas(n):
    key = "soup64pool"
    if key not in _cache:
        _cache[key] = isc.pool_of(["soup64"])
    w = _Wide(_Scene(_cache[key], ni.instances(isc.seeded_transforms(n, 100 + n, spread=10.0), [0] * n)))
    assert (w.res.numNodes == 0) == (n == 1) and w.res.numLeafLinks == (0 if n == 1 else n)
    rays = isc.scene_rays((16, 8), 128)
    _assert_equals_spec(w, rays, "%d instances" % n, counters=True)


# ---- trace ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_trace_equals_the_spec_on_the_scenes_with_counters(name):
    w = _named(name)
    out = _assert_equals_spec(w, _rays(), name, counters=True)
    c = out[False][2]
    assert c["numHits"] > 500 and c["numTopInnerVisits"] > 0 and c["numInstancesMasked"] == 0
    # vis == NULL launches the same kernel
    assert _launch(w, _rays(), False, null_vis=True)[:2] == out[False][:2]
    print("%s: %r, %d algorithmic bytes" % (name, c, nw.algorithmic_bytes(c)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ray_counts(n):
    w = _named("three")
    _assert_equals_spec(w, isc.scene_rays((8, 8), 1000)[:n], "%d rays" % n, counters=(n == 65))


def test_odd_rays_through_one_identity_instance():
    w = _Wide(_Scene(isc.pool_of(["soup1000"]), ni.instances([ni.IDENTITY], [0])))
    assert w.s.res.rootLink == -1 and w.res.nodesBytes == 0 and w.res.stackBound == 1 + w.pool_res.stackBound
    for rays, what in ((isc.odd_rays(), "odd"), (isc.finite_edge_rays(), "edge")):
        out = _assert_equals_spec(w, rays, what + " rays", counters=True)
        assert out[False][2]["numTopInnerVisits"] == 0


def test_a_deep_blas_instanced_twice_uses_the_scratch_part_of_the_stack():
    pool = isc.pool_of(["nested90"])
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0)), isc.transform(isc.rotation(np.random.default_rng(8)), 1.0, (0.25, 0.25, 0))])
    w = _Wide(_Scene(pool, ni.instances(tf, [0, 0])))
    assert w.res.stackBound == 1 + 1 + 89
    rng = np.random.default_rng(2)
    rays = scenes.random_rays(1000, 6, extent=1.0)
    for k in ("ox", "oy", "oz"):
        rays[k] = (rng.uniform(0, 1, 1000) ** 8 * 4.0).astype(F)   # most origins near the small end of the chain
    rays["oz"] -= F(2.0)
    rays["dx"], rays["dy"], rays["dz"] = rng.normal(0, 0.1, 1000).astype(F), rng.normal(0, 0.1, 1000).astype(F), F(1.0)
    probe = {}
    out = _assert_equals_spec(w, rays, "nested", counters=True, probe=probe)
    assert probe["maxStack"] > 16, probe                 # some ray holds more than the 16 LDS entries: the scratch part runs
    assert out[False][2]["numHits"] > 0 and nt.trace_status() == 0


def test_masks_on_the_grid():
    w = _named("grid")
    n = w.s.n
    rays = _rays()[:6000]
    r = np.arange(rays.shape[0])
    base = _spec(w, rays, False)
    for ray_mask in (1, 2):
        out = _assert_equals_spec(w, rays, "parity, ray mask %d" % ray_mask, counters=(ray_mask == 2), inst_masks=_parity(n), ray_mask=ray_mask)
        assert out[False][0] != base[0] and out[False][2]["numInstancesMasked"] > 0
    out = _assert_equals_spec(w, rays, "per-ray masks by lane", counters=True, inst_masks=_parity(n), ray_masks=(1 + r % 2).astype(np.uint32))
    assert out[False][2]["numInstancesMasked"] > 0 and out[False][2]["numHits"] > 0
    miss = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    miss["id"], miss["t"] = -1, rays["tmax"]
    out = _assert_equals_spec(w, rays, "rayMask 0", counters=True, ray_mask=0)
    assert out[False][0] == miss.tobytes() and out[False][1] == np.full(rays.shape[0], -1, np.int32).tobytes()
    assert out[False][2]["numInstanceEntries"] == 0 < out[False][2]["numInstancesMasked"]


def test_bad_links_and_offsets_read_zeros_and_miss():
    """The range checks at work: a record that points beyond the wide pool and a top-level link ~i with i >= numInstances end as the
    spec says -- the instance's node reads as zeros, the link is popped -- and the launch returns."""
    w = _named("three")
    rays = _rays()[:4096]
    good = _spec(w, rays, False)
    gids = np.frombuffer(good[1], np.int32)
    assert (gids == 1).sum() > 20 and (gids == 2).sum() > 20       # (the spec on the intact scene: enough rays for the two cases)
    rec = w.wt["records"].copy()
    rec[1, 12] = (w.wpool_bytes + 0x100000) & ~127                 # instance 1's wide BLAS: beyond the wide pool
    want = _spec(w, rays, False, records=rec)
    got = _launch(w, rays, False, rec=up(rec))
    assert got[:2] == want[:2] and not (np.frombuffer(got[1], np.int32) == 1).any()
    st = _launch(w, rays, False, rec=up(rec), how="stats")
    assert st[:2] == want[:2] and st[2].as_dict() == want[2]
    tl = w.wt["nodes"].copy()
    links = tl[:, 12:16]
    assert (links == ~2).sum() == 1
    links[links == ~2] = ~(w.s.n + 5)                              # instance 2's leaf link: no such instance
    want = _spec(w, rays, False, tlas=tl)
    got = _launch(w, rays, False, tlas=up(tl))
    assert got[:2] == want[:2] and not (np.frombuffer(got[1], np.int32) == 2).any() and (np.frombuffer(got[1], np.int32) >= 0).any()


def test_a_captured_launch_replays_to_the_same_bytes():
    w = _named("mirror")
    rays = _rays()[:4096]
    n = rays.shape[0]
    d_rays, d_res, d_ids = up(rays), _filled(16 * n + 64), _filled(4 * n + 64)
    want = _spec(w, rays, False)
    stream = torch.cuda.Stream()                         # a fresh stream, a single linear branch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        nt.trace_instanced_wide(*w.args(d_rays, d_res, d_ids, n, False), stream=torch.cuda.current_stream().cuda_stream, timed=False)
        errs = []
        try:                                             # the blocking forms are refused while capturing, and launch nothing
            nt.trace_instanced_wide_stats(*w.args(d_rays, d_res, d_ids, n, False), stream=torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            errs.append(e.code)
        s = w.s
        for call in (lambda cs: nt.pool_widen(s.pool["ranges"], s.d_nodes.data_ptr(), s.pool["nodes"].size, w.d_wpool.data_ptr(),
                                              nt.pool_widen_capacity(s.pool["ranges"]), stream=cs),
                     lambda cs: nt.tlas_widen(s.n, s.d_inst.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes, s.res.rootLink, s.pool["ranges"],
                                              w.wide_ranges, w.d_wtlas.data_ptr(), nt.bvh_widen_capacity(s.res.nodesBytes), w.d_wrec.data_ptr(),
                                              64 * s.n, stream=cs)):
            try:
                call(torch.cuda.current_stream().cuda_stream)
            except nt.NtrError as e:
                errs.append(e.code)
    assert errs == [-1, -1, -1]
    for _ in range(2):
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all()
        assert res[:16 * n].tobytes() == want[0] and ids[:4 * n].tobytes() == want[1]
    assert nt.trace_status() == 0


def test_determinism_and_no_scratch_grows():
    w = _named("mirror")
    pools = (nt.tlas_scratch_bytes, nt.tlas_refit_scratch_bytes, nt.ploc_scratch_bytes, nt.bvh_refit_scratch_bytes, nt.bvh_widen_scratch_bytes)
    rays = _rays()[:4096]
    kw = dict(inst_masks=_parity(w.s.n))
    a = _launch(w, rays, False, **kw)
    held = [f() for f in pools]
    n = rays.shape[0]
    d_rays, d_res, d_ids = up(rays), _filled(16 * n + 64), _filled(4 * n + 64)
    for _ in range(20):
        nt.trace_instanced_wide(*w.args(d_rays, d_res, d_ids, n, False), timed=False)
    torch.cuda.synchronize()
    assert [f() for f in pools] == held
    assert _launch(w, rays, False, **kw)[:2] == a[:2]
    sa, sb = _launch(w, rays, True, how="stats", **kw), _launch(w, rays, True, how="stats", **kw)
    assert sa[:2] == sb[:2] and sa[2].as_dict() == sb[2].as_dict()
    # the widening keeps its table in the widening pass's pool, which ntr_lbvh_release_workspace returns
    assert nt.bvh_widen_scratch_bytes() > 0
    nt.lbvh_release_workspace()
    assert nt.bvh_widen_scratch_bytes() == 0
