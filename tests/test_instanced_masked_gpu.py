"""Instance visibility masks and counters on the device: ntr_trace_instanced_masked equals the numpy spec (tests/np_instanced_masked.py)
in all four result words and the instance id, bit for bit, for closest hit and any hit; ntr_trace_instanced_stats gives the same bytes
and the spec's eight counters; the unmasked forms give ntr_trace_instanced's bytes; a captured launch reads the masks at replay time.
Output buffers are prefilled with 0xAB and nothing beyond the results may be written; the status word stays clear."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_masked as nm
from gpu_util import up
from test_instanced_gpu import _Scene, _filled

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ["three", "grid", "mirror"]
ALL = 0xFFFFFFFF
_cache = {}


def _named(name):
    if name not in _cache:
        sc = isc.scene(name)
        _cache[name] = _Scene(isc.pool_of(sc["names"]), ni.instances(sc["transforms"], sc["blas"]))
    return _cache[name]


def _rays():
    if "rays" not in _cache:
        _cache["rays"] = isc.scene_rays()
    return _cache["rays"]


def _parity(n):
    return np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)


def _random_words(n, seed):
    """Random 32-bit words, every fourth with only bit 31 set and every seventh zero."""
    w = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[::4] = 0x80000000
    w[3::7] = 0
    return w


def _launch(s, rays, any_hit, inst_masks=None, ray_masks=None, ray_mask=ALL, how="masked", null_vis=False, d_inst_masks=None):
    """-> (results as bytes, instance ids as bytes, stats or None); how: 'masked', 'stats' or 'old' (ntr_trace_instanced)."""
    n = rays.shape[0]
    d_rays = up(rays)
    d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
    d_M = d_inst_masks if d_inst_masks is not None else (up(np.asarray(inst_masks, np.uint32)) if inst_masks is not None else None)
    d_m = up(np.asarray(ray_masks, np.uint32)) if ray_masks is not None else None
    vis = None if null_vis else nt.InstanceVisibility(d_M.data_ptr() if d_M is not None else 0, d_m.data_ptr() if d_m is not None else 0, ray_mask)
    args = (n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes, s.res.rootLink,
            s.d_rec.data_ptr(), s.n, s.d_nodes.data_ptr(), s.pool["nodes"].size, s.d_woop.data_ptr(), s.pool["woop"].size, s.d_idx.data_ptr())
    st = None
    if how == "old":
        nt.trace_instanced(*args)
    elif how == "stats":
        st = nt.trace_instanced_stats(*args, vis=vis)
    else:
        nt.trace_instanced_masked(*args, vis=vis)
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
    assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
    return res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st


def _spec(s, rays, any_hit, **kw):
    rid, rt, ru, rv, rinst, c = nm.trace(s.tlas, s.res.rootLink, s.records, s.pool, rays, any_hit, **kw)
    rec = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    rec["id"], rec["t"], rec["padA"], rec["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    return rec.tobytes(), rinst.astype(np.int32).tobytes(), c


def _assert_equals_spec(s, rays, what, counters=False, **kw):
    """Both hit modes: the masked launch equals the spec in every byte; with counters, so does the instrumented launch, counters too."""
    out = {}
    for any_hit in (False, True):
        want = _spec(s, rays, any_hit, **kw)
        got = _launch(s, rays, any_hit, **kw)
        for name, g, e, dt in (("record", got[0], want[0], np.uint32), ("instance", got[1], want[1], np.int32)):
            if g != e:
                g, e = np.frombuffer(g, dt), np.frombuffer(e, dt)
                bad = np.flatnonzero(g != e)
                raise AssertionError("%s anyHit=%d: %d %s words differ, first at word %d: %r != %r" % (what, any_hit, bad.size, name, bad[0], g[bad[0]], e[bad[0]]))
        if counters:
            res, ids, st = _launch(s, rays, any_hit, how="stats", **kw)
            assert res == got[0] and ids == got[1], (what, any_hit, "the instrumented kernel's records differ")
            assert st.as_dict() == want[2], (what, any_hit, st.as_dict(), want[2])
        out[any_hit] = want
    return out


# ---- scenes and masks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_parity_masks_on_the_scenes_with_counters(name):
    s = _named(name)
    M = _parity(s.n)
    base = _assert_equals_spec(s, _rays(), name + " unmasked", counters=True)
    for ray_mask in (1, 2, 3, 0x80000000):
        w = _assert_equals_spec(s, _rays(), "%s parity, ray mask %#x" % (name, ray_mask), counters=ray_mask in (2, 0x80000000), inst_masks=M, ray_mask=ray_mask)
        c = w[False][2]
        if ray_mask == 3:
            assert w[False][0] == base[False][0] and c["numInstancesMasked"] == 0
        if ray_mask == 0x80000000:       # nothing visible: no ray pays a bottom-level step
            assert c["numInstanceEntries"] == c["numInnerVisits"] == c["numTriTests"] == c["numLeafVisits"] == c["numHits"] == 0 < c["numInstancesMasked"]
        if ray_mask in (1, 2):
            assert w[False][0] != base[False][0] and c["numInstancesMasked"] > 0
    st = _launch(s, _rays(), False, inst_masks=M, ray_mask=2, how="stats")[2]
    print("%s, parity masks, ray mask 2: %r, %d algorithmic bytes" % (name, st.as_dict(), st.algorithmic_bytes(instance_masks=True)))


@pytest.mark.parametrize("name", SCENES)
def test_random_mask_words_on_the_scenes(name):
    s = _named(name)
    M = _random_words(s.n, 40 + s.n)
    M[0] = 0x80000000                    # only bit 31
    for ray_mask in (1, 2, 3, 0x80000000):
        _assert_equals_spec(s, _rays(), "%s random words, ray mask %#x" % (name, ray_mask), counters=ray_mask == 0x80000000, inst_masks=M, ray_mask=ray_mask)


# ---- per-ray masks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_per_ray_masks_by_lane_by_wave_and_random(n):
    """One wave makes both decisions at once: lanes that enter beside lanes that are refused, under one fetch."""
    s = _named("three")
    rays = isc.scene_rays((8, 8), 1000)[:n]
    r = np.arange(n)
    for what, m in (("by lane", 1 + r % 2), ("by wave", 1 + (r // 64) % 2), ("random", _random_words(n, n))):
        for M, which in ((_parity(s.n), "parity"), (_random_words(s.n, 7), "random"), (None, "none")):
            _assert_equals_spec(s, rays, "%d rays, ray masks %s, instance masks %s" % (n, what, which), counters=(what == "by lane"),
                                inst_masks=M, ray_masks=m.astype(np.uint32))


def test_per_ray_masks_on_the_grid():
    s = _named("grid")
    r = np.arange(_rays().shape[0])
    w = _assert_equals_spec(s, _rays(), "grid by lane", counters=True, inst_masks=_parity(s.n), ray_masks=(1 + r % 2).astype(np.uint32))
    assert w[False][2]["numInstancesMasked"] > 0 and w[False][2]["numHits"] > 0


# ---- all or nothing -------------------------------------------------------------------------------------------------------------------
def test_all_or_nothing():
    s = _named("grid")
    rays = _rays()[:3000]
    miss = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
    miss["id"], miss["t"] = -1, rays["tmax"]
    for kw in (dict(inst_masks=np.zeros(s.n, np.uint32)), dict(ray_mask=0), dict(inst_masks=_parity(s.n), ray_masks=np.zeros(rays.shape[0], np.uint32))):
        w = _assert_equals_spec(s, rays, "nothing visible", counters=True, **kw)
        assert w[False][0] == miss.tobytes() and w[False][1] == np.full(rays.shape[0], -1, np.int32).tobytes()
    # N = 1: rootLink = ~0, no top-level node
    one = _Scene(isc.pool_of(["soup1000"]), ni.instances([isc.transform(np.eye(3), 1.0, (0.5, 0, 0))], [0]))
    assert one.res.rootLink == -1
    for M, hits in ((np.array([0], np.uint32), False), (np.array([0x80000000], np.uint32), True), (np.array([4], np.uint32), False)):
        w = _assert_equals_spec(one, rays, "N = 1", counters=True, inst_masks=M, ray_mask=0x80000001)
        c = w[False][2]
        assert (c["numHits"] > 0) == hits and c["numTopInnerVisits"] == 0
        assert (c["numInstanceEntries"], c["numInstancesMasked"]) == ((c["numRays"], 0) if hits else (0, c["numRays"]))


# ---- unmasked equals old ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_unmasked_forms_give_the_old_entry_points_bytes(name):
    s = _named(name)
    n = _rays().shape[0]
    for any_hit in (False, True):
        old = _launch(s, _rays(), any_hit, how="old")[:2]
        assert _launch(s, _rays(), any_hit, null_vis=True)[:2] == old                      # vis == NULL
        assert _launch(s, _rays(), any_hit)[:2] == old                                     # two NULLs and rayMask 0xFFFFFFFF
        assert _launch(s, _rays(), any_hit, inst_masks=np.full(s.n, ALL, np.uint32), ray_masks=np.full(n, ALL, np.uint32))[:2] == old
        assert _launch(s, _rays(), any_hit, inst_masks=np.full(s.n, ALL, np.uint32))[:2] == old
        assert _launch(s, _rays(), any_hit, how="stats", null_vis=True)[:2] == old


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
def test_hiding_the_twin_that_wins_the_tie_names_the_other_with_the_same_t():
    pool = isc.pool_of(["soup1000"])
    s = _Scene(pool, ni.instances(np.tile(isc.transform(np.eye(3), 1.0, (0.5, 0, 0)), (2, 1)), [0, 0]))
    rays = isc.scene_rays((64, 32), 1024)
    old_res, old_ids, _ = _launch(s, rays, False, how="old")
    ids = np.frombuffer(old_ids, np.int32)
    assert (ids >= 0).any() and (ids[ids >= 0] == 0).all()
    M = np.array([2, 1], np.uint32)                      # hide instance 0, the one the unmasked trace reports
    w = _assert_equals_spec(s, rays, "twins", counters=True, inst_masks=M, ray_mask=1)
    assert w[False][0] == old_res                                                           # the same records: id, t, u and v bits
    assert np.array_equal(np.frombuffer(w[False][1], np.int32), np.where(ids >= 0, 1, -1))


# ---- deep stack ---------------------------------------------------------------------------------------------------------------------------
def test_a_deep_blas_instanced_twice_with_the_first_instance_hidden():
    pool = isc.pool_of(["nested90"])
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0)), isc.transform(isc.rotation(np.random.default_rng(8)), 1.0, (0.25, 0.25, 0))])
    s = _Scene(pool, ni.instances(tf, [0, 0]))
    rng = np.random.default_rng(2)
    rays = scenes.random_rays(1000, 6, extent=1.0)
    for k in ("ox", "oy", "oz"):
        rays[k] = (rng.uniform(0, 1, 1000) ** 8 * 4.0).astype(F)   # most origins near the small end of the chain
    rays["oz"] -= F(2.0)
    rays["dx"], rays["dy"], rays["dz"] = rng.normal(0, 0.1, 1000).astype(F), rng.normal(0, 0.1, 1000).astype(F), F(1.0)
    w = _assert_equals_spec(s, rays, "nested", counters=True, inst_masks=np.array([1, 2], np.uint32), ray_mask=2)
    ids = np.frombuffer(w[False][1], np.int32)
    assert (ids == 1).any() and not (ids == 0).any()
    assert nt.trace_status() == 0                        # no overflow bit (every _launch asserts it too)


# ---- counters: the empty launch and a capturing stream ------------------------------------------------------------------------------------
def test_stats_of_an_empty_launch_and_on_a_capturing_stream():
    s = _named("three")
    rays = _rays()[:256]
    d_rays, d_res, d_ids, d_M = up(rays), _filled(16 * 256), _filled(4 * 256), up(_parity(s.n))
    vis = nt.InstanceVisibility(d_M.data_ptr(), 0, 2)
    args = (d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes, s.res.rootLink,
            s.d_rec.data_ptr(), s.n, s.d_nodes.data_ptr(), s.pool["nodes"].size, s.d_woop.data_ptr(), s.pool["woop"].size, s.d_idx.data_ptr())
    st = nt.InstancedTraceStats()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert nt.lib().ntr_trace_instanced_stats(0, 0, *args, C.byref(vis), C.byref(st), None) == 0 and bytes(st) == bytes(64)
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=stream):
        cs = torch.cuda.current_stream().cuda_stream
        d_ids.fill_(0xAB)   # so that the graph is not empty
        try:
            nt.trace_instanced_stats(256, False, *args, vis=vis, stream=cs)
        except nt.NtrError as e:
            errs.append(e.code)
    assert errs == [-1]
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0xAB).all()           # the refused call launched nothing
    assert nt.trace_instanced_stats(256, False, *args, vis=vis).numRays == 256   # and the stream's end leaves the call usable


# ---- graph --------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_launch_reads_the_masks_at_replay_time():
    s = _named("grid")
    rays = _rays()[:4096]
    n = rays.shape[0]
    d_rays, d_res, d_ids = up(rays), _filled(16 * n + 64), _filled(4 * n + 64)
    first, second = _parity(s.n), _random_words(s.n, 3)
    d_M = up(first)
    vis = nt.InstanceVisibility(d_M.data_ptr(), 0, 1)
    stream = torch.cuda.Stream()                         # a fresh stream, a single linear branch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        nt.trace_instanced_masked(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes,
                                  s.res.rootLink, s.d_rec.data_ptr(), s.n, s.d_nodes.data_ptr(), s.pool["nodes"].size, s.d_woop.data_ptr(),
                                  s.pool["woop"].size, s.d_idx.data_ptr(), vis=vis, stream=torch.cuda.current_stream().cuda_stream, timed=False)
    got = []
    for M in (first, second):
        d_M.copy_(up(M))
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all()
        want = _spec(s, rays, False, inst_masks=M, ray_mask=1)
        assert res[:16 * n].tobytes() == want[0] and ids[:4 * n].tobytes() == want[1]
        got.append(want[0])
    assert got[0] != got[1] and nt.trace_status() == 0


# ---- determinism and scratch ----------------------------------------------------------------------------------------------------------------
def test_determinism_and_no_scratch_grows():
    s = _named("mirror")
    pools = (nt.tlas_scratch_bytes, nt.tlas_refit_scratch_bytes, nt.ploc_scratch_bytes, nt.bvh_refit_scratch_bytes)
    held = [f() for f in pools]
    kw = dict(inst_masks=_parity(s.n), ray_masks=_random_words(_rays().shape[0], 9))
    a, b = _launch(s, _rays(), False, **kw), _launch(s, _rays(), False, **kw)
    assert a[:2] == b[:2]
    sa, sb = _launch(s, _rays(), True, how="stats", **kw), _launch(s, _rays(), True, how="stats", **kw)
    assert sa[:2] == sb[:2] and sa[2].as_dict() == sb[2].as_dict()
    assert [f() for f in pools] == held
