"""The seeded two-level trace on the device: ntr_trace_instanced_seeded and ntr_trace_instanced_wide_seeded equal the numpy spec
(tests/np_instanced_seeded.py) in all four result words and the instance id, closest hit and any hit, whether the seed comes from
ntr_trace_bvh on the world BLAS's range of the pool or is uploaded; the _stats forms give the same bytes and the spec's counters; in
place equals out of place; an all-miss seed gives the unseeded kernels' bytes; hostile seed words are taken as they are; world trace,
seeded trace and hit attributes replay as one graph.  Output buffers are prefilled with 0xAB and nothing beyond the extents may be
written; the status word stays clear."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_frame as nf
import np_instanced_seeded as nsd
import seeded_scenes as sds
from gpu_util import up
from test_instanced_frame_cpu import geometry
from test_instanced_gpu import _Scene, _filled
from test_instanced_wide_gpu import _Wide

pytestmark = pytest.mark.gpu

F = np.float32
ALL = 0xFFFFFFFF
KERNEL = "fermi_speculative_while_while"
FORMS = ["binary", "wide"]
_cache = {}


class _World:
    """A seeded_scenes scene on the device: the pool, the top-level tree over the N instances built and widened on the device (and
    compared with the specs on the way), and the world BLAS's range of the pool as ntr_trace_bvh takes it."""

    def __init__(self, sc, inst=None):
        self.sc = sc
        self.s = _Scene(sc["pool"], sc["inst"] if inst is None else inst)
        self.w = _Wide(self.s)
        self.n = self.s.n
        n_off, n_bytes, w_off, w_bytes = sc["pool"]["ranges"][sc["world"]]
        self.world_args = (self.s.d_nodes.data_ptr() + n_off, n_bytes, self.s.d_woop.data_ptr() + w_off, w_bytes,
                           self.s.d_idx.data_ptr() + 4 * (w_off // 16))

    def trace_world(self, n, any_hit, d_rays, d_seed, stream=0):
        nt.trace_bvh(KERNEL, n, any_hit, d_rays.data_ptr(), d_seed.data_ptr(), *self.world_args, stream=stream, timed=False)

    def args(self, form, n, any_hit, d_rays, d_seed, seed_instance, d_res, d_ids):
        """The seeded entry points' positional arguments."""
        s = self.s
        head = (n, any_hit, d_rays.data_ptr(), d_seed.data_ptr(), seed_instance, d_res.data_ptr(), d_ids.data_ptr())
        if form == "binary":
            return head + (s.d_tlas.data_ptr(), s.res.nodesBytes, s.res.rootLink, s.d_rec.data_ptr(), s.n, s.d_nodes.data_ptr(), s.pool["nodes"].size,
                           s.d_woop.data_ptr(), s.pool["woop"].size, s.d_idx.data_ptr())
        return head + self.w.args(d_rays, d_res, d_ids, n, any_hit)[5:]

    def spec(self, form, seed, seed_instance, rays, any_hit, **kw):
        """-> (records as bytes, instance ids as bytes, counters)"""
        s, w = self.s, self.w
        if form == "binary":
            out = nsd.trace(seed, seed_instance, s.tlas, s.res.rootLink, s.records, s.pool, rays, any_hit, **kw)
        else:
            out = nsd.trace_wide(seed, seed_instance, w.wt["nodes"], s.res.rootLink, w.wt["records"], s.pool, w.wpool, rays, any_hit, **kw)
        words = np.stack([np.ascontiguousarray(x).view(np.uint32) for x in out[:4]], axis=1)
        return words.tobytes(), out[4].astype(np.int32).tobytes(), out[5]


def _world(name="world"):
    if name not in _cache:
        _cache[name] = _World(sds.world_scene() if name == "world" else sds.three_scene())
    return _cache[name]


def _launch(wd, form, rays, any_hit, seed, seed_instance, how="trace", in_place=False, inst_masks=None, ray_masks=None, ray_mask=ALL, null_vis=False):
    """seed: (n, 4) uint32 words to upload, or None: ntr_trace_bvh of the world BLAS writes the seed on the device.
    -> (records as bytes, instance ids as bytes, stats or None, the seed words the launch started from)"""
    n = rays.shape[0]
    d_rays = up(rays)
    d_seed = _filled(16 * n + 64)
    if seed is None:
        wd.trace_world(n, any_hit, d_rays, d_seed)
        torch.cuda.synchronize()
        seed = d_seed.cpu().numpy()[:16 * n].view(np.uint32).reshape(-1, 4).copy()
    else:
        d_seed[:16 * n] = up(seed)
    d_res = d_seed if in_place else _filled(16 * n + 64)
    d_ids = _filled(4 * n + 64)
    d_M = up(np.asarray(inst_masks, np.uint32)) if inst_masks is not None else None
    d_m = up(np.asarray(ray_masks, np.uint32)) if ray_masks is not None else None
    vis = None if null_vis else nt.InstanceVisibility(d_M.data_ptr() if d_M is not None else 0, d_m.data_ptr() if d_m is not None else 0, ray_mask)
    fn = {("binary", "trace"): nt.trace_instanced_seeded, ("binary", "stats"): nt.trace_instanced_seeded_stats,
          ("wide", "trace"): nt.trace_instanced_wide_seeded, ("wide", "stats"): nt.trace_instanced_wide_seeded_stats}[form, how]
    st = fn(*wd.args(form, n, any_hit, d_rays, d_seed, seed_instance, d_res, d_ids), vis=vis)
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    res, ids, sd = d_res.cpu().numpy(), d_ids.cpu().numpy(), d_seed.cpu().numpy()
    assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all() and (sd[16 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
    if not in_place:
        assert sd[:16 * n].tobytes() == seed.tobytes(), "the seed buffer was written"
    return res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st if how == "stats" else None, seed


def _assert_same(got, want, what):
    for name, g, e, dt in (("record", got[0], want[0], np.uint32), ("instance", got[1], want[1], np.int32)):
        if g != e:
            g, e = np.frombuffer(g, dt), np.frombuffer(e, dt)
            bad = np.flatnonzero(g != e)
            raise AssertionError("%s: %d %s words differ, first at word %d: %r != %r" % (what, bad.size, name, bad[0], g[bad[0]], e[bad[0]]))


def _assert_equals_spec(wd, form, rays, seed, seed_instance, what, counters=False, **kw):
    """Both hit modes: the launch equals the spec in every byte; with counters, so does the instrumented launch, counters too.
    seed: words, None (the device's world trace) or a function of any_hit."""
    out = {}
    masks = (kw.get("inst_masks") is not None, kw.get("ray_masks") is not None)
    for any_hit in (False, True):
        sd = seed(any_hit) if callable(seed) else seed
        got = _launch(wd, form, rays, any_hit, sd, seed_instance, **kw)
        want = wd.spec(form, got[3], seed_instance, rays, any_hit, **kw)
        _assert_same(got, want, "%s %s anyHit=%d" % (what, form, any_hit))
        if counters:
            st = _launch(wd, form, rays, any_hit, got[3], seed_instance, how="stats", **kw)
            assert st[:2] == got[:2], (what, form, any_hit, "the instrumented kernel's records differ")
            assert st[2].as_dict() == want[2], (what, form, any_hit, st[2].as_dict(), want[2])
            spec_bytes = nsd.algorithmic_bytes if form == "binary" else nsd.algorithmic_bytes_wide
            assert st[2].algorithmic_bytes(*masks) + 16 * rays.shape[0] == spec_bytes(want[2], *masks)
        out[any_hit] = (got, want)
    return out


def _random_words(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


# ---- device against spec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["world", "three"])
def test_world_trace_then_seeded_trace_equals_the_spec(name, form):
    """ntr_trace_bvh on the world BLAS's range of the pool, then the seeded call: world-hit rays are compared on the seed's own words,
    whatever ntr_trace_bvh wrote there."""
    wd, rays = _world(name), sds.rays()
    out = _assert_equals_spec(wd, form, rays, None, wd.n, name + ", device seed", counters=True)
    for any_hit in (False, True):
        got, want = out[any_hit]
        seed = got[3]
        spec_seed = sds.world_seed(wd.sc, rays, any_hit)
        assert np.array_equal(seed[:, :2], spec_seed[:, :2])             # the world trace is the single-level spec's, id and t
        ids = np.frombuffer(got[1], np.int32)
        assert (ids == wd.n).sum() > 100 and ((ids >= 0) & (ids < wd.n)).sum() > 50 and (ids == -1).sum() > 100
        kept = ids == wd.n
        assert np.array_equal(np.frombuffer(got[0], np.uint32).reshape(-1, 4)[kept], seed[kept])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["world", "three"])
def test_uploaded_seed_equals_the_spec(name, form):
    wd, rays = _world(name), sds.rays()
    n = rays.shape[0]

    def seed(any_hit):                                   # the spec's world trace with two words that are nobody's floats
        s = sds.world_seed(wd.sc, rays, any_hit)
        s[:, 2], s[:, 3] = _random_words(n, 31), _random_words(n, 32)
        return s
    out = _assert_equals_spec(wd, form, rays, seed, wd.n, name + ", uploaded seed", counters=True)
    # vis == NULL launches the same kernel
    got, _ = out[False]
    assert _launch(wd, form, rays, False, got[3], wd.n, null_vis=True)[:2] == got[:2]


@pytest.mark.parametrize("form", FORMS)
def test_in_place_equals_out_of_place(form):
    wd, rays = _world(), sds.rays()
    for any_hit in (False, True):
        for how in ("trace", "stats"):
            a = _launch(wd, form, rays, any_hit, None, wd.n, how=how)
            b = _launch(wd, form, rays, any_hit, None, wd.n, how=how, in_place=True)
            assert a[:2] == b[:2] and a[3].tobytes() == b[3].tobytes(), (form, any_hit, how)
            assert how == "trace" or a[2].as_dict() == b[2].as_dict()


@pytest.mark.parametrize("form", FORMS)
def test_an_all_miss_seed_gives_the_unseeded_kernels_bytes(form):
    wd, rays = _world(), sds.rays()
    n = rays.shape[0]
    s = wd.s
    d_rays = up(rays)
    for any_hit in (False, True):
        for vis in (None, nt.InstanceVisibility(0, 0, 0x5)):
            d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
            if form == "binary":
                nt.trace_instanced_masked(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_tlas.data_ptr(), s.res.nodesBytes,
                                          s.res.rootLink, s.d_rec.data_ptr(), s.n, s.d_nodes.data_ptr(), s.pool["nodes"].size, s.d_woop.data_ptr(),
                                          s.pool["woop"].size, s.d_idx.data_ptr(), vis=vis)
            else:
                nt.trace_instanced_wide(*wd.w.args(d_rays, d_res, d_ids, n, any_hit), vis=vis)
            torch.cuda.synchronize()
            want = d_res.cpu().numpy()[:16 * n].tobytes(), d_ids.cpu().numpy()[:4 * n].tobytes()
            got = _launch(wd, form, rays, any_hit, sds.miss_seed(rays), 9, ray_mask=ALL if vis is None else 0x5)
            _assert_same(got, want, "all-miss seed %s anyHit=%d" % (form, any_hit))


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_one_instance_has_no_top_level_node(form):
    if "one" not in _cache:
        sc = sds.world_scene()
        _cache["one"] = _World(sc, inst=sc["inst"][24:25])              # one soup64 instance: rootLink == ~0
    wd = _cache["one"]
    assert wd.n == 1 and wd.s.res.rootLink == -1
    rays = np.concatenate([sds.rays()[:3877], isc.odd_rays()])           # 4 096 + 37 rays: the last workgroup is part empty
    assert rays.shape[0] == 4096 + 37
    out = _assert_equals_spec(wd, form, rays, None, 1, "one instance", counters=True)
    assert out[False][1][2]["numTopInnerVisits"] == 0 and out[False][1][2]["numInstanceEntries"] > 0


@pytest.mark.parametrize("form", FORMS)
def test_odd_rays_and_a_ragged_ray_count(form):
    wd = _world()
    odd = isc.odd_rays()
    _assert_equals_spec(wd, form, odd, None, wd.n, "odd rays", counters=True)
    rays = sds.rays()[:4096 + 37]
    _assert_equals_spec(wd, form, rays, None, wd.n, "4 096 + 37 rays")
    for n in (1, 63, 65):
        _assert_equals_spec(wd, form, rays[2048:2048 + n], None, wd.n, "%d rays" % n)


@pytest.mark.parametrize("form", FORMS)
def test_masks_compose_with_seeding(form):
    wd, rays = _world(), sds.rays()
    n = wd.n
    inst_masks = np.where(np.arange(n) % 2 == 0, 0x80000001, 0x2).astype(np.uint32)
    ray_masks = np.where(np.arange(rays.shape[0]) % 3 == 0, 0x80000000, 0x3).astype(np.uint32)
    ray_masks[np.arange(rays.shape[0]) % 7 == 0] = 0x4                   # rays that every instance refuses: their seed stays
    out = _assert_equals_spec(wd, form, rays, None, n, "per-ray masks", counters=True, inst_masks=inst_masks, ray_masks=ray_masks)
    got, want = out[False]
    ids = np.frombuffer(got[1], np.int32)
    refused = ray_masks == 0x4
    assert want[2]["numInstancesMasked"] > 0 and want[2]["numInstanceEntries"] > 0
    assert np.array_equal(np.frombuffer(got[0], np.uint32).reshape(-1, 4)[refused], got[3][refused])
    assert np.array_equal(ids[refused], np.where(got[3][refused, 0].view(np.int32) != -1, n, -1))
    out = _assert_equals_spec(wd, form, rays, None, n, "ray mask 2", counters=True, inst_masks=inst_masks, ray_mask=0x2)
    ids = np.frombuffer(out[False][0][1], np.int32)
    real = (ids >= 0) & (ids < n)
    assert real.sum() > 20 and (ids[real] % 2 == 1).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seed_instance", [-2, 32, 2 ** 31 - 1])
def test_the_seed_instance_is_stored_verbatim(form, seed_instance):
    wd, rays = _world(), sds.rays()[:2048 + 37]
    assert wd.n == 32
    out = _assert_equals_spec(wd, form, rays, None, seed_instance, "seedInstance %d" % seed_instance)
    got = out[False][0]
    ids = np.frombuffer(got[1], np.int32)
    world = got[3][:, 0].view(np.int32) != -1
    assert (ids == seed_instance).sum() > 50 and not (ids[~world] == seed_instance).any()


@pytest.mark.parametrize("form", FORMS)
def test_hostile_seed_words_are_taken_as_they_are(form):
    """Well-defined behaviour, not a provocation: the seed's t only ever enters one comparison and the box and triangle tests as tmax,
    its id is only ever compared with -1, and w2, w3 are copied.  NaN, infinities, negative t, id = INT_MIN: the result is the spec's
    and nothing beyond the buffers is written."""
    wd, rays = _world(), sds.rays()[:4096]
    n = rays.shape[0]
    ts = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 1e30, -0.0, 3.0e38], F)[np.arange(n) % 8]
    ids = np.where(np.arange(n) % 3 == 0, -1, np.where(np.arange(n) % 3 == 1, np.iinfo(np.int32).min, 7)).astype(np.int32)
    seed = nsd.seed_of(ids, ts, _random_words(n, 41), 0x7FC00001)
    seed[5::16, 1] = 0xFFC12345                                          # a NaN with a payload and a sign
    out = _assert_equals_spec(wd, form, rays, seed, -2 ** 31, "hostile seeds", counters=True)
    got, want = out[False]
    ids_out = np.frombuffer(got[1], np.int32)
    assert ((ids_out >= 0) & (ids_out < wd.n)).sum() > 20 and (ids_out == -2 ** 31).sum() > 500


# ---- one graph ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_world_trace_seeded_trace_and_attributes_replay_as_one_graph(form):
    wd, rays = _world(), sds.rays()[:4096 + 37]
    sc = wd.sc
    n = rays.shape[0]
    tri, pos, blas_tris = geometry(sc["names"])
    d_tri, d_pos, d_bt, d_inst = up(tri), up(pos), up(blas_tris), up(sc["inst_all"])     # the world's record appended: instance N
    geom = nt.InstancedGeometry(wd.n + 1, blas_tris.shape[0], tri.shape[0], pos.shape[0], d_inst.data_ptr(), d_bt.data_ptr(), d_tri.data_ptr(),
                                d_pos.data_ptr())
    d_rays = up(rays)
    d_res, d_ids, d_out, d_nrm = _filled(16 * n + 64), _filled(4 * n + 64), _filled(16 * n + 64), _filled(16 * n + 64)
    fn = nt.trace_instanced_seeded if form == "binary" else nt.trace_instanced_wide_seeded
    stats_fn = nt.trace_instanced_seeded_stats if form == "binary" else nt.trace_instanced_wide_seeded_stats

    def frame(cs):                                       # the seed buffer is the result buffer: the world trace rewrites it every time
        wd.trace_world(n, False, d_rays, d_res, stream=cs)
        fn(*wd.args(form, n, False, d_rays, d_res, wd.n, d_res, d_ids), stream=cs, timed=False)
        nt.instanced_hit_attributes(n, d_res.data_ptr(), d_ids.data_ptr(), geom, d_out.data_ptr(), d_nrm.data_ptr(), cs)

    def down():
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        bufs = [b.cpu().numpy() for b in (d_res, d_ids, d_out, d_nrm)]
        for b, e in zip(bufs, (16 * n, 4 * n, 16 * n, 16 * n)):
            assert (b[e:] == 0xAB).all()
        return [b[:e].tobytes() for b, e in zip(bufs, (16 * n, 4 * n, 16 * n, 16 * n))]

    stream = torch.cuda.Stream()                         # a fresh stream, a single linear branch
    with torch.cuda.stream(stream):
        frame(stream.cuda_stream)                        # the first pass, uncaptured
    first = down()
    want = wd.spec(form, sds.world_seed(sc, rays), wd.n, rays, False)
    res = np.frombuffer(first[0], np.uint32).reshape(-1, 4)
    spec_res = np.frombuffer(want[0], np.uint32).reshape(-1, 4)
    real = np.frombuffer(first[1], np.int32) != wd.n     # (a world hit's w2, w3 are ntr_trace_bvh's)
    assert first[1] == want[1] and np.array_equal(res[:, :2], spec_res[:, :2]) and np.array_equal(res[real], spec_res[real])
    want_out, want_nrm = nf.hit_attributes(np.frombuffer(first[0], nt.RESULT_DTYPE), np.frombuffer(first[1], np.int32), sc["inst_all"], blas_tris,
                                           tri, pos)
    assert first[2] == want_out.tobytes() and first[3] == np.ascontiguousarray(want_nrm).tobytes()
    world_ids = np.frombuffer(first[2], nt.RESULT_DTYPE)["id"][~real]
    assert (world_ids >= blas_tris[sc["world"], 0]).all() and (world_ids < blas_tris[sc["world"]].sum()).all() and world_ids.size > 100
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        cs = torch.cuda.current_stream().cuda_stream
        frame(cs)
        errs = []
        try:                                             # the blocking forms are refused while capturing, and launch nothing
            stats_fn(*wd.args(form, n, False, d_rays, d_res, wd.n, d_res, d_ids), stream=cs)
        except nt.NtrError as e:
            errs.append(e.code)
    assert errs == [-1]
    for _ in range(2):
        for b in (d_res, d_ids, d_out, d_nrm):
            b.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        assert down() == first
