"""The FAST wide two-level trace on the device: ntr_instanced_wide_validate equals the spec (tests/np_instanced_wide_fast.py) on
device-widened pools and top-level trees, at every planted threshold in rows 0..2 and in rows 4..6, across the seam between the two
buffers and beyond one pass of the grid; ntr_trace_instanced_wide_fast equals the spec AND ntr_trace_instanced_wide with `vis` /
ntr_trace_instanced_wide_seeded on the same buffers in all four result words and the instance id, closest hit and any hit, and its
instrumented form in the seven counters and the four new ones, on the cases of tests/instanced_wide_fast_cases.py (64 * 3 + 17 rays: a
ragged last wave) -- whose FAST share tests/test_instanced_wide_fast_cpu.py pins from the spec alone; the all-wide frame (wide pool
refit with rows, wide top-level refit, wide validate, wide fast trace) replays as one graph after vertex uploads.  Output buffers are
prefilled with 0xAB and nothing beyond the extents may be written; the status word stays clear."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_fast_cases as fc
import instanced_scenes as isc
import instanced_wide_fast_cases as wc
import np_bvh_refit as rf
import np_instanced as ni
import np_instanced_wide_fast as nwf
from gpu_util import up
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED
from test_instanced_fast_cpu import THRESHOLDS
from test_instanced_gpu import _filled
from test_instanced_wide_fast_cpu import _plain_wide, _planted
from test_refit_batch_gpu import _Pool
from test_wide_refit_gpu import _WidePool, _WideTlas

pytestmark = pytest.mark.gpu

F = np.float32
ALL4 = FINITE | FASTDIV | NOTINY | ORDERED
_cache = {}


def _flags_buffer():
    return torch.full((16 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")


def _validate(d_tlas, tlas_bytes, d_pool, pool_bytes, d_flags=None, stream=0):
    """-> the withheld pair as the device wrote it; words 2 and 3 are zero, nothing behind them is written, and
    ntr_instanced_flags_read returns the complements."""
    d_flags = _flags_buffer() if d_flags is None else d_flags
    nt.instanced_wide_validate(d_tlas.data_ptr() if d_tlas is not None else 0, tlas_bytes, d_pool.data_ptr(), pool_bytes, d_flags.data_ptr(),
                               stream)
    return _read(d_flags)


def _read(d_flags):
    torch.cuda.synchronize()
    raw = d_flags.cpu().numpy()
    w = raw[:16].view(np.uint32)
    assert w[2] == 0 and w[3] == 0 and (raw[16:] == 0xAB).all()
    assert nt.instanced_flags_read(d_flags.data_ptr()) == (ALL4 & ~int(w[0]), ALL4 & ~int(w[1]))
    return int(w[0]), int(w[1])


# ---- validate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [["soup64"], ["soup64", "soup1000", "nested90"], ["soup64", "one"], ["one", "soup1000", "nested90", "one"]])
@pytest.mark.parametrize("n", [1, 2, 64])
def test_wide_validate_equals_the_spec_on_device_widened_pools_and_trees(names, n):
    key = tuple(names)
    if key not in _cache:
        pool = _Pool(ploc=[isc.blas(name)[:2] for name in names])
        ranges = [e[0] for e in pool.entries]
        cap = nt.pool_widen_capacity(ranges)
        d_wide = _filled(cap + 64)
        wide_ranges, res = nt.pool_widen_batch(ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_wide.data_ptr(), cap)
        torch.cuda.synchronize()
        _cache[key] = (pool, ranges, wide_ranges, d_wide, int(res.nodesBytes))
    pool, ranges, wide_ranges, d_wide, wide_bytes = _cache[key]
    rng = np.random.default_rng(n)
    inst = ni.instances(isc.seeded_transforms(n, 40 + n, spread=20.0), rng.integers(0, len(names), n))
    d_inst = up(inst)
    caps = nt.tlas_capacity(n)
    d_tlas, d_rec = _filled(caps[0] + 64), _filled(caps[1] + 64)
    t = nt.tlas_build(n, d_inst.data_ptr(), ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(), caps[1])
    cap = max(nt.bvh_widen_capacity(t.nodesBytes), 128) if n > 1 else 128
    d_wt, d_wrec = _filled(cap + 64), _filled(64 * n + 64)
    w = nt.tlas_widen(n, d_inst.data_ptr(), d_tlas.data_ptr(), t.nodesBytes, t.rootLink, ranges, wide_ranges, d_wt.data_ptr(), cap,
                      d_wrec.data_ptr(), 64 * n)
    torch.cuda.synchronize()
    assert (w.nodesBytes == 0) == (n == 1)
    got = _validate(d_wt, w.nodesBytes, d_wide, wide_bytes)
    want = nwf.validate(d_wt.cpu().numpy()[:w.nodesBytes], d_wide.cpu().numpy()[:wide_bytes])
    assert got == want, (names, n, got, want)
    assert got == (0, (FINITE | FASTDIV | ORDERED) if "one" in names else 0)
    # two slots of slack behind the last wide BLAS count, whatever they hold
    assert wide_bytes + 256 <= d_wide.numel()
    assert _validate(d_wt, w.nodesBytes, d_wide, wide_bytes + 256) == nwf.validate(d_wt.cpu().numpy()[:w.nodesBytes],
                                                                                   d_wide.cpu().numpy()[:wide_bytes + 256])
    # d_wideTlasNodes == NULL, and wideTlasNodesBytes == 0, withhold nothing for the top level
    assert _validate(None, 0, d_wide, wide_bytes) == want
    assert _validate(d_wt, 0, d_wide, wide_bytes) == want


def test_wide_validate_at_every_planted_threshold_in_either_buffer_and_either_half_of_a_slot():
    plain = up(np.stack([_plain_wide()] * 2))
    assert _validate(plain, 256, plain, 256) == (0, 0)
    for lo, hi, bits in THRESHOLDS:
        for pair in (0, 5, 6, 11):                       # rows 0 and 2, rows 4 and 6
            planted = _planted(pair, lo, hi)
            assert nwf.withheld_wide(planted) == bits
            d = up(planted)
            assert _validate(d, planted.nbytes, plain, 256) == (bits, 0), (lo, hi, pair)
            assert _validate(plain, 256, d, planted.nbytes) == (0, bits), (lo, hi, pair)
    # the links and the count words are not tested; a slack slot of 0xAB bytes and a zeroed one withhold nothing
    n = np.stack([_plain_wide()] * 4)
    n[:, 12:16] = 0xABABABAB
    n[:, 28:32] = 0xABABABAB
    n[1, 12:16] = 0x7FC00000
    n[1, 28:32] = 0x7F800000
    n[2] = 0xABABABAB
    n[3] = 0
    assert nwf.withheld_wide(n) == 0 and _validate(plain, 256, up(n), n.nbytes) == (0, 0)


def test_wide_validate_across_the_seam_and_beyond_one_pass_of_the_grid():
    """A top level of ONE wide node puts the seam inside a wave (8 float4 of 64 lanes); 2048 workgroups of 256 cover 65 536 wide nodes in
    one pass, so node 70 000 is reached by the stride.  One planted float at a time: the last node and the first of the pool, and the
    top level's only node, in rows 0..2 and in rows 4..6."""
    big = np.stack([_plain_wide()] * 70001)
    small = np.stack([_plain_wide()] * 1)
    d_big, d_small = up(big), up(small)
    assert _validate(d_small, small.nbytes, d_big, big.nbytes) == (0, 0)
    for buf, d_buf, slot in ((big, d_big, 70000), (big, d_big, 0), (small, d_small, 0)):
        for word, value, bits in ((11, 2.0 ** 55, FASTDIV), (0, -fc.below(2.0 ** -93), NOTINY), (27, 2.0 ** 55, FASTDIV),
                                  (16, -fc.below(2.0 ** -93), NOTINY)):
            keep = buf[slot].copy()
            buf[slot, word:word + 1].view(F)[0] = F(value)
            d_buf[128 * slot:128 * slot + 128] = up(buf[slot])
            want = nwf.validate(small, big)
            assert want == ((bits, 0) if buf is small else (0, bits))
            assert _validate(d_small, small.nbytes, d_big, big.nbytes) == want, (slot, word)
            buf[slot] = keep
            d_buf[128 * slot:128 * slot + 128] = up(keep)
    assert _validate(d_small, small.nbytes, d_big, big.nbytes) == (0, 0)


# ---- the trace ----------------------------------------------------------------------------------------------------------------------------
class _Dev:
    """A case of instanced_wide_fast_cases on the device: the spec's own wide trees uploaded beside the pool's rows, and the flags
    validated there."""

    def __init__(self, c):
        self.c = c
        pool, (tl, self.root_link, rec) = c["pool"], c["wide_tlas"]
        self.d_wide, self.d_woop, self.d_idx = up(c["wide_pool"]), up(pool["woop"]), up(pool["tri_index"])
        self.tlas_bytes = tl.nbytes
        self.d_tlas = up(tl) if tl.nbytes else _filled(128)
        self.d_rec = up(rec)
        self.n = rec.shape[0]
        self.d_flags = _flags_buffer()
        self.flags = _validate(self.d_tlas, self.tlas_bytes, self.d_wide, c["wide_pool"].size, self.d_flags)
        assert self.flags == nwf.validate(tl, c["wide_pool"])
        self.d_M = up(c["inst_masks"]) if "inst_masks" in c else None
        self.d_m = up(c["ray_masks"]) if "ray_masks" in c else None

    def tail(self):
        p = self.c["pool"]
        return (self.d_tlas.data_ptr(), self.tlas_bytes, self.root_link, self.d_rec.data_ptr(), self.n, self.d_wide.data_ptr(),
                self.c["wide_pool"].size, self.d_woop.data_ptr(), p["woop"].size, self.d_idx.data_ptr())

    def vis(self):
        return nt.InstanceVisibility(self.d_M.data_ptr() if self.d_M is not None else 0, self.d_m.data_ptr() if self.d_m is not None else 0)

    def launch(self, how, rays, any_hit, seed=None, d_flags=None, null_vis=False):
        """how: fast, fast_stats, plain (ntr_trace_instanced_wide with vis / _wide_seeded), plain_stats.
        -> (records as bytes, instance ids as bytes, counters dict or None, fast counters dict or None)"""
        n = rays.shape[0]
        d_rays = up(rays) if n else _filled(32)
        d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
        d_seed = up(seed) if seed is not None else None
        head = (n, any_hit, d_rays.data_ptr())
        out = (d_res.data_ptr(), d_ids.data_ptr())
        flags = (self.d_flags if d_flags is None else d_flags).data_ptr()
        vis = None if null_vis else self.vis()
        sd = dict(d_seed_results=d_seed.data_ptr(), seed_instance=self.c.get("seed_instance", -1)) if seed is not None else {}
        st = fs = None
        if how == "fast":
            nt.trace_instanced_wide_fast(*head, *out, *self.tail(), flags, vis=vis, **sd)
        elif how == "fast_stats":
            st, fs = nt.trace_instanced_wide_fast_stats(*head, *out, *self.tail(), flags, vis=vis, **sd)
        elif seed is None:
            fn = nt.trace_instanced_wide if how == "plain" else nt.trace_instanced_wide_stats
            st = fn(*head, *out, *self.tail(), vis=vis)
        else:
            fn = nt.trace_instanced_wide_seeded if how == "plain" else nt.trace_instanced_wide_seeded_stats
            st = fn(*head, d_seed.data_ptr(), sd["seed_instance"], *out, *self.tail(), vis=vis)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        if seed is not None:
            assert d_seed.cpu().numpy().tobytes() == np.ascontiguousarray(seed).tobytes(), "the seed buffer was written"
        return (res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st.as_dict() if how.endswith("stats") else None, fs.as_dict() if fs is not None else None)


def _dev(name):
    if name not in _cache:
        _cache[name] = _Dev(wc.case(name))
    return _cache[name]


def _spec(c, flags, rays, any_hit, seed):
    tl = c["wide_tlas"]
    out = nwf.trace(flags, tl[0], tl[1], tl[2], c["pool"], c["wide_pool"], rays, any_hit, c.get("inst_masks"), c.get("ray_masks"), seed=seed,
                    seed_instance=c.get("seed_instance", -1))
    words = np.stack([np.ascontiguousarray(x).view(np.uint32) for x in out[:4]], axis=1)
    return words.tobytes(), out[4].astype(np.int32).tobytes(), out[5], out[6]


def _assert_same(got, want, what):
    for name, g, e, dt in (("record", got[0], want[0], np.uint32), ("instance", got[1], want[1], np.int32)):
        if g != e:
            g, e = np.frombuffer(g, dt), np.frombuffer(e, dt)
            bad = np.flatnonzero(g != e)
            raise AssertionError("%s: %d %s words differ, first at word %d: %r != %r" % (what, bad.size, name, bad[0], g[bad[0]], e[bad[0]]))


def _assert_case(d, rays, what, flags=None, d_flags=None):
    """Both hit modes: the wide fast launch and its instrumented form against the spec and against the wide / wide seeded entry points."""
    c = d.c
    for any_hit in (False, True):
        seed = c["seed"](any_hit) if "seed" in c else None
        want = _spec(c, d.flags if flags is None else flags, rays, any_hit, seed)
        label = "%s anyHit=%d" % (what, any_hit)
        got = d.launch("fast", rays, any_hit, seed, d_flags)
        _assert_same(got, want, label + " against the spec")
        plain = d.launch("plain", rays, any_hit, seed)
        _assert_same(got, plain, label + " against the wide / wide seeded entry point")
        st = d.launch("fast_stats", rays, any_hit, seed, d_flags)
        _assert_same(st, want, label + ", instrumented")
        print(label, st[2], st[3])
        want_cnt = {k: v for k, v in want[2].items() if k in st[2]}
        assert st[2] == want_cnt, (label, st[2], want_cnt)
        assert st[3] == want[3], (label, st[3], want[3])
        assert st[2] == d.launch("plain_stats", rays, any_hit, seed)[2], label


@pytest.mark.parametrize("name", wc.NAMES)
def test_wide_fast_trace_equals_the_spec_and_the_wide_or_wide_seeded_entry_point(name):
    d = _dev(name)
    _assert_case(d, d.c["rays"], name)


def test_zero_rays_one_ray_65_rays_and_a_null_vis():
    d = _dev("all_nice")
    rays = d.c["rays"]
    for any_hit in (False, True):
        for how in ("fast", "fast_stats"):
            got = d.launch(how, rays[:0], any_hit)
            assert got[0] == b"" and got[1] == b""
            assert how == "fast" or (not any(got[2].values()) and not any(got[3].values()))
        assert d.launch("fast", rays, any_hit, null_vis=True)[:2] == d.launch("fast", rays, any_hit)[:2]      # vis may be NULL
    _assert_case(d, rays[100:101], "one ray")
    _assert_case(d, rays[:65], "65 rays")


def test_wrongly_withheld_flags_only_cost_speed():
    """FASTDIV withheld on both levels, on one level, NOTINY withheld, and all four bits set by hand, over buffers that would grant
    them: the same records, and the counters the spec gives for those words."""
    d = _dev("object_origin_zero")
    assert d.flags == (0, 0)
    for flags in ((FASTDIV, FASTDIV), (FASTDIV, 0), (0, FASTDIV), (NOTINY, NOTINY), (ALL4, ALL4)):
        d_flags = up(np.array([flags[0], flags[1], 0, 0], np.uint32))
        _assert_case(d, d.c["rays"], "flags %r" % (flags,), flags=flags, d_flags=d_flags)
    for any_hit in (False, True):
        want = _spec(d.c, (ALL4, ALL4), d.c["rays"], any_hit, None)
        assert want[3]["fastWaveSteps"] == 0 and want[3]["niceStarts"] == 0 and want[3]["niceEntries"] == 0 < want[3]["waveSteps"]
        got = d.launch("fast_stats", d.c["rays"], any_hit, None, up(np.array([ALL4, ALL4, 0, 0], np.uint32)))
        assert got[3]["fastWaveSteps"] == 0 and got[:2] == d.launch("plain", d.c["rays"], any_hit)[:2]


# ---- one graph ----------------------------------------------------------------------------------------------------------------------------
def test_the_all_wide_frame_replays_as_one_graph_after_vertex_uploads():
    """ntr_pool_wide_refit(rewriteRows = 1) + ntr_tlas_wide_refit + ntr_instanced_wide_validate + ntr_trace_instanced_wide_fast, captured
    once and replayed over rewritten vertices.  No binary refit runs: the binary pool's boxes stay what the build made, so only a
    validate over the wide buffers can see the vertex at 2^56."""
    sc = isc.scene("three")
    wp = _WidePool(ploc=[isc.blas(name)[:2] for name in sc["names"]])
    pool = wp.pool
    inst = ni.instances(sc["transforms"], sc["blas"])
    s = _WideTlas(wp, inst)
    rays = fc.nice_rays()
    n = rays.shape[0]
    d_rays = up(rays)
    d_flags = _flags_buffer()
    d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
    d_pos = up(pool.pos)
    sel = list(range(len(wp.entries)))
    tail = (s.d_wt.data_ptr(), s.nodes_bytes, s.root, s.d_rec.data_ptr(), s.n, wp.d_wide.data_ptr(), wp.wide_bytes, pool.bufs[1].data_ptr(),
            pool.caps[1], pool.bufs[2].data_ptr())
    far = pool.pos.copy()
    far[pool.tri[pool.entries[1][1] + 3, 0], 1] = F(2.0 ** 56)          # a vertex of the second BLAS beyond 2^55: the wide pool loses FASTDIV
    uploads = [rf.moved(pool.pos, 0.02), far, rf.moved(pool.pos, 0.3)]
    binary_nodes = pool.download()[0].tobytes()

    def frame(cs):
        wp.call(sel, d_pos, 1, stream=cs, blocking=False)
        s.refit(blocking=False, stream=cs)
        nt.instanced_wide_validate(s.d_wt.data_ptr(), s.nodes_bytes, wp.d_wide.data_ptr(), wp.wide_bytes, d_flags.data_ptr(), cs)
        nt.trace_instanced_wide_fast(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), *tail, d_flags.data_ptr(), stream=cs, timed=False)

    def down():
        """-> records, ids, flags; asserted: the flags are the spec's of the refitted wide buffers, and the records are the non-fast wide
        launch's on the same buffers."""
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        r, i = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (r[16 * n:] == 0xAB).all() and (i[4 * n:] == 0xAB).all()
        flags = _read(d_flags)
        assert flags == nwf.validate(s.download()[0], wp.download()[0][:wp.wide_bytes])
        d_res2, d_ids2 = _filled(16 * n + 64), _filled(4 * n + 64)
        nt.trace_instanced_wide(n, False, d_rays.data_ptr(), d_res2.data_ptr(), d_ids2.data_ptr(), *tail, vis=nt.InstanceVisibility(0, 0))
        torch.cuda.synchronize()
        assert r[:16 * n].tobytes() == d_res2.cpu().numpy()[:16 * n].tobytes() and i[:4 * n].tobytes() == d_ids2.cpu().numpy()[:4 * n].tobytes()
        assert pool.download()[0].tobytes() == binary_nodes, "the all-wide path wrote the binary nodes"
        return r[:16 * n].tobytes(), i[:4 * n].tobytes(), flags

    def prepare(p):
        d_pos.copy_(up(p))
        for b in (d_res, d_ids, d_flags):
            b.fill_(0xAB)
        torch.cuda.synchronize()

    st = torch.cuda.Stream()
    first = []
    for p in uploads:                                    # the uncaptured sequence, per upload
        prepare(p)
        with torch.cuda.stream(st):
            frame(st.cuda_stream)
        first.append(down())
    assert first[0][2] == (0, 0) and first[2][2] == (0, 0)
    assert first[1][2][1] & FASTDIV, "the wide pool keeps FASTDIV with a vertex at 2^56"
    assert (np.frombuffer(first[0][1], np.int32) >= 0).sum() > 20
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        cs = torch.cuda.current_stream().cuda_stream
        frame(cs)
        errs = []
        try:                                             # the blocking form is refused while capturing, and launches nothing
            nt.trace_instanced_wide_fast_stats(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), *tail, d_flags.data_ptr(), stream=cs)
        except nt.NtrError as e:
            errs.append(e.code)
    assert errs == [-1]
    for which in (1, 2, 0):
        prepare(uploads[which])
        g.replay()
        assert down() == first[which], which
    del g
