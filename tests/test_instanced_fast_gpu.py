"""The FAST two-level trace on the device: ntr_instanced_validate equals the spec (tests/np_instanced_fast.py) on device-built pools, at
every planted threshold, across the seam between the two buffers and beyond one pass of the grid, and as a captured launch replayed
after a refit; ntr_trace_instanced_fast equals the spec AND ntr_trace_instanced_masked / _seeded on the same buffers in all four result
words and the instance id, closest hit and any hit, and its instrumented form in the eight counters and the four new ones, on the cases
of tests/instanced_fast_cases.py (64 * 3 + 17 rays: a ragged last wave) -- whose FAST share tests/test_instanced_fast_cpu.py pins from
the spec alone; refit, top-level refit, validate and trace replay as one graph.  Output buffers are prefilled with 0xAB and nothing
beyond the extents may be written; the status word stays clear."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_fast_cases as fc
import instanced_scenes as isc
import np_bvh_refit as rf
import np_instanced as ni
import np_instanced_fast as nfa
from gpu_util import up
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED
from test_instanced_fast_cpu import THRESHOLDS, _plain_node, _planted
from test_instanced_gpu import _filled
from test_refit_batch_gpu import _Pool

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
    nt.instanced_validate(d_tlas.data_ptr() if d_tlas is not None else 0, tlas_bytes, d_pool.data_ptr(), pool_bytes, d_flags.data_ptr(), stream)
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
def test_validate_equals_the_spec_on_device_built_pools_and_trees(names, n):
    key = tuple(names)
    if key not in _cache:
        _cache[key] = _Pool(ploc=[isc.blas(name)[:2] for name in names])
    pool = _cache[key]
    rng = np.random.default_rng(n)
    inst = ni.instances(isc.seeded_transforms(n, 40 + n, spread=20.0), rng.integers(0, len(names), n))
    d_inst = up(inst)
    caps = nt.tlas_capacity(n)
    d_tlas, d_rec = _filled(caps[0] + 64), _filled(caps[1] + 64)
    res = nt.tlas_build(n, d_inst.data_ptr(), [e[0] for e in pool.entries], pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), caps[0],
                        d_rec.data_ptr(), caps[1])
    assert (res.nodesBytes == 0) == (n == 1)
    # the pool's extent and, a second time, its 0xAB slack with it: every slot counts
    for pool_bytes in (pool.caps[0], pool.caps[0] + 256):
        got = _validate(d_tlas, res.nodesBytes, pool.bufs[0], pool_bytes)
        want = nfa.validate(d_tlas.cpu().numpy()[:res.nodesBytes], pool.host[0][:pool_bytes])
        assert got == want, (names, n, got, want)
        assert got == (0, (FINITE | FASTDIV | ORDERED) if "one" in names else 0)
    # d_tlasNodes == NULL withholds nothing for the top level
    assert _validate(None, 0, pool.bufs[0], pool.caps[0]) == want


def test_validate_at_every_planted_threshold_in_either_buffer():
    plain = up(np.stack([_plain_node()] * 2))
    assert _validate(plain, 128, plain, 128) == (0, 0)
    for lo, hi, bits in THRESHOLDS:
        for pair in (0, 5):
            planted = _planted(pair, lo, hi)
            assert nfa.withheld(planted) == bits
            d = up(planted)
            assert _validate(d, planted.nbytes, plain, 128) == (bits, 0), (lo, hi, pair)
            assert _validate(plain, 128, d, planted.nbytes) == (0, bits), (lo, hi, pair)
    # the child words are not tested; a slack slot of 0xAB bytes and a zeroed one withhold nothing
    n = np.stack([_plain_node()] * 4)
    n[:, 12:] = 0x7FC00000
    n[2] = 0xABABABAB
    n[3] = 0
    assert nfa.withheld(n) == 0 and _validate(plain, 128, up(n), n.nbytes) == (0, 0)


def test_validate_across_the_seam_and_beyond_one_pass_of_the_grid():
    """A top level of 5 nodes puts the seam inside a wave (20 float4 of 64 lanes); 2048 workgroups of 256 cover 131 072 nodes in one
    pass, so node 140 000 is reached by the stride.  One planted float at a time: the last node and the first of either buffer."""
    big = np.stack([_plain_node()] * 140001)
    small = np.stack([_plain_node()] * 5)
    d_big, d_small = up(big), up(small)
    assert _validate(d_small, small.nbytes, d_big, big.nbytes) == (0, 0)
    for buf, d_buf, slot in ((big, d_big, 140000), (big, d_big, 0), (small, d_small, 4), (small, d_small, 0)):
        for word, value, bits in ((11, 2.0 ** 55, FASTDIV), (0, -fc.below(2.0 ** -93), NOTINY)):
            keep = buf[slot].copy()
            buf[slot, :12].view(F)[word] = F(value)
            d_buf[64 * slot:64 * slot + 64] = up(buf[slot])
            want = nfa.validate(small, big)
            assert want == ((bits, 0) if buf is small else (0, bits))
            assert _validate(d_small, small.nbytes, d_big, big.nbytes) == want, (slot, word)
            buf[slot] = keep
            d_buf[64 * slot:64 * slot + 64] = up(keep)
    assert _validate(d_small, small.nbytes, d_big, big.nbytes) == (0, 0)


def test_a_captured_validate_replayed_after_a_refit_that_moves_a_vertex_across_2_to_the_55():
    pool = _Pool(ploc=[isc.blas(name)[:2] for name in ("soup64", "soup1000")])
    d_flags = _flags_buffer()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        nt.instanced_validate(0, 0, pool.bufs[0].data_ptr(), pool.caps[0], d_flags.data_ptr(), s.cuda_stream)
    assert _read(d_flags) == (0, 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nt.instanced_validate(0, 0, pool.bufs[0].data_ptr(), pool.caps[0], d_flags.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for x, bits in ((2.0 ** 55, FASTDIV), (fc.below(2.0 ** 55), 0), (-2.0 ** 100, FASTDIV | FINITE), (1.0, 0)):
        p = pool.pos.copy()
        p[pool.tri[5, 1], 0] = F(x)
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, up(p), None))
        d_flags.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        got = _read(d_flags)
        assert got == (0, nfa.withheld(pool.download()[0][:pool.caps[0]])) and got == (0, bits), (x, got)


# ---- the trace ----------------------------------------------------------------------------------------------------------------------------
class _Dev:
    """A case of instanced_fast_cases on the device: the spec's own top-level tree uploaded beside the pool, and the flags validated there."""

    def __init__(self, c):
        self.c = c
        pool, (tl, self.root_link, rec) = c["pool"], c["tlas"]
        self.d_nodes, self.d_woop, self.d_idx = up(pool["nodes"]), up(pool["woop"]), up(pool["tri_index"])
        self.tlas_bytes = tl.nbytes
        self.d_tlas = up(tl) if tl.nbytes else _filled(64)
        self.d_rec = up(rec)
        self.n = rec.shape[0]
        self.d_flags = _flags_buffer()
        self.flags = _validate(self.d_tlas, self.tlas_bytes, self.d_nodes, pool["nodes"].size, self.d_flags)
        assert self.flags == nfa.validate(tl, pool["nodes"])
        self.d_M = up(c["inst_masks"]) if "inst_masks" in c else None
        self.d_m = up(c["ray_masks"]) if "ray_masks" in c else None

    def tail(self):
        p = self.c["pool"]
        return (self.d_tlas.data_ptr(), self.tlas_bytes, self.root_link, self.d_rec.data_ptr(), self.n, self.d_nodes.data_ptr(), p["nodes"].size,
                self.d_woop.data_ptr(), p["woop"].size, self.d_idx.data_ptr())

    def vis(self):
        if self.d_M is None and self.d_m is None:
            return None
        return nt.InstanceVisibility(self.d_M.data_ptr() if self.d_M is not None else 0, self.d_m.data_ptr() if self.d_m is not None else 0)

    def launch(self, how, rays, any_hit, seed=None, d_flags=None):
        """how: fast, fast_stats, plain (ntr_trace_instanced_masked / _seeded), plain_stats.
        -> (records as bytes, instance ids as bytes, counters dict or None, fast counters dict or None)"""
        n = rays.shape[0]
        d_rays = up(rays) if n else _filled(32)
        d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
        d_seed = up(seed) if seed is not None else None
        head = (n, any_hit, d_rays.data_ptr())
        out = (d_res.data_ptr(), d_ids.data_ptr())
        flags = (self.d_flags if d_flags is None else d_flags).data_ptr()
        sd = dict(d_seed_results=d_seed.data_ptr(), seed_instance=self.c.get("seed_instance", -1)) if seed is not None else {}
        st = fs = None
        if how == "fast":
            nt.trace_instanced_fast(*head, *out, *self.tail(), flags, vis=self.vis(), **sd)
        elif how == "fast_stats":
            st, fs = nt.trace_instanced_fast_stats(*head, *out, *self.tail(), flags, vis=self.vis(), **sd)
        elif seed is None:
            fn = nt.trace_instanced_masked if how == "plain" else nt.trace_instanced_stats
            st = fn(*head, *out, *self.tail(), vis=self.vis())
        else:
            fn = nt.trace_instanced_seeded if how == "plain" else nt.trace_instanced_seeded_stats
            st = fn(*head, d_seed.data_ptr(), sd["seed_instance"], *out, *self.tail(), vis=self.vis())
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        if seed is not None:
            assert d_seed.cpu().numpy().tobytes() == np.ascontiguousarray(seed).tobytes(), "the seed buffer was written"
        return (res[:16 * n].tobytes(), ids[:4 * n].tobytes(), st.as_dict() if how.endswith("stats") else None, fs.as_dict() if fs is not None else None)


def _dev(name):
    if name not in _cache:
        _cache[name] = _Dev(fc.case(name))
    return _cache[name]


def _spec(c, flags, rays, any_hit, seed):
    tl = c["tlas"]
    out = nfa.trace(flags, tl[0], tl[1], tl[2], c["pool"], rays, any_hit, c.get("inst_masks"), c.get("ray_masks"), seed=seed,
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
    """Both hit modes: the fast launch and its instrumented form against the spec and against the masked / seeded entry points."""
    c = d.c
    for any_hit in (False, True):
        seed = c["seed"](any_hit) if "seed" in c else None
        want = _spec(c, d.flags if flags is None else flags, rays, any_hit, seed)
        label = "%s anyHit=%d" % (what, any_hit)
        got = d.launch("fast", rays, any_hit, seed, d_flags)
        _assert_same(got, want, label + " against the spec")
        plain = d.launch("plain", rays, any_hit, seed)
        _assert_same(got, plain, label + " against the masked / seeded entry point")
        st = d.launch("fast_stats", rays, any_hit, seed, d_flags)
        _assert_same(st, want, label + ", instrumented")
        print(label, st[2], st[3])
        assert st[2] == want[2], (label, st[2], want[2])
        assert st[3] == want[3], (label, st[3], want[3])
        assert st[2] == d.launch("plain_stats", rays, any_hit, seed)[2], label


@pytest.mark.parametrize("name", fc.NAMES)
def test_fast_trace_equals_the_spec_and_the_masked_or_seeded_entry_point(name):
    d = _dev(name)
    _assert_case(d, d.c["rays"], name)


def test_zero_rays_and_one_ray():
    d = _dev("all_nice")
    rays = d.c["rays"]
    for any_hit in (False, True):
        for how in ("fast", "fast_stats"):
            got = d.launch(how, rays[:0], any_hit)
            assert got[0] == b"" and got[1] == b""
            assert how == "fast" or (not any(got[2].values()) and not any(got[3].values()))
    _assert_case(d, rays[100:101], "one ray")
    _assert_case(d, rays[:65], "65 rays")


def test_wrongly_withheld_flags_only_cost_speed():
    """FASTDIV withheld on both levels, on one level, and NOTINY withheld, over buffers that would grant them: the same records, and the
    counters the spec gives for those words."""
    d = _dev("object_origin_zero")
    assert d.flags == (0, 0)
    for flags in ((FASTDIV, FASTDIV), (FASTDIV, 0), (0, FASTDIV), (NOTINY, NOTINY), (ALL4, ALL4)):
        d_flags = up(np.array([flags[0], flags[1], 0, 0], np.uint32))
        _assert_case(d, d.c["rays"], "flags %r" % (flags,), flags=flags, d_flags=d_flags)
    want = _spec(d.c, (FASTDIV, FASTDIV), d.c["rays"], False, None)
    assert want[3]["fastWaveSteps"] == 0 and want[3]["niceStarts"] == 0 and want[3]["niceEntries"] == 0 < want[3]["waveSteps"]


# ---- one graph ----------------------------------------------------------------------------------------------------------------------------
def test_refit_tlas_refit_validate_and_fast_trace_replay_as_one_graph():
    sc = isc.scene("three")
    pool = _Pool(ploc=[isc.blas(name)[:2] for name in sc["names"]])
    rays = fc.nice_rays()
    n = rays.shape[0]
    inst = ni.instances(sc["transforms"], sc["blas"])
    ni_ = inst.shape[0]
    d_inst, d_rays = up(inst), up(rays)
    caps = nt.tlas_capacity(ni_)
    d_tlas, d_rec = _filled(caps[0] + 64), _filled(caps[1] + 64)
    ranges = [e[0] for e in pool.entries]
    res = nt.tlas_build(ni_, d_inst.data_ptr(), ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(), caps[1])
    d_flags = _flags_buffer()
    d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
    d_pos = up(pool.pos)
    tail = (d_tlas.data_ptr(), res.nodesBytes, res.rootLink, d_rec.data_ptr(), ni_, pool.bufs[0].data_ptr(), pool.caps[0], pool.bufs[1].data_ptr(),
            pool.caps[1], pool.bufs[2].data_ptr())
    far = pool.pos.copy()
    far[pool.tri[pool.entries[1][1] + 3, 0], 1] = F(2.0 ** 56)          # a vertex of the second BLAS beyond 2^55: the pool loses FASTDIV
    uploads = [rf.moved(pool.pos, 0.02), far, rf.moved(pool.pos, 0.3)]

    def frame(cs):
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None), stream=cs, blocking=False)
        nt.tlas_refit(ni_, d_inst.data_ptr(), ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), res.nodesBytes, res.rootLink,
                      d_rec.data_ptr(), caps[1], stream=cs, blocking=False)
        nt.instanced_validate(d_tlas.data_ptr(), res.nodesBytes, pool.bufs[0].data_ptr(), pool.caps[0], d_flags.data_ptr(), cs)
        nt.trace_instanced_fast(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), *tail, d_flags.data_ptr(), stream=cs, timed=False)

    def down():
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        r, i = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (r[16 * n:] == 0xAB).all() and (i[4 * n:] == 0xAB).all()
        return r[:16 * n].tobytes(), i[:4 * n].tobytes(), _read(d_flags), d_tlas.cpu().numpy().tobytes(), pool.download()[0].tobytes()

    def prepare(p):
        d_pos.copy_(up(p))
        pool.reset()
        for b in (d_res, d_ids, d_flags):
            b.fill_(0xAB)
        torch.cuda.synchronize()

    s = torch.cuda.Stream()
    first = []
    for p in uploads:                                    # the uncaptured sequence, per upload
        prepare(p)
        with torch.cuda.stream(s):
            frame(s.cuda_stream)
        first.append(down())
        # ... whose records are the masked entry point's on the same buffers
        d_res2, d_ids2 = _filled(16 * n + 64), _filled(4 * n + 64)
        nt.trace_instanced_masked(n, False, d_rays.data_ptr(), d_res2.data_ptr(), d_ids2.data_ptr(), *tail)
        torch.cuda.synchronize()
        assert first[-1][0] == d_res2.cpu().numpy()[:16 * n].tobytes() and first[-1][1] == d_ids2.cpu().numpy()[:4 * n].tobytes()
    assert [f[2] for f in first] == [(0, 0), (FASTDIV, FASTDIV), (0, 0)]
    assert (np.frombuffer(first[0][1], np.int32) >= 0).sum() > 20
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        frame(cs)
        errs = []
        for fn in (lambda: nt.trace_instanced_fast_stats(n, False, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), *tail, d_flags.data_ptr(),
                                                         stream=cs),
                   lambda: nt.instanced_flags_read(d_flags.data_ptr(), cs)):
            try:                                         # the blocking forms are refused while capturing, and launch nothing
                fn()
            except nt.NtrError as e:
                errs.append(e.code)
    assert errs == [-1, -1]
    for which in (1, 2, 0):
        prepare(uploads[which])
        g.replay()
        assert down() == first[which], which
