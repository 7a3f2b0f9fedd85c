"""ntr_bvh_reorder on the device: the three output buffers equal the numpy spec (tests/np_bvh_reorder.py) byte for byte for trees of
every builder, and nothing beyond the output's extents is written (the buffers are filled with 0xAB to capacity); the known answer;
the reordered tree is the same tree (trace records, visit counters, SAH cost, flags, leaf depths, refit); a reordered device SAH
tree meets the host SAH tree; two calls give the same bytes; the scratch is reported and released; the errors that need a device."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import kat_bvh_reorder as kat
import np_bvh_reorder as ro
import sah_sweep_scenes as ss
import test_bvh_refit_gpu as tr
import test_sah_device_gpu as sd
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
_cache = {}


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Tree:
    """A Compact tree on the device with its byte extents."""

    def __init__(self, nodes, woop, idx):
        self.h = (_u8(nodes).copy(), _u8(woop).copy(), _u8(idx).copy())
        self.d = tuple(up(a) for a in self.h)
        self.nb, self.wb, self.ib = (a.nbytes for a in self.h)

    def ptrs(self):
        return self.d[0].data_ptr(), self.nb, self.d[1].data_ptr(), self.wb, self.d[2].data_ptr(), self.ib


class _Out:
    """reorder(tree) into buffers of the given capacities (default: the input's extents), filled with 0xAB to capacity."""

    def __init__(self, t, caps=None, check=True):
        self.caps = caps or (t.nb, t.wb, t.ib)
        self.d = tuple(torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in self.caps)
        self.res = nt.BvhReorderResult()
        self.code = 0
        try:
            nt.bvh_reorder(*t.ptrs(), self.d[0].data_ptr(), self.caps[0], self.d[1].data_ptr(), self.caps[1], self.d[2].data_ptr(),
                           self.caps[2], result=self.res)
        except nt.NtrError as e:
            if check:
                raise
            self.code, self.message = e.code, str(e)
        torch.cuda.synchronize()
        r = self.res
        self.nb, self.wb, self.ib = r.nodesBytes, r.triWoopBytes, r.triIndexBytes
        self.raw = tuple(x.cpu().numpy() for x in self.d)

    def ptrs(self):
        return self.d[0].data_ptr(), self.nb, self.d[1].data_ptr(), self.wb, self.d[2].data_ptr(), self.ib

    def untouched(self):
        return all((x == 0xAB).all() for x in self.raw)

    def buffers(self):
        """The output inside its extents; asserts that everything beyond them is untouched."""
        ext = (self.nb, self.wb, self.ib)
        for x, e in zip(self.raw, ext):
            assert 0 <= e <= x.size and (x[e:] == 0xAB).all(), "bytes beyond the output's extents were written"
        return tuple(x[:e] for x, e in zip(self.raw, ext))


def _assert_equals_spec(out, spec, what=""):
    n, w, i = out.buffers()
    assert n.tobytes() == spec["nodes"].tobytes(), ("nodes differ", what)
    assert w.tobytes() == spec["woop"].tobytes(), ("triWoop differs", what)
    assert i.tobytes() == spec["tri_index"].tobytes(), ("triIndex differs", what)
    r = out.res
    got = dict(numNodes=r.numNodes, numLeaves=r.numLeaves, numRows=r.numRows, numDroppedSlots=r.numDroppedSlots)
    assert got == spec["stats"], (got, spec["stats"], what)
    assert r.seconds > 0


def _check(nodes, woop, idx, what=""):
    t = _Tree(nodes, woop, idx)
    out = _Out(t)
    _assert_equals_spec(out, ro.reorder(*t.h), what)
    return t, out


def _soup(n, seed=5):
    return scenes.random_soup(n, seed=seed, walls=False)[:2]


def _soup20000():
    if "soup20000" not in _cache:
        _cache["soup20000"] = scenes.random_soup(20000, seed=77, walls=False)
    return _cache["soup20000"]


def _optimised_lbvh5000():
    """(tri, pos, tree) of the 5 000-triangle soup's LBVH after two optimiser passes."""
    if "opt5000" not in _cache:
        tri, pos = _soup(5000)
        nodes, woop, idx = tr._build("lbvh", tri, pos)
        d = tr._Dev(nodes, woop, idx, tri, pos)
        res = nt.bvh_optimize(d.ptr(d.d_nodes), d.nb, 2)
        assert res.rewritten[0] > 0
        _cache["opt5000"] = (tri, pos, (d.download()[0], woop, idx))
    return _cache["opt5000"]


# ---- the known answer ---------------------------------------------------------------------------------------------------------
def test_known_answer():
    ni, w, ti = kat.before()
    want = kat.after()
    t = _Tree(ni, w, ti)
    out = _Out(t, caps=(t.nb, 16 * 23 + 64, 4 * 23 + 16))      # the shared leaf needs three rows more than the input holds
    n, wo, io = out.buffers()
    assert np.array_equal(n.view(np.int32).reshape(-1, 16), want[0])
    assert np.array_equal(wo.view(np.uint32).reshape(-1, 4), want[1])
    assert np.array_equal(io.view(np.int32), want[2])
    r = out.res
    assert dict(numNodes=r.numNodes, numLeaves=r.numLeaves, numRows=r.numRows, numDroppedSlots=r.numDroppedSlots) == kat.STATS
    assert (r.nodesBytes, r.triWoopBytes, r.triIndexBytes) == (64 * 5, 16 * 23, 4 * 23)


# ---- device == spec, byte for byte, for every tree source ------------------------------------------------------------------
@pytest.mark.parametrize("prefs", ss.LEAF_PREFS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_device_sah_trees_equal_spec(name, prefs):
    tri, pos = ss.scene(name)
    b = sd._Built(tri, pos, prefs, room=4 if name == "huge" else 1)
    _, out = _check(b.nodes, b.woop, b.idx, (name, prefs))
    print("%s %s: %d nodes, %d rows, reorder %.1f us" % (name, prefs, out.res.numNodes, out.res.numRows, out.res.seconds * 1e6))


def test_lbvh_known_answer_tree_equals_spec():
    import kat_lbvh as kl
    from test_lbvh_gpu import gpu_lbvh
    tri, pos = kl.scene()
    nodes, woop, idx = gpu_lbvh(tri, pos, kl.LEAF_SIZE, kl.EPSILON)[:3]   # a 30-level chain: the parent walk
    _check(nodes, woop, idx, "kat_lbvh")


@pytest.mark.parametrize("kind,n", [("lbvh", 1000), ("lbvh", 5000), ("hlbvh", 5000), ("binned", 5000)])
def test_device_builders_equal_spec(kind, n):
    tri, pos = _soup(n)
    nodes, woop, idx = tr._build(kind, tri, pos)               # lbvh: 1 000 the top-down fallback, 5 000 the bottom-up emit
    t, out = _check(nodes, woop, idx, (kind, n))
    assert out.res.numNodes == nodes.nbytes // 64 - out.res.numDroppedSlots
    print("%s %d: %d nodes (%d dropped), reorder %.1f us" % (kind, n, out.res.numNodes, out.res.numDroppedSlots, out.res.seconds * 1e6))


def test_optimised_lbvh_equals_spec():
    _, _, tree = _optimised_lbvh5000()
    _check(*tree, "lbvh + 2 passes")


def test_uploaded_host_tree_is_a_fixed_point():
    tri, pos, _ = _soup20000()
    h = nt.sah_build(tri, pos)
    t, out = _check(h.nodes, h.woop, h.tri_index, "host sah 20000")   # the slots span many workgroups
    for got, want in zip(out.buffers(), t.h):
        assert got.tobytes() == want.tobytes()


def test_seeded_soups_equal_spec():
    rng = np.random.default_rng(20261017)
    for i in range(50):
        n = 1 if i == 0 else int(rng.integers(1, 601))
        kind = i % 4
        if kind == 0:
            tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        elif kind == 1:   # a grid of coordinates: equal keys, equal costs, flat and degenerate triangles
            pos = rng.integers(-4, 5, (3 * n, 3)).astype(F)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        elif kind == 2:   # shared vertices, some degenerate triangles
            pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
            tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
        else:             # tiny extents and -0 / +0 coordinates
            pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)
            pos[rng.random(pos.shape) < 0.2] = F(-0.0)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        builder = ("sah", "lbvh", "hlbvh", "binned", "sah48")[(i // 4) % 5]
        if builder.startswith("sah"):
            b = sd._Built(tri, pos, (4, 8) if builder == "sah48" else (1, 1))
            tree = (b.nodes, b.woop, b.idx)
        else:
            tree = tr._build(builder, tri, pos)
        _check(*tree, (i, n, kind, builder))


# ---- the same tree --------------------------------------------------------------------------------------------------------------
def _records(ptrs, flags, d_rays, n, kernel, any_hit):
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    nt.trace_bvh(kernel, n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], bvh_flags=flags)
    torch.cuda.synchronize()
    return d_res.cpu().numpy()


def _assert_same_tree(t, out, tri, pos, cam, monkeypatch, what):
    a, b = t.ptrs(), out.ptrs()
    fa, fb = nt.bvh_validate(a[0], a[1]), nt.bvh_validate(b[0], b[1])
    assert fa == fb, (what, "validate flags")
    ca, cb = nt.bvh_sah_cost(*a[:4]), nt.bvh_sah_cost(*b[:4])
    assert F(ca.sahCost).tobytes() == F(cb.sahCost).tobytes(), (what, "SAH cost")
    assert (ca.numNodes, ca.numLeaves, ca.numTris, ca.height) == (cb.numNodes, cb.numLeaves, cb.numTris, cb.height)
    n_tris = tri.shape[0]
    da, db = (torch.full((n_tris,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2))
    la = nt.bvh_leaf_depths(a[0], a[1], a[2], a[3], a[4], n_tris, da.data_ptr())
    lb = nt.bvh_leaf_depths(b[0], b[1], b[2], b[3], b[4], n_tris, db.data_ptr())
    torch.cuda.synchronize()
    assert la == lb and torch.equal(da, db), (what, "leaf depths")
    prim = scenes.primary_rays(cam, 128, 128)[0]               # 16 384 rays
    rnd = scenes.random_rays(16384, 5, extent=float(np.abs(pos).max()))
    monkeypatch.setenv("NTR_TRACE_ROUTE", "0")
    nt.set_tunables()
    try:
        for rays, any_hit in ((prim, False), (rnd, True), (rnd, False)):
            d_rays = up(rays)
            n = rays.shape[0]
            for kernel in nt.KERNELS:
                ra, rb = _records(a, fa, d_rays, n, kernel, any_hit), _records(b, fb, d_rays, n, kernel, any_hit)
                assert ra.tobytes() == rb.tobytes(), (what, kernel, any_hit, "records")   # all four words of every record
            sa = nt.trace_bvh_stats("fermi_speculative_while_while", n, any_hit, d_rays.data_ptr(),
                                    torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0").data_ptr(), *a[:5])
            sb = nt.trace_bvh_stats("fermi_speculative_while_while", n, any_hit, d_rays.data_ptr(),
                                    torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0").data_ptr(), *b[:5])
            assert sa.as_dict() == sb.as_dict() and sa.numInnerVisits > 0, (what, any_hit, "visit counters")
    finally:
        monkeypatch.delenv("NTR_TRACE_ROUTE", raising=False)
        nt.set_tunables()
    assert nt.trace_status() == 0
    # the refit works on the output: unmoved vertices and epsilon 0 keep the links
    before = out.buffers()[0].view(np.int32).reshape(-1, 16)[:, 12:].copy()
    d_tri, d_pos = up(np.ascontiguousarray(tri, np.int32)), up(np.ascontiguousarray(pos, F))
    res = nt.bvh_refit(b[0], b[1], b[2], b[3], b[4], b[5], n_tris, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), 0.0)
    torch.cuda.synchronize()
    assert res.numNodes == out.res.numNodes and res.numLeaves == out.res.numLeaves and res.numRows == out.res.numRows
    after = out.d[0].cpu().numpy()[:out.nb].view(np.int32).reshape(-1, 16)[:, 12:]
    assert np.array_equal(before, after), (what, "links after the refit")


def test_reordered_device_sah_tree_is_the_same_tree(monkeypatch):
    tri, pos, cam = _soup20000()
    b = sd._Built(tri, pos)
    t = _Tree(b.nodes, b.woop, b.idx)
    out = _Out(t)
    assert out.buffers()[0].tobytes() != t.h[0].tobytes()      # level order is not the host's order
    _assert_same_tree(t, out, tri, pos, cam, monkeypatch, "device sah 20000")


def test_reordered_optimised_lbvh_is_the_same_tree(monkeypatch):
    tri, pos, tree = _optimised_lbvh5000()
    cam = scenes.random_soup(5000, seed=5, walls=False)[2]
    t = _Tree(*tree)
    _assert_same_tree(t, _Out(t), tri, pos, cam, monkeypatch, "lbvh 5000 + 2 passes")


# ---- device SAH meets host SAH ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup1000", "soup20000", "grid"])
def test_reordered_device_sah_tree_meets_the_host_tree(name):
    tri, pos = _soup20000()[:2] if name == "soup20000" else ss.scene(name)
    b = sd._Built(tri, pos)
    out = _Out(_Tree(b.nodes, b.woop, b.idx))
    h = nt.sah_build(tri, pos)
    n, w, i = out.buffers()
    assert (n.nbytes, w.nbytes, i.nbytes) == (h.nodes.nbytes, h.woop.nbytes, h.tri_index.nbytes)
    gn, hn = n.view(np.int32).reshape(-1, 16), h.nodes.view(np.int32).reshape(-1, 16)
    assert np.array_equal(gn[:, 12:], hn[:, 12:]), "links, word 14 or word 15 differ"
    assert np.array_equal(gn[:, :12].view(F), hn[:, :12].view(F)), "box values differ"   # -0 == +0
    assert np.array_equal(i.view(np.int32), h.tri_index)


# ---- determinism, counts, scratch ----------------------------------------------------------------------------------------------
def test_determinism_counts_and_scratch():
    nt.lbvh_release_workspace()
    assert nt.bvh_reorder_scratch_bytes() == 0
    tri, pos = _soup(5000)
    nodes, woop, idx = tr._build("lbvh", tri, pos)
    t = _Tree(nodes, woop, idx)
    a, b = _Out(t), _Out(t)
    for x, y in zip(a.raw, b.raw):
        assert x.tobytes() == y.tobytes()
    _assert_equals_spec(a, ro.reorder(*t.h))                   # result's counts equal the spec's
    held = nt.bvh_reorder_scratch_bytes()
    assert held >= 52 * (t.nb // 64)
    nt.lbvh_release_workspace()
    assert nt.bvh_reorder_scratch_bytes() == 0


# ---- errors that need a device -----------------------------------------------------------------------------------------------------
def test_short_capacities_overflow_and_leave_the_outputs_untouched():
    tri, pos = ss.scene("soup1000")
    b = sd._Built(tri, pos)
    t = _Tree(b.nodes, b.woop, b.idx)
    for caps in ((t.nb - 64, t.wb, t.ib), (t.nb - 1, t.wb, t.ib), (t.nb, t.wb - 16, t.ib), (t.nb, t.wb, t.ib - 4), (t.nb, t.wb, t.ib - 1)):
        out = _Out(t, caps, check=False)
        assert out.code == -6 and out.untouched(), (caps, out.code)
        assert out.res.numNodes == t.nb // 64 and out.res.numRows == t.wb // 16   # the counts still tell what is needed
    ni, w, ti = kat.before()                                   # the shared leaf: the input's row extent is three rows short
    out = _Out(_Tree(ni, w, ti), check=False)
    assert out.code == -6 and out.untouched() and out.res.numRows == 23


def test_malformed_trees_are_reported_and_the_output_equals_spec():
    ni, w, ti = kat.before()
    caps = (ni.nbytes, 16 * 40, 4 * 40)
    bad = ni.copy()
    bad[6, 12] = 64 * kat.NUM_SLOTS                            # LINK_BAD: one slot past the end
    t = _Tree(bad, w, ti)
    out = _Out(t, caps, check=False)
    spec = ro.reorder(*t.h)
    assert out.code == -4 and "link" in out.message and spec["bad_links"] == 1
    _assert_equals_spec(out, spec, "LINK_BAD")
    w2 = w.copy()
    w2[19, 0] = 1
    noterm = ni.copy()
    noterm[5, 12] = ~16                                        # rows 16, 19, then past the end: no terminator
    t = _Tree(noterm, w2, ti)
    out = _Out(t, caps, check=False)
    spec = ro.reorder(*t.h)
    assert out.code == -4 and "terminator" in out.message and spec["bad_leaves"] == 1
    _assert_equals_spec(out, spec, "no terminator")


@pytest.mark.timeout(30)
def test_a_cycle_among_unreached_slots_returns():
    ni, w, ti = kat.before()
    cyc = ni.copy()
    cyc[1] = ni[3]
    cyc[4] = ni[3]
    cyc[1, 12], cyc[4, 12] = 64 * 4, 64 * 1                    # slots 1 and 4 name each other; no reached slot names either
    t = _Tree(cyc, w, ti)
    out = _Out(t, (t.nb, 16 * 23, 4 * 23))
    want = kat.after()
    n, wo, io = out.buffers()
    assert np.array_equal(n.view(np.int32).reshape(-1, 16), want[0]) and np.array_equal(wo.view(np.uint32).reshape(-1, 4), want[1])
    _assert_equals_spec(out, ro.reorder(*t.h), "cycle among unreached slots")
    # a cycle among reached slots is no tree: reported, nothing written
    cyc = ni.copy()
    cyc[6, 12] = 64 * 2
    out = _Out(_Tree(cyc, w, ti), (t.nb, 16 * 40, 4 * 40), check=False)
    assert out.code == -4 and out.untouched()


def test_a_capturing_stream_is_refused():
    ni, w, ti = kat.before()
    t = _Tree(ni, w, ti)
    outs = [torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in (t.nb, 16 * 23, 4 * 23)]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        outs[0].fill_(0xAB)   # so that the graph is not empty
        try:
            nt.bvh_reorder(*t.ptrs(), outs[0].data_ptr(), t.nb, outs[1].data_ptr(), 16 * 23, outs[2].data_ptr(), 4 * 23, stream=cs)
        except nt.NtrError as e:
            errs.append(e.code)
    assert errs == [-1]
