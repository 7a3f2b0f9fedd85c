"""The 4-wide BVH on the device: ntr_bvh_widen equals the numpy spec (tests/np_bvh_wide.py) byte for byte and in every result field on
trees of every origin; ntr_trace_wide equals the spec in all four result words for closest hit and any hit, with bvhFlags 0 and with the
binary tree's validated flags; the stats variant returns the same records and the spec's counters; a deep chain runs past the LDS
stack; two runs give the same bytes and the scratch pool is released; a link outside the extent is reported after the work.  Output
buffers are prefilled with 0xAB and nothing beyond the extents may be written."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import np_bvh_wide as wd
import sah_sweep_scenes as ss
import wide_trees as wt
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
_dev = {}


def _filled(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xAB, dtype=torch.uint8, device="cuda:0")


class _Tree:
    """A binary tree on the device and its wide tree, built into a 0xAB-filled buffer of the capacity plus a guard."""

    def __init__(self, nodes, woop, tri_index, check=True):
        self.nodes, self.woop, self.tri_index = nodes, woop, tri_index
        self.d_nodes, self.d_woop, self.d_idx = up(nodes), up(woop), up(tri_index)
        self.cap = nt.bvh_widen_capacity(nodes.nbytes)
        assert self.cap == 128 * (nodes.nbytes // 64)
        self.flags = nt.bvh_validate(self.d_nodes.data_ptr(), nodes.nbytes)
        self.widen(check)

    def widen(self, check=True):
        self.d_wide = _filled(self.cap + 256)
        res = nt.BvhWideResult()
        self.rc = nt.lib().ntr_bvh_widen(self.d_nodes.data_ptr(), self.nodes.nbytes, self.d_wide.data_ptr(), self.cap, C.byref(res), None)
        assert self.rc == 0 or not check, nt.lib().ntr_last_error()
        torch.cuda.synchronize()
        self.res = res
        raw = self.d_wide.cpu().numpy()
        assert 0 < res.nodesBytes <= self.cap and (raw[res.nodesBytes:] == 0xAB).all(), "bytes beyond the result's extent were written"
        self.wide = raw[:res.nodesBytes].view(np.int32).reshape(-1, 32).copy()
        return self

    def trace(self, rays, any_hit, flags=0, stats=False, timed=True):
        n = rays.shape[0]
        d_rays, d_res = up(rays), _filled(16 * n + 64)
        args = (n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.d_wide.data_ptr(), self.res.nodesBytes, self.d_woop.data_ptr(),
                self.woop.nbytes, self.d_idx.data_ptr(), flags)
        out = nt.trace_wide_stats(*args) if stats else nt.trace_wide(*args, timed=timed)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        raw = d_res.cpu().numpy()
        assert (raw[16 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        return raw[:16 * n].view(nt.RESULT_DTYPE).copy(), out


def _named(name):
    if name not in _dev:
        _dev[name] = _Tree(*wt.tree(name))
    return _dev[name]


def _assert_widen_equals_spec(t, ref, what=""):
    r = t.res
    got = dict(numNodes=r.numNodes, counts=list(r.counts), numLeafLinks=r.numLeafLinks, height=r.height, stackBound=r.stackBound)
    assert got == ref["stats"], (got, ref["stats"], what)
    assert r.nodesBytes == ref["nodes"].nbytes and r.seconds > 0
    assert t.wide.shape == ref["nodes"].shape, what
    bad = np.flatnonzero((t.wide != ref["nodes"]).any(axis=1))
    assert bad.size == 0, ("wide nodes differ", what, int(bad[0]), t.wide[bad[0]], ref["nodes"][bad[0]])


def _assert_trace_equals_spec(t, ref_nodes, rays, what=""):
    for any_hit in (False, True):
        rid, rt, ru, rv = wd.trace(ref_nodes, t.woop, t.tri_index, rays, any_hit)
        got0, _ = t.trace(rays, any_hit, 0)
        got1, _ = t.trace(rays, any_hit, t.flags)
        assert got0.tobytes() == got1.tobytes(), "%s anyHit=%d: flags 0 and flags 0x%x give different bytes" % (what, any_hit, t.flags)
        for name, g, e in (("id", got0["id"], rid), ("t", got0["t"].view(np.uint32), rt.view(np.uint32)),
                           ("u", got0["padA"].view(np.uint32), ru.view(np.uint32)), ("v", got0["padB"].view(np.uint32), rv.view(np.uint32))):
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, "%s anyHit=%d: %d %s mismatches of %d rays, first at ray %d: %r != %r" % (
                what, any_hit, bad.size, name, rays.shape[0], bad[0], g[bad[0]], e[bad[0]])
    return rid


# ---- the widening pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "soup2", "soup3", "soup4", "soup5", "soup64", "soup65", "soup1000", "cornell", "grid", "identical",
                                  "nested90", "sah8", "spread"])
def test_widen_equals_spec(name):
    t = _named(name)
    _assert_widen_equals_spec(t, wt.wide(name), name)
    r = t.res
    print("%s: %d slots -> %d wide nodes %s, height %d, stackBound %d, %.3f ms" % (name, t.nodes.shape[0], r.numNodes, list(r.counts), r.height,
                                                                                  r.stackBound, r.seconds * 1e3))


def _device_build(kind, tri, pos):
    n = tri.shape[0]
    caps = nt.lbvh_capacity(n)
    d_tri, d_pos = up(tri), up(pos)
    d_n, d_w, d_i = (torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps)
    mn, mx = pos.min(axis=0), pos.max(axis=0)
    if kind == "lbvh":
        r = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, d_n.data_ptr(), caps[0], d_w.data_ptr(), caps[1],
                          d_i.data_ptr(), caps[2])
    else:
        r = nt.ploc_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, d_n.data_ptr(), caps[0], d_w.data_ptr(), caps[1],
                          d_i.data_ptr(), caps[2])
        nt.bvh_optimize(d_n.data_ptr(), r.nodesBytes, 1)
    torch.cuda.synchronize()
    return (d_n.cpu().numpy()[:r.nodesBytes].view(np.int32).reshape(-1, 16).copy(), d_w.cpu().numpy()[:r.triWoopBytes].copy(),
            d_i.cpu().numpy()[:r.triIndexBytes].view(np.int32).copy())


def test_widen_a_device_lbvh_tree_with_leaf_size_8():
    """ntr_lbvh_build at leafSize 8 (the bottom-up emit) over a soup plus forty identical triangles.  Such a buffer may hold zero-filled
    slots no link reaches (NtrLbvhResult); how many this one holds is printed, and whatever it holds, the wide tree is the spec's: an
    unreached slot is dropped.  The tree 'spread' has such slots by construction."""
    tri, pos = scenes.random_soup(5000, seed=5005, walls=False)[:2]
    tri2, pos2 = ss.scene("identical")
    tri, pos = np.concatenate([tri, tri2 + pos.shape[0]]), np.concatenate([pos, pos2])
    nodes, woop, idx = _device_build("lbvh", tri, pos)
    t = _Tree(nodes, woop, idx)
    ref = wd.widen(nodes)
    _assert_widen_equals_spec(t, ref, "lbvh")
    zero = (nodes == 0).all(axis=1)
    print("lbvh: %d slots, %d of them zero-filled, %d wide nodes" % (nodes.shape[0], int(zero.sum()), t.res.numNodes))
    assert not zero[ref["kept"]].any()
    _assert_trace_equals_spec(t, ref["nodes"], scenes.random_rays(1000, 4), "lbvh")


def test_widen_a_device_ploc_tree_after_optimize():
    tri, pos = ss.scene("soup1000")
    nodes, woop, idx = _device_build("ploc", tri, pos)
    t = _Tree(nodes, woop, idx)
    _assert_widen_equals_spec(t, wd.widen(nodes), "ploc + optimize")


def test_widen_across_the_scan_chunk_boundary():
    """65 537 binary slots and more: the scan of the kept flags takes 257 workgroups of 256, one more than scan_block_sums covers in a
    single chunk, and the marking's levels outgrow one workgroup."""
    tri, pos = scenes.random_soup(66000, seed=66, walls=False)[:2]
    nodes, woop, idx = _device_build("ploc", tri, pos)
    assert nodes.shape[0] > 65536 + 256
    t = _Tree(nodes, woop, idx)
    _assert_widen_equals_spec(t, wd.widen(nodes), "66000")


# ---- the trace ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup1000", "sah8"])
def test_trace_equals_spec(name):
    t = _named(name)
    rays = wt.rays_for(name)
    rid = _assert_trace_equals_spec(t, wt.wide(name)["nodes"], rays, name)
    assert (rid >= 0).sum() > rays.shape[0] // 8
    if name != "cornell":
        assert t.flags & nt.BVH_FASTDIV, "the soup's flags were expected to select the FAST path"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ray_counts(n):
    _assert_trace_equals_spec(_named("soup1000"), wt.wide("soup1000")["nodes"], wt.rays_for("soup1000")[4000:4000 + n], n)


@pytest.mark.parametrize("any_hit", [False, True])
def test_stats_variant_returns_the_same_records_and_the_specs_counters(any_hit):
    t = _named("sah8")
    rays = wt.rays_for("sah8")[6000:10000]
    want = wd.trace(wt.wide("sah8")["nodes"], t.woop, t.tri_index, rays, any_hit, return_stats=True)[4]
    for flags in (0, t.flags):
        plain, _ = t.trace(rays, any_hit, flags)
        got, st = t.trace(rays, any_hit, flags, stats=True)
        assert got.tobytes() == plain.tobytes()
        assert st.as_dict() == want, (st.as_dict(), want)


def test_a_deep_chain_runs_past_the_lds_stack():
    t = _named("nested90")
    ref = wt.wide("nested90")
    assert 16 < ref["stats"]["stackBound"] <= wd.MAX_STACK and t.res.stackBound == ref["stats"]["stackBound"]
    rays = wt.deep_rays()
    rid = _assert_trace_equals_spec(t, ref["nodes"], rays, "nested90")   # (the status word is checked clear after every trace)
    assert (rid >= 0).any()
    probe = {}
    wd.trace(ref["nodes"], t.woop, t.tri_index, rays, False, probe=probe)
    assert probe["maxStack"] > 16, probe                                 # the traversal held more than the LDS entries


def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.bvh_widen_scratch_bytes() == 0
    t = _Tree(*wt.tree("soup1000"))
    held = nt.bvh_widen_scratch_bytes()
    assert held > 0
    first = t.wide.copy()
    t.widen()
    assert nt.bvh_widen_scratch_bytes() == held and t.wide.tobytes() == first.tobytes()
    rays = wt.rays_for("soup1000")[:4096]
    assert t.trace(rays, False)[0].tobytes() == t.trace(rays, False)[0].tobytes()
    nt.lbvh_release_workspace()
    assert nt.bvh_widen_scratch_bytes() == 0
    t.widen()
    assert t.wide.tobytes() == first.tobytes()
    nt.lbvh_release_workspace()


def test_asynchronous_trace_then_status():
    t = _named("soup1000")
    rays = wt.rays_for("soup1000")[:4096]
    timed, sec = t.trace(rays, False)
    got, none = t.trace(rays, False, timed=False)        # ends with ntr_trace_status: 0
    assert none is None and sec > 0 and got.tobytes() == timed.tobytes()


def test_a_link_outside_the_extent_is_reported_after_the_work():
    nodes, woop, idx = wt.tree("soup64")
    bad = nodes.copy()
    slot = int(np.flatnonzero(bad[:, 12] > 0)[-1])
    bad[slot, 12] = 64 * bad.shape[0]                     # the first slot beyond the extent
    t = _Tree(bad, woop, idx, check=False)
    assert t.rc == -4 and b"name no node slot" in nt.lib().ntr_last_error()
    with pytest.raises(wd.LayoutError) as e:
        wd.widen(bad)
    ref = e.value.result
    assert ref["bad_links"] == 1
    _assert_widen_equals_spec(t, ref, "bad link")
    _assert_trace_equals_spec(t, ref["nodes"], wt.rays_for("soup1000")[8000:9000], "bad link")


def test_argument_errors_on_the_device():
    t = _named("soup64")
    d_out = _filled(t.cap)
    good = dict(d_nodes=t.d_nodes.data_ptr(), nodes_bytes=t.nodes.nbytes, d_wide_nodes=d_out.data_ptr(), wide_capacity=t.cap)
    for change in (dict(wide_capacity=t.cap - 1), dict(nodes_bytes=t.nodes.nbytes - 32), dict(d_nodes=0), dict(d_wide_nodes=0),
                   dict(d_wide_nodes=t.d_nodes.data_ptr()), dict(d_wide_nodes=t.d_nodes.data_ptr() + 64)):
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_widen(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xAB).all()            # refused before any device work
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    res = nt.BvhWideResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d_out.fill_(0xAB)   # so that the graph is not empty
        rc = nt.lib().ntr_bvh_widen(good["d_nodes"], good["nodes_bytes"], good["d_wide_nodes"], good["wide_capacity"], C.byref(res), cs)
    assert rc == -1 and b"captured" in nt.lib().ntr_last_error() and bytes(res) == bytes(C.sizeof(res))
    r = nt.bvh_widen(**good)
    assert r.numNodes == wt.wide("soup64")["stats"]["numNodes"] and r.seconds > 0
