"""ntr_ploc_build on the device: nodes, Woop rows, triIndex, rounds, height and extents equal the numpy spec (tests/np_bvh_ploc.py)
byte for byte at every size where the kernels take another path (the tail alone, the hand-over, one and several tiles, halos across
tile edges, ties across tile edges, chains); trace records over the device tree equal oracle.trace under every kernel name; validate,
SAH cost, refit, optimise and reorder take the tree as it is; two builds give the same bytes and the scratch pool is released; every
argument check is reported."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_bvh_optimize as op
import np_bvh_ploc as pl
import np_bvh_reorder as ro
import sah_sweep_scenes as ss
from gpu_util import assert_parity, up

pytestmark = pytest.mark.gpu

F = np.float32
THREADS = 16
TAIL, TILE = nt.PLOC_TAIL, nt.PLOC_TILE
_cache = {}


class _Built:
    """A device build into buffers of lbvh_capacity(n) bytes filled with 0xAB; nothing beyond the result's extents is written."""

    def __init__(self, tri, pos, radius=8, box=None):
        tri = np.ascontiguousarray(tri, np.int32)
        pos = np.ascontiguousarray(pos, F)
        n = tri.shape[0]
        self.n, self.nv = n, pos.shape[0]
        self.box = box or pl.scene_box(pos)
        self.d_tri, self.d_pos = up(tri), up(pos)
        self.caps = nt.lbvh_capacity(n)
        self.d_nodes, self.d_woop, self.d_idx = (torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in self.caps)
        self.res = nt.ploc_build(n, self.d_tri.data_ptr(), self.nv, self.d_pos.data_ptr(), self.box[0], self.box[1], self.d_nodes.data_ptr(),
                                 self.caps[0], self.d_woop.data_ptr(), self.caps[1], self.d_idx.data_ptr(), self.caps[2], radius)
        torch.cuda.synchronize()
        r = self.res
        raw = tuple(x.cpu().numpy() for x in (self.d_nodes, self.d_woop, self.d_idx))
        for x, e in zip(raw, (r.nodesBytes, r.triWoopBytes, r.triIndexBytes)):
            assert 0 < e <= x.size and (x[e:] == 0xAB).all(), "bytes beyond the result's extents were written"
        self.nodes = raw[0][:r.nodesBytes].view(np.int32).reshape(-1, 16).copy()
        self.woop = raw[1][:r.triWoopBytes].copy()
        self.idx = raw[2][:r.triIndexBytes].view(np.int32).copy()

    def ptrs(self):
        r = self.res
        return self.d_nodes.data_ptr(), r.nodesBytes, self.d_woop.data_ptr(), r.triWoopBytes, self.d_idx.data_ptr(), r.triIndexBytes


def _woop_equal(got, exp):
    """A NaN that arithmetic produces carries the processor's sign and payload (the overflowing Woop rows of "huge", the underflowing
    ones of the long chain): such words are compared as NaN == NaN, every other word by bits."""
    got, exp = got.view(np.uint32), exp.view(np.uint32)
    return got.shape == exp.shape and bool(((got == exp) | (np.isnan(got.view(F)) & np.isnan(exp.view(F)))).all())


def _assert_equal_to_spec(b, ref, what=""):
    assert np.array_equal(b.nodes, ref["nodes"]), ("nodes differ", what, int(np.flatnonzero((b.nodes != ref["nodes"]).any(axis=1))[0]))
    assert np.array_equal(b.idx, ref["tri_index"]), ("triIndex differs", what)
    assert _woop_equal(b.woop, ref["woop"]), ("triWoop differs", what)
    r = b.res
    got = dict(numNodes=r.numNodes, numLeaves=r.numLeaves, numRounds=r.numRounds, height=r.height)
    assert got == ref["stats"], (got, ref["stats"], what)
    assert r.nodesBytes == ref["nodes"].nbytes and r.triWoopBytes == ref["woop"].nbytes and r.triIndexBytes == ref["tri_index"].nbytes
    sizes = ref["sizes"]
    tail = next((s for s in sizes if s <= TAIL), 0)
    assert r.tailClusters == tail, (r.tailClusters, tail, what)


def _check(tri, pos, radius=8, what=""):
    b = _Built(tri, pos, radius)
    _assert_equal_to_spec(b, pl.build(tri, pos, b.box[0], b.box[1], radius), (what, radius))
    return b


def _soup(n, seed):
    return scenes.random_soup(n, seed=seed, walls=False)[:2]


def _soup20000():
    """(tri, pos, cam, device build, spec) of random_soup(20000, 5), built once."""
    if "soup20000" not in _cache:
        tri, pos, cam = scenes.random_soup(20000, seed=5)
        b = _Built(tri, pos)
        _cache["soup20000"] = (tri, pos, cam, b, pl.build(tri, pos, b.box[0], b.box[1], 8))
    return _cache["soup20000"]


# ---- device == spec ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 8, 64])
@pytest.mark.parametrize("name", ss.NAMES)
def test_device_build_equals_spec(name, radius):
    tri, pos = ss.scene(name)
    b = _check(tri, pos, radius, name)
    r = b.res
    print("%s R=%d: %d tris, %d rounds, height %d, %.3f ms (check %.3f, sort %.3f, emit %.3f, rounds %.3f, tail %.3f)"
          % (name, radius, tri.shape[0], r.numRounds, r.height, r.seconds * 1e3, r.mortonMs, r.sortMs, r.emitMs, r.roundsMs, r.tailMs))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_meshes_equal_spec(n):
    tri, pos = _soup(n, 40 + n)
    for radius in (1, 8, 64):
        _check(tri, pos, radius, n)


@pytest.mark.parametrize("radius", [8, 64])
@pytest.mark.parametrize("n", sorted({TAIL - 1, TAIL, TAIL + 1, TILE - 1, TILE + 1, 2 * TILE + 1}))
def test_sizes_around_the_tail_and_the_tile_equal_spec(n, radius):
    """One more cluster than the tail holds makes one round of launches; one more than a tile makes a second workgroup whose halo
    reaches back over the tile edge; 2 * TILE + 1 has a tile with a halo on both sides."""
    tri, pos = _soup(n, 7)
    b = _check(tri, pos, radius, n)
    assert (b.res.tailClusters == n) == (n <= TAIL)


def test_soup_20000_equals_spec():
    tri, pos, cam, b, ref = _soup20000()
    _assert_equal_to_spec(b, ref, "soup20000")
    assert sum(s > 2 * TILE for s in ref["sizes"]) >= 3      # several rounds of more than two tiles before the tail
    r = b.res
    print("soup20000: %d rounds, tail at %d, height %d, %.3f ms (check %.3f, sort %.3f, emit %.3f, rounds %.3f, tail %.3f)"
          % (r.numRounds, r.tailClusters, r.height, r.seconds * 1e3, r.mortonMs, r.sortMs, r.emitMs, r.roundsMs, r.tailMs))


def test_identical_triangles_tie_across_every_tile_edge():
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0.5)] * 3000, F)
    tri = np.arange(9000, dtype=np.int32).reshape(-1, 3)
    for radius in (1, 8):
        b = _check(tri, pos, radius, "identical3000")
        assert b.res.numRounds == 12                         # 3000, 1500, 750, 375, 188, ...: the list halves


@pytest.mark.parametrize("n", [90, TAIL + 50])
def test_nested_chain_equals_spec(n):
    """n = 90: 89 tail rounds of one merge each, height 89.  n = TAIL + 50: the chain crosses the hand-over (sizes that 1.25 ** k
    cannot reach in binary32: np_bvh_ploc.nested_long); its height is beyond what may be traced, so the call reports it -- and the
    bytes it wrote are still the spec's."""
    tri, pos = pl.nested_scene(n) if n <= pl.MAX_HEIGHT else pl.nested_long(n)
    box = pl.scene_box(pos)
    if n <= pl.MAX_HEIGHT:
        b = _check(tri, pos, 8, n)
        assert b.res.height == n - 1 and b.res.numRounds == n - 1
        return
    d_tri, d_pos = up(tri), up(pos)
    caps = nt.lbvh_capacity(n)
    bufs = [torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in caps]
    with pytest.raises(nt.NtrError) as e:
        nt.ploc_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), box[0], box[1], bufs[0].data_ptr(), caps[0], bufs[1].data_ptr(),
                      caps[1], bufs[2].data_ptr(), caps[2], 8)
    assert e.value.code == -6
    ref = pl.build(tri, pos, box[0], box[1], 8)
    assert ref["stats"]["height"] == n - 1 and ref["sizes"][50] == TAIL
    assert np.array_equal(bufs[0].cpu().numpy()[:ref["nodes"].nbytes].view(np.int32).reshape(-1, 16), ref["nodes"])
    assert _woop_equal(bufs[1].cpu().numpy()[:ref["woop"].nbytes], ref["woop"])
    assert np.array_equal(bufs[2].cpu().numpy()[:ref["tri_index"].nbytes].view(np.int32), ref["tri_index"])


def test_seeded_soups_equal_spec():
    rng = np.random.default_rng(20261018)
    for i in range(50):
        n = int(rng.integers(1, 5001))
        kind = i % 4
        if kind == 0:
            tri, pos = _soup(n, int(rng.integers(1 << 30)))
        elif kind == 1:   # a grid of coordinates: equal codes, equal distances, flat and degenerate triangles
            pos = rng.integers(-4, 5, (3 * n, 3)).astype(F)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        elif kind == 2:   # shared vertices, some degenerate triangles
            pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
            tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
        else:             # tiny extents and -0 / +0 coordinates
            pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)
            pos[rng.random(pos.shape) < 0.2] = F(-0.0)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        _check(tri, pos, (1, 8, 3, 64, 17)[i % 5], (i, n, kind))


# ---- overflow ---------------------------------------------------------------------------------------------------------------------
def test_a_tree_higher_than_the_tracer_stack_is_an_overflow():
    tri, pos = pl.nested_scene(120)
    with pytest.raises(nt.NtrError) as e:
        _Built(tri, pos)
    assert e.value.code == -6 and "height 119" in str(e.value)


# ---- trace records ----------------------------------------------------------------------------------------------------------------
def test_trace_records_equal_oracle_under_every_kernel():
    tri, pos, cam, b, _ = _soup20000()
    view = nt.BvhView(b.d_nodes.data_ptr(), b.res.nodesBytes, b.d_woop.data_ptr(), b.res.triWoopBytes, b.d_idx.data_ptr())
    view.validate()
    rays, _ = scenes.primary_rays(cam, 128, 128)
    d_rays = up(rays)
    for any_hit in (False, True):
        ref, _ = oracle.trace(b.nodes, b.woop, b.idx, rays, any_hit=any_hit, threads=THREADS)
        for kernel in nt.KERNELS:
            d_res = torch.full((rays.shape[0] * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
            view.trace(kernel, rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr())
            torch.cuda.synchronize()
            assert_parity(d_res.cpu().numpy().view(nt.RESULT_DTYPE), ref, "%s anyHit=%d" % (kernel, any_hit))
    assert (ref["id"] >= 0).any()


# ---- the calls downstream -----------------------------------------------------------------------------------------------------------
def _same_float(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def test_validate_and_sah_cost():
    tri, pos, cam, b, _ = _soup20000()
    flags = nt.bvh_validate(b.d_nodes.data_ptr(), b.res.nodesBytes)
    assert flags & nt.BVH_FINITE and flags & nt.BVH_ORDERED
    got = nt.bvh_sah_cost(b.d_nodes.data_ptr(), b.res.nodesBytes, b.d_woop.data_ptr(), b.res.triWoopBytes)
    ref = op.sah_cost(b.nodes, b.woop)
    assert _same_float(got.sahCost, ref["sahCost"]), (got.sahCost, ref["sahCost"])
    assert (got.numNodes, got.numLeaves, got.numTris, got.height) == (ref["numNodes"], ref["numLeaves"], ref["numTris"], ref["height"])
    assert got.numTris == b.n and got.height == b.res.height
    print("soup20000 sahCost %r, height %d" % (got.sahCost, got.height))


def test_refit_with_unmoved_vertices_changes_nothing():
    tri, pos = ss.scene("soup1000")
    b = _Built(tri, pos)
    nt.bvh_refit(*b.ptrs(), b.n, b.d_tri.data_ptr(), b.nv, b.d_pos.data_ptr(), 0.0)
    torch.cuda.synchronize()
    r = b.res
    assert np.array_equal(b.d_nodes.cpu().numpy()[:r.nodesBytes].view(np.int32).reshape(-1, 16), b.nodes)
    assert np.array_equal(b.d_woop.cpu().numpy()[:r.triWoopBytes], b.woop)
    assert np.array_equal(b.d_idx.cpu().numpy()[:r.triIndexBytes].view(np.int32), b.idx)


def test_one_optimise_pass_equals_the_spec_on_the_spec_tree():
    tri, pos = _soup(5000, 5)
    b = _Built(tri, pos)
    spec = pl.build(tri, pos, b.box[0], b.box[1], 8)
    want = op.optimize(spec["nodes"], passes=1)
    res = nt.bvh_optimize(b.d_nodes.data_ptr(), b.res.nodesBytes, 1)
    torch.cuda.synchronize()
    got = b.d_nodes.cpu().numpy()[:b.res.nodesBytes].view(np.int32).reshape(-1, 16)
    assert np.array_equal(got, want["nodes"])
    assert res.formed[0] == want["passes"][0]["formed"] and res.rewritten[0] == want["passes"][0]["rewritten"]


def test_reorder_equals_spec():
    tri, pos = _soup(5000, 5)
    b = _Built(tri, pos)
    want = ro.reorder(b.nodes.view(np.uint8).reshape(-1), b.woop, b.idx.view(np.uint8))
    r = b.res
    out = [torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in (r.nodesBytes, r.triWoopBytes, r.triIndexBytes)]
    res = nt.bvh_reorder(*b.ptrs(), out[0].data_ptr(), r.nodesBytes, out[1].data_ptr(), r.triWoopBytes, out[2].data_ptr(), r.triIndexBytes)
    torch.cuda.synchronize()
    for o, e, key in zip(out, (res.nodesBytes, res.triWoopBytes, res.triIndexBytes), ("nodes", "woop", "tri_index")):
        assert o.cpu().numpy()[:e].tobytes() == want[key].tobytes(), key


# ---- determinism and scratch --------------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.ploc_scratch_bytes() == 0
    tri, pos = _soup(6000, 3)
    a = _Built(tri, pos)
    held = nt.ploc_scratch_bytes()
    assert held > 0
    c = _Built(tri, pos)
    assert nt.ploc_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.ploc_scratch_bytes() == 0
    d = _Built(tri, pos)
    for other in (c, d):
        for x, y in ((a.nodes, other.nodes), (a.woop, other.woop), (a.idx, other.idx)):
            assert x.tobytes() == y.tobytes()
    print("scratch: %.1f B per triangle" % (held / tri.shape[0]))
    nt.lbvh_release_workspace()
    assert nt.ploc_scratch_bytes() == 0


# ---- the error table ------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    tri, pos = ss.scene("cornell")
    d_tri, d_pos = up(tri), up(pos)
    n, nv = tri.shape[0], pos.shape[0]
    caps = nt.lbvh_capacity(n)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps]
    mn, mx = pl.scene_box(pos)
    good = dict(num_tris=n, d_tri=d_tri.data_ptr(), num_verts=nv, d_pos=d_pos.data_ptr(), scene_min=mn, scene_max=mx,
                d_nodes=bufs[0].data_ptr(), nodes_cap=caps[0], d_woop=bufs[1].data_ptr(), woop_cap=caps[1], d_idx=bufs[2].data_ptr(),
                idx_cap=caps[2], radius=8)
    inf_box, nan_box, swapped = mx.copy(), mn.copy(), mn.copy()
    inf_box[1] = np.inf
    nan_box[2] = np.nan
    swapped[0] = mx[0] + 1
    cases = [dict(num_tris=0), dict(num_tris=1 << 28), dict(num_verts=0), dict(d_tri=0), dict(d_pos=0), dict(radius=0), dict(radius=65),
             dict(radius=-1), dict(scene_max=inf_box), dict(scene_min=nan_box), dict(scene_min=swapped), dict(d_nodes=0), dict(d_woop=0),
             dict(d_idx=0), dict(nodes_cap=caps[0] - 1), dict(woop_cap=caps[1] - 1), dict(idx_cap=caps[2] - 1)]
    for change in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.ploc_build(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    assert not any(x.any().item() for x in bufs)             # refused before any device work
    # null scene box pointers and a null result, through the raw entry point; a failed call zeroes *result
    L = nt.lib()
    res = nt.PlocResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    box = (C.c_float * 3)(*[float(x) for x in mn]), (C.c_float * 3)(*[float(x) for x in mx])
    tail = (bufs[0].data_ptr(), caps[0], bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(), caps[2])
    assert L.ntr_ploc_build(n, d_tri.data_ptr(), nv, d_pos.data_ptr(), None, box[1], 8, *tail, C.byref(res), None) == -1
    assert bytes(res) == bytes(C.sizeof(res))
    assert L.ntr_ploc_build(n, d_tri.data_ptr(), nv, d_pos.data_ptr(), box[0], box[1], 8, *tail, None, None) == -1
    assert L.ntr_ploc_scratch_bytes(None) == -1
    # found on the device: a vertex index out of range is reported, nothing is written and *result is zeroed
    for bad_index in (nv, -1):
        bad = tri.copy()
        bad[3, 1] = bad_index
        d_bad = up(bad)
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        assert L.ntr_ploc_build(n, d_bad.data_ptr(), nv, d_pos.data_ptr(), box[0], box[1], 8, *tail, C.byref(res), None) == -1
        assert b"vertex index" in L.ntr_last_error() and bytes(res) == bytes(C.sizeof(res))
        torch.cuda.synchronize()
        assert not any(x.any().item() for x in bufs)
    r = nt.ploc_build(**good)
    assert (r.numNodes, r.numLeaves, r.tailClusters) == (33, 34, 34) and r.seconds > 0
