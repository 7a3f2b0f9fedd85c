"""ntr_bvh_optimize and ntr_bvh_sah_cost on the device: the node buffer (all 64 bytes of every slot) equals the numpy spec
(tests/np_bvh_optimize.py) byte for byte for trees of every builder, passes 1 and 3, between guard bytes that survive; two runs
give the same bytes; the SAH cost equals the spec's binary32 value bit for bit (any NaN equals any NaN) before and after, counts
included; trace records over the optimised tree equal the oracle's for every kernel name; refit, optimise and refit again compose,
each step equal to its spec applied to the previous step's bytes; the hairball optimises, validates and traces without a stack
overflow; the scratch grows, is reported and released.

Brute force runs over the edge rays and every 512th of the 1080p primary rays, as in tests/test_bvh_refit_gpu.py."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_bvh_optimize as op
import np_bvh_refit as rf
import ray_sets
import test_bvh_refit_gpu as tr
import test_persistent_bvh_gpu as tp
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
BUILDERS = tr.BUILDERS
SCENES = ("cornell", "soup1500", "one", "stacked", "flat", "zero_area", "atrium")


def _optimize(d, passes):
    return nt.bvh_optimize(d.ptr(d.d_nodes), d.nb, passes)


def _sah(d):
    return nt.bvh_sah_cost(d.ptr(d.d_nodes), d.nb, d.ptr(d.d_woop), d.wb)


def _same_float(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def _assert_sah_equals_spec(d, nodes, woop, what):
    got, ref = _sah(d), op.sah_cost(nodes, woop)
    assert _same_float(got.sahCost, ref["sahCost"]), (what, got.sahCost, ref["sahCost"])
    assert dict(numNodes=got.numNodes, numLeaves=got.numLeaves, numTris=got.numTris, height=got.height) == \
        {k: ref[k] for k in ("numNodes", "numLeaves", "numTris", "height")}, what
    assert got.seconds > 0
    return got


def _assert_equals_spec(d, before, spec, res, what):
    nodes, woop, idx, _ = d.download()                     # asserts the guard bytes
    assert np.array_equal(woop, before[1]) and np.array_equal(idx, before[2]), "%s: triWoop or triIndex changed" % (what,)
    assert np.array_equal(nodes.view(np.int32).reshape(-1, 16), spec["nodes"]), "%s: nodes differ" % (what,)
    if res is not None:
        n = len(spec["passes"])
        assert res.passes == n and res.seconds > 0
        for key in ("formed", "rewritten", "heightBefore", "heightAfter"):
            assert list(getattr(res, key))[:n] == [p[key] for p in spec["passes"]], (what, key)
        ref = op.sah_cost(before[0], before[1])
        assert res.numNodes == ref["numNodes"], what
    return nodes


@pytest.mark.parametrize("kind", BUILDERS)
@pytest.mark.parametrize("name", SCENES)
def test_device_optimize_equals_spec(name, kind):
    tri, pos = tp._scene(name)
    nodes, woop, idx = tr._tree(name, kind)
    for passes in (1, 3):
        d = tr._Dev(nodes, woop, idx, tri, pos)
        s0 = _assert_sah_equals_spec(d, nodes, woop, (name, kind, "before"))
        res = _optimize(d, passes)
        spec = op.optimize(nodes, passes)
        got = _assert_equals_spec(d, (nodes, woop, idx), spec, res, (name, kind, passes))
        s1 = _assert_sah_equals_spec(d, got, woop, (name, kind, passes, "after"))
        print("%s %s passes %d: %d nodes, formed %s rewritten %s, height %d -> %d, SAH %.4f -> %.4f, %.1f us (sah %.1f us)" % (
            name, kind, passes, res.numNodes, list(res.formed)[:passes], list(res.rewritten)[:passes], res.heightBefore[0],
            res.heightAfter[passes - 1], s0.sahCost, s1.sahCost, res.seconds * 1e6, s1.seconds * 1e6))


def test_seeded_soups_equal_spec():
    rng = np.random.default_rng(20261017)
    for i in range(50):
        n = int(rng.integers(20000, 50001)) if i % 10 == 9 else int(rng.integers(1, 3000))
        if i == 0:
            n = 1
        tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        for kind in ("lbvh", "binned"):
            nodes, woop, idx = tr._build(kind, tri, pos)
            nodes = np.concatenate([nodes, np.zeros(64, np.uint8)])   # a slot no link reaches, inside the extent
            d = tr._Dev(nodes, woop, idx, tri, pos)
            passes = 1 + i % 3
            res = _optimize(d, passes)
            spec = op.optimize(nodes, passes)
            got = _assert_equals_spec(d, (nodes, woop, idx), spec, res, (i, n, kind))
            assert not spec["nodes"][-1].any()
            _assert_sah_equals_spec(d, got, woop, (i, n, kind))


def test_two_runs_give_identical_bytes_and_a_second_call_continues_the_first():
    tri, pos = tp._scene("atrium")
    nodes, woop, idx = tr._tree("atrium", "lbvh")
    a, b, c = (tr._Dev(nodes, woop, idx, tri, pos) for _ in range(3))
    _optimize(a, 3)
    _optimize(b, 3)
    _optimize(c, 1)
    _optimize(c, 2)                                        # passes carry no state but the tree
    ga, gb, gc = a.download()[0], b.download()[0], c.download()[0]
    assert ga.tobytes() == gb.tobytes() == gc.tobytes()


def test_links_outside_the_extent_are_reported_and_never_followed():
    tri, pos = tp._scene("soup1500")
    nodes, woop, idx = tr._tree("soup1500", "lbvh")
    ni = nodes.view(np.int32).reshape(-1, 16).copy()
    inner = np.flatnonzero(ni[:, 12] > 0)
    ni[inner[len(inner) // 2], 12] = 64 * ni.shape[0]      # one slot past the end
    bad = ni.view(np.uint8).reshape(-1)
    d = tr._Dev(bad, woop, idx, tri, pos)
    with pytest.raises(nt.NtrError) as e:
        _optimize(d, 2)
    assert e.value.code == -4 and "link" in str(e.value)
    spec = op.optimize(bad, 2)
    assert spec["bad_links"] == 1
    got = d.download()[0]
    assert np.array_equal(got.view(np.int32).reshape(-1, 16), spec["nodes"])
    with pytest.raises(nt.NtrError) as e:
        _sah(d)
    assert e.value.code == -4


@pytest.mark.parametrize("kind", BUILDERS)
def test_trace_records_over_the_optimised_tree_equal_oracle(kind, monkeypatch):
    tri, pos, cam = scenes.atrium()
    nodes, woop, idx = tr._tree("atrium", kind)
    # As in tests/test_bvh_refit_gpu.py the tree is first refitted to the mesh moved by 2 %: on the undeformed atrium some axis-parallel
    # edge rays run inside faces of boxes and along shared triangle edges, where the traversal of ANY tree (the slab test's 0 * inf)
    # and brute force disagree before the optimiser has done anything.  The fresh trees are traced in the spec, hairball and host tests.
    pos = rf.deform(pos, 0.02)
    d = tr._Dev(nodes, woop, idx, tri, pos)
    d.refit(0.0 if kind == "sah" else 0.001)
    res = _optimize(d, 3)
    assert res.rewritten[0] > 0
    edge = ray_sets.edge_rays(float(np.abs(pos).max()))
    tr._check_records(d, edge, (kind, "edge"), monkeypatch, brute=np.arange(edge.shape[0]))
    if kind in ("sah", "lbvh"):
        prim = scenes.primary_rays(cam, 1920, 1080)[0]
        tr._check_records(d, prim, (kind, "1080p"), monkeypatch, brute=np.arange(0, prim.shape[0], 512))


@pytest.mark.parametrize("kind", ("sah", "lbvh"))
def test_refit_optimise_refit_compose(kind):
    tri, pos = tp._scene("atrium")
    nodes, woop, idx = tr._tree("atrium", kind)
    eps = 0.0 if kind == "sah" else 0.001
    p1, p2 = rf.deform(pos, 0.10), rf.deform(pos, 0.02)
    d = tr._Dev(nodes, woop, idx, tri, p1)
    d.refit(eps)
    s1 = rf.refit(nodes, woop, idx, tri, p1, eps)
    tr._assert_equals_spec(d, idx, s1, what="refit 10 %")
    c0 = _assert_sah_equals_spec(d, s1["nodes"], s1["woop"], "refitted")
    res = _optimize(d, 2)
    s2 = op.optimize(s1["nodes"], 2)
    got = _assert_equals_spec(d, (s1["nodes"], s1["woop"], idx), s2, res, "optimise after refit")
    c1 = _assert_sah_equals_spec(d, got, s1["woop"], "optimised")
    assert c1.sahCost < c0.sahCost
    d.set_pos(p2)
    d.refit(eps)
    s3 = rf.refit(s2["nodes"], s1["woop"], idx, tri, p2, eps)
    tr._assert_equals_spec(d, idx, s3, what="refit after optimise")
    print("%s refit 10 %% SAH %.3f, + 2 passes %.3f (%d + %d treelets rewritten)" % (kind, c0.sahCost, c1.sahCost, res.rewritten[0],
                                                                                 res.rewritten[1]))


def test_arguments_and_capture_are_refused():
    d_buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    for passes in (0, 9, -1):
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_optimize(d_buf.data_ptr(), 128, passes)
        assert e.value.code == -1
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d_buf.fill_(0)   # so that the graph is not empty
        for call in (lambda: nt.bvh_optimize(d_buf.data_ptr(), 128, 1, cs), lambda: nt.bvh_sah_cost(d_buf.data_ptr(), 128, d_buf.data_ptr(), 64, cs)):
            try:
                call()
            except nt.NtrError as e:
                errs.append(e.code)
    assert errs == [-1, -1]


def test_hairball_optimises_validates_and_traces_and_the_scratch_is_released():
    nt.lbvh_release_workspace()
    assert nt.bvh_optimize_scratch_bytes() == 0
    tri, pos, _ = scenes.random_soup(2000, seed=3)
    nodes, woop, idx = tr._build("lbvh", tri, pos)
    _optimize(tr._Dev(nodes, woop, idx, tri, pos), 1)
    small = nt.bvh_optimize_scratch_bytes()
    assert small >= 32 * (nodes.nbytes // 64)
    tri, pos, cam = scenes.hairball()
    nodes, woop, idx = tr._build("lbvh", tri, pos)
    d = tr._Dev(nodes, woop, idx, tri, pos)
    c0 = _sah(d)
    res = _optimize(d, 2)
    big = nt.bvh_optimize_scratch_bytes()
    assert big > small and big >= 32 * (nodes.nbytes // 64)
    c1 = _sah(d)
    assert c1.numNodes == c0.numNodes == res.numNodes and c1.numTris == c0.numTris == tri.shape[0] and c1.numLeaves == c0.numLeaves
    assert c1.sahCost < c0.sahCost and res.rewritten[0] > 0 and c1.height == res.heightAfter[1]
    flags = nt.bvh_validate(d.ptr(d.d_nodes), d.nb)
    assert flags & nt.BVH_FINITE and flags & nt.BVH_ORDERED
    rays = scenes.primary_rays(cam, 256, 256)[0]
    nt.trace_status()
    got = tr._records(tr._trace(d, flags, up(rays), rays.shape[0], "fermi_speculative_while_while", False))
    assert nt.trace_status() == 0
    gn, gw, gi, _ = d.download()
    ref, _ = oracle.trace(gn, gw, gi, rays, threads=16)
    tp._assert_records(got, ref, False, "hairball")
    assert (got["id"] >= 0).mean() > 0.1
    print("hairball %d: %d nodes, 2 passes %.3f ms (rewritten %d + %d), SAH %.3f -> %.3f, height %d -> %d" % (
        tri.shape[0], res.numNodes, res.seconds * 1e3, res.rewritten[0], res.rewritten[1], c0.sahCost, c1.sahCost, res.heightBefore[0],
        res.heightAfter[1]))
    nt.lbvh_release_workspace()
    assert nt.bvh_optimize_scratch_bytes() == 0


def test_known_answers():
    import kat_bvh_optimize as kat
    before, want = kat.before(), kat.after()
    woop = np.full((8, 4), 0x80000000, np.uint32)          # never read by the optimiser
    d = tr._Dev(before.view(np.uint8).reshape(-1), woop.view(np.uint8).reshape(-1), np.zeros(8, np.int32), np.zeros((1, 3), np.int32),
                np.zeros((3, 3), F))
    res = _optimize(d, 1)
    assert (res.formed[0], res.rewritten[0], res.heightBefore[0], res.heightAfter[0]) == (1, 1, kat.HEIGHT_BEFORE, kat.HEIGHT_AFTER)
    assert np.array_equal(d.download()[0].view(np.int32).reshape(-1, 16), want)
    res = _optimize(d, 2)                                  # a fixed point
    assert list(res.rewritten)[:2] == [0, 0] and np.array_equal(d.download()[0].view(np.int32).reshape(-1, 16), want)
    ni, w = kat.sah_tree()
    d = tr._Dev(ni.view(np.uint8).reshape(-1), w.view(np.uint8).reshape(-1), np.zeros(21, np.int32), np.zeros((1, 3), np.int32),
                np.zeros((3, 3), F))
    got = _sah(d)
    assert got.sahCost == kat.SAH_COST
    assert dict(numNodes=got.numNodes, numLeaves=got.numLeaves, numTris=got.numTris, height=got.height) == kat.SAH_COUNTS
