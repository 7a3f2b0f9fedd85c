"""The numpy spec of the device binned SAH BVH build (tests/np_bvh_binned.py) on hand-derived trees -- four separated triangles,
coincident centroids (the median fallback), empty sides, SAH termination and the depth cap -- plus invariants on seeded soups, the
binning's sweeps against a direct evaluation of every plane, and traces over the spec's tree equal to brute force."""
import numpy as np
import pytest

from ntrace_amd import scenes
from oracle import oracle

import np_bvh_binned as bb
import np_hlbvh

F = np.float32


def _row(xs, y=0.0, z=0.0, s=0.25):
    pos = np.array([v for x in xs for v in [(x, y, z), (x + s, y, z), (x, y + s, z)]], F)
    return np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3), pos


def _leaf_ids(r):
    return [list(map(int, ids)) for _, _, _, _, ids, _ in bb.leaves(r)]


def test_four_separated_triangles():
    """Centroids x = 0.125, 10.125, 20.125, 30.125 in a root box [0, 30.25].  On y and z every centroid lies on one side (NaN
    costs); on x a 1 / 3 split costs 2 * 20.25 * 0.25 * 3 + 2 * 0.25 * 0.25 = 30.5 and the 2 / 2 split 2 * (2 * 10.25 * 0.25 * 2) =
    20.5, reached by planes 4, 5 and 6 (12.60, 15.125, 17.65): the lowest, plane 4, wins.  Side -1 -- centroids at or above the plane --
    is child 0, so child 0 holds triangles 2, 3 and child 1 triangles 0, 1; one level below, the same rule puts 3 before 2, 1 before 0."""
    tri, pos = _row([0.0, 10.0, 20.0, 30.0])
    levels = []
    r = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=0), trace_levels=levels)
    nodes = r["nodes"]
    assert nodes.shape == (3, 16)
    assert levels[0]["k"][0] == 4 and levels[0]["axis"][0] == 0
    assert levels[0]["split"][0] == F(F(0.0) + F(30.25) * (F(5) / F(12)))
    assert nodes[0, 12:16].tolist() == [64, 128, 0, 0]
    assert nodes[1, 12:14].tolist() == [~0, ~4] and nodes[2, 12:14].tolist() == [~8, ~12]
    assert _leaf_ids(r) == [[3], [2], [1], [0]]
    assert r["tri_index"].tolist() == [3, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert (r["woop"].view(np.uint32).reshape(-1, 4)[3::4] == 0x80000000).all()
    # root's child 0 box: triangles 2 and 3 grown by FLT_EPSILON
    eps = bb.FLT_EPSILON
    f = nodes[0].view(F)
    assert f[0] == F(F(20.0) - eps) and f[1] == F(F(30.25) + eps) and f[4] == F(F(0.0) - eps) and f[5] == F(F(10.25) + eps)
    assert r["stats"] == dict(numInnerNodes=3, numLeaves=4, numLevels=3, maxDepth=2, medianFallbacks=0, costLeaves=0, depthLeaves=0)


def test_coincident_centroids_take_the_median():
    tri, pos = _row([1.0] * 8)
    r = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=0))
    assert r["stats"]["medianFallbacks"] == 7 and r["stats"]["numInnerNodes"] == 7
    assert _leaf_ids(r) == [[i] for i in range(8)]
    assert all(int(w) == 0 for w in r["nodes"][:, 14])         # a median split writes axis 0
    # boxes of the median path: the triangles' union grown by epsilon
    f = r["nodes"][0].view(F)
    eps = bb.FLT_EPSILON
    assert f[0] == F(F(1.0) - eps) and f[1] == F(F(1.25) + eps) and f[8] == F(F(0.0) - eps) and f[9] == F(F(0.0) + eps)
    # an odd count: child 0 gets n // 2
    tri, pos = _row([1.0] * 5)
    lv = []
    r = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=0), trace_levels=lv)
    assert _leaf_ids(r) == [[0], [1], [2], [3], [4]]
    assert lv[0]["median"][0] and lv[0]["nl"][0] == 2 and lv[0]["nr"][0] == 3


def test_empty_side_never_wins():
    # an empty side has the box (FLT_MAX, -FLT_MAX): infinite area, times a count of 0 is NaN
    lo, hi = np.full((1, 3), bb.FLT_MAX, F), np.full((1, 3), -bb.FLT_MAX, F)
    with np.errstate(all="ignore"):
        assert np.isnan(bb.area(lo, hi) * F(0))
    # two clusters far apart on x, close on y: every y plane leaves a side empty; the x split separates them
    tri, pos = _row([0.0, 0.5, 100.0, 100.5], y=0.0)
    lv = []
    r = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=0), trace_levels=lv)
    assert lv[0]["axis"][0] == 0 and lv[0]["nl"][0] == 2 and lv[0]["nr"][0] == 2 and not lv[0]["median"][0]
    assert _leaf_ids(r) == [[3], [2], [1], [0]]
    # no split of a seeded soup leaves a side empty
    for seed in range(6):
        tri, pos, _ = scenes.random_soup(300, seed=seed)
        lv = []
        bb.build(tri, pos, params=dict(triLimit=2), trace_levels=lv)
        for d in lv:
            split = ~d["leaf"] | d["ended"]
            assert ((d["nl"][split] > 0) & (d["nr"][split] > 0)).all()


def test_sah_termination():
    # 40 triangles in a row; ct = 1000 ends every task of <= triMaxLimit references
    tri, pos = _row([float(i) for i in range(40)])
    r = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=16, ct=1000.0))
    st = r["stats"]
    assert st["costLeaves"] > 0 and st["depthLeaves"] == 0
    sizes = [len(ids) for ids in _leaf_ids(r)]
    assert all(1 < s <= 16 for s in sizes) and sum(sizes) == 40
    assert st["numLeaves"] == st["costLeaves"]
    # with the default ct the same tasks split on
    r2 = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=16))
    assert r2["stats"]["costLeaves"] == 0 and all(len(ids) == 1 for ids in _leaf_ids(r2))
    # DEVIATION: a root that termination ends is split anyway into two leaves, and is not counted as a cost leaf
    tri, pos = _row([0.0, 10.0, 20.0, 30.0])
    r3 = bb.build(tri, pos, params=dict(triLimit=1, triMaxLimit=100, ct=1000.0))
    assert r3["nodes"].shape[0] == 1 and _leaf_ids(r3) == [[2, 3], [0, 1]] and r3["stats"]["costLeaves"] == 0


def test_depth_cap():
    tri, pos = _row([float(i) for i in range(64)])
    r = bb.build(tri, pos, params=dict(triLimit=1, maxDepth=2))
    st = r["stats"]
    assert st["numInnerNodes"] == 3 and st["numLeaves"] == 4 and st["maxDepth"] == 2 and st["depthLeaves"] == 4
    assert sorted(sum(_leaf_ids(r), [])) == list(range(64))
    r1 = bb.build(tri, pos, params=dict(triLimit=1, maxDepth=1))
    assert r1["stats"]["numInnerNodes"] == 1 and r1["stats"]["depthLeaves"] == 2
    r50 = bb.build(tri, pos, params=dict(triLimit=1))
    assert r50["stats"]["depthLeaves"] == 0 and r50["stats"]["numLeaves"] == 64


def test_one_triangle():
    tri, pos = _row([1.0])
    r = bb.build(tri, pos)
    assert r["nodes"].shape == (1, 16) and r["nodes"][0, 12:14].tolist() == [~0, ~1]
    f = r["nodes"][0].view(F)
    assert (f[[0, 2, 8]] == bb.FLT_MAX).all() and (f[[1, 3, 9]] == -bb.FLT_MAX).all()
    assert _leaf_ids(r) == [[], [0]]
    assert r["stats"]["medianFallbacks"] == 1


def test_binning_equals_direct_plane_evaluation():
    """The sweeps over 12 / 12 / 11 bins give every plane the counts and boxes of a direct test of every triangle."""
    for seed in range(4):
        tri, pos, _ = scenes.random_soup(200, seed=seed, walls=False)
        lv = []
        r = bb.build(tri, pos, params=dict(triLimit=4), trace_levels=lv)
        lo, hi, cen = bb.tri_terms(tri, pos)
        d = lv[0]
        # root: re-evaluate all 32 planes directly and redo the choice
        mn = np_hlbvh.i2f(np_hlbvh.f2i(pos).min(axis=0)).astype(F)
        mx = np_hlbvh.i2f(np_hlbvh.f2i(pos).max(axis=0)).astype(F)
        best = (np.inf, -1)
        for k in range(32):
            a, j = k // 11, k % 11
            p = F(mn[a] + (mx[a] - mn[a]) * bb.RPOS[j])
            neg = bb.side_neg(p, cen[:, a])
            if neg.all() or not neg.any():
                continue
            with np.errstate(all="ignore"):
                s = F(bb.area(lo[neg].min(0), hi[neg].max(0)) * F(neg.sum()) + bb.area(lo[~neg].min(0), hi[~neg].max(0)) * F((~neg).sum()))
            if np.isfinite(s) and s < best[0]:
                best = (s, k)
        assert d["k"][0] == best[1]
        bb.check_invariants(r, tri, pos, dict(triLimit=4))


@pytest.mark.parametrize("seed", range(5))
def test_invariants_and_brute_force(seed):
    tri, pos, cam = scenes.random_soup(800, seed=seed)
    for params in (None, dict(triLimit=1, triMaxLimit=0), dict(triLimit=3, triMaxLimit=32, ct=0.2)):
        r = bb.build(tri, pos, params=params)
        bb.check_invariants(r, tri, pos, params)
        n = tri.shape[0]
        assert r["stats"]["numInnerNodes"] == r["stats"]["numLeaves"] - 1 <= max(n - 1, 1)
        assert r["woop"].nbytes == 16 * (3 * n + r["stats"]["numLeaves"])
        nodes = r["nodes"].reshape(-1).view(np.uint8)
        for rays in (scenes.random_rays(256, seed), scenes.primary_rays(cam, 24, 24)[0]):
            res, _ = oracle.trace(nodes, r["woop"], r["tri_index"], rays)
            bf = oracle.bruteforce_closest(r["woop"], r["tri_index"], rays)
            assert np.array_equal(res["t"].view(np.uint32), bf["t"].view(np.uint32))
            assert np.array_equal(res["id"], bf["id"])


def test_atrium_builds_in_seconds():
    import time
    tri, pos, _ = scenes.atrium()
    t0 = time.time()
    r = bb.build(tri, pos)
    assert time.time() - t0 < 60
    bb.check_invariants(r, tri, pos)
