"""The PLOC rule (tests/np_bvh_ploc.py) on the CPU, without the library's device code: the tree's structure, a known answer worked
by hand, ties, the nested chain, traversal against brute force, and the quality condition against the oracle's LBVH."""
import numpy as np
import pytest

from ntrace_amd import scenes
from oracle import oracle

import kat_bvh_ploc as kat
import np_bvh_optimize as op
import np_bvh_ploc as pl
import np_hlbvh
import ray_sets
import sah_sweep_scenes as ss

F = np.float32
_cache = {}


def _build(name, radius=8):
    """(tri, pos, spec tree) of a named scene, built once per (name, radius)."""
    if (name, radius) not in _cache:
        if name == "soup20000":
            tri, pos = scenes.random_soup(20000, seed=5)[:2]
        else:
            tri, pos = ss.scene(name)
        _cache[(name, radius)] = (tri, pos, pl.build(tri, pos, *pl.scene_box(pos), radius))
    return _cache[(name, radius)]


def _check_structure(tri, pos, r):
    """Every triangle in exactly one leaf; N - 1 reached slots from the root at slot 0; every stored child box the union below it."""
    n = tri.shape[0]
    ni, nf = r["nodes"], r["nodes"].view(F)
    w = r["woop"].view(np.uint32).reshape(-1, 4)
    ti = r["tri_index"]
    assert ni.shape[0] == max(n - 1, 1) and w.shape[0] == ti.shape[0]
    seen_tri, seen_slot = np.zeros(n, int), np.zeros(ni.shape[0], int)
    v = pos[tri]
    t_lo, t_hi = np_hlbvh.f2i(v).min(axis=1), np_hlbvh.f2i(v).max(axis=1)

    def child_box(slot, k):
        b = nf[slot]
        lo = np.array([b[4 * k], b[4 * k + 2], b[8 + 2 * k]], F)
        hi = np.array([b[4 * k + 1], b[4 * k + 3], b[9 + 2 * k]], F)
        return np_hlbvh.f2i(lo), np_hlbvh.f2i(hi)

    # children before parents: slots are handed out from the top, so a child's slot is above its parent's
    below = {}
    for slot in range(ni.shape[0] - 1, -1, -1):
        boxes = []
        for k in (0, 1):
            c = int(ni[slot, 12 + k])
            lo, hi = child_box(slot, k)
            if c < 0:
                row = ~c
                if w[row, 0] == pl.TERM:          # the empty leaf of the one-triangle tree
                    assert n == 1 and k == 0 and (np_hlbvh.i2f(lo) == pl.FLT_MAX).all() and (np_hlbvh.i2f(hi) == -pl.FLT_MAX).all()
                    continue
                t = int(ti[row])
                assert w[row + 3, 0] == pl.TERM and (ti[row + 1:row + 4] == 0).all()
                seen_tri[t] += 1
                want = (t_lo[t], t_hi[t])
            else:
                assert c % 64 == 0 and slot < c // 64 < ni.shape[0]
                seen_slot[c // 64] += 1
                want = below[c // 64]
            assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]), (slot, k)
            boxes.append(want)
        below[slot] = (np.minimum.reduce([b[0] for b in boxes]), np.maximum.reduce([b[1] for b in boxes]))
        assert ni[slot, 14] == 0 and ni[slot, 15] == 0
    assert (seen_tri == 1).all() and (seen_slot[1:] == 1).all() and seen_slot[0] == 0
    assert op.sah_cost(r["nodes"], r["woop"])["numTris"] == n


@pytest.mark.parametrize("radius", [1, 8, 64])
@pytest.mark.parametrize("name", ss.NAMES)
def test_structure(name, radius):
    tri, pos, r = _build(name, radius)
    _check_structure(tri, pos, r)
    st = r["stats"]
    assert st["numRounds"] == len(r["sizes"]) and st["numRounds"] <= max(tri.shape[0] - 1, 0)
    assert st["height"] == op.sah_cost(r["nodes"], r["woop"])["height"]


def test_known_answer():
    tri, pos = kat.scene()
    rounds = []
    r = pl.build(tri, pos, kat.SCENE_MIN, kat.SCENE_MAX, kat.RADIUS, trace_rounds=rounds)
    assert [nn.tolist() for nn, _ in rounds] == kat.NN
    assert [low.tolist() for _, low in rounds] == kat.MERGED_LOW
    assert r["sizes"] == kat.SIZES and r["stats"] == kat.STATS
    assert np.array_equal(r["nodes"], kat.nodes())
    assert np.array_equal(r["tri_index"], kat.tri_index())
    w = r["woop"].view(np.uint32).reshape(-1, 4)
    assert (w[3::4] == pl.TERM).all()
    rows = np_hlbvh.woop_rows(tri, pos).view(np.uint32).reshape(-1, 3, 4)
    assert np.array_equal(w.reshape(-1, 4, 4)[:, :3], rows[kat.SORTED_IDS])
    _check_structure(tri, pos, r)


def test_identical_triangles_halve_per_round():
    for radius in (1, 8, 64):
        tri, pos, r = _build("identical", radius)
        assert r["sizes"] == [40, 20, 10, 5, 3, 2] and r["stats"]["numRounds"] == 6


@pytest.mark.parametrize("n", [90, 120])
def test_nested_scene_is_a_chain(n):
    tri, pos = pl.nested_scene(n)
    rounds = []
    r = pl.build(tri, pos, *pl.scene_box(pos), 8, trace_rounds=rounds)
    assert all(low.tolist() == [0] for _, low in rounds)          # one merge per round, at the small end
    assert r["stats"]["height"] == n - 1 and r["stats"]["numRounds"] == n - 1
    assert (r["stats"]["height"] > pl.MAX_HEIGHT) == (n == 120)
    _check_structure(tri, pos, r)


def test_long_nested_scene_is_a_chain_too():
    tri, pos = pl.nested_long(1100)
    r = pl.build(tri, pos, *pl.scene_box(pos), 8)
    assert r["stats"]["height"] == 1099 and r["sizes"] == list(range(1100, 1, -1))


def test_one_triangle():
    tri, pos = ss.scene("soup1")
    r = pl.build(tri, pos, *pl.scene_box(pos), 8)
    assert r["stats"] == dict(numNodes=1, numLeaves=2, numRounds=0, height=1)
    assert r["nodes"][0, 12] == ~0 and r["nodes"][0, 13] == ~1 and r["tri_index"].tolist() == [0, 0, 0, 0, 0]
    w = r["woop"].view(np.uint32).reshape(-1, 4)
    assert (w[0] == pl.TERM).all() and (w[4] == pl.TERM).all() and w[1, 0] != pl.TERM
    _check_structure(tri, pos, r)


def test_traversal_equals_brute_force():
    """Closest-hit t through the spec tree equals brute force over the same rows, for ray_sets' edge rays, a primary batch and random
    rays.  One kind of edge ray cannot meet brute force whatever the tree: with tmax = +inf a Woop test can saturate to t = FLT_MAX
    (an axis-parallel ray beside a triangle), which brute force accepts from whichever triangle gives it first; that is no distance
    any box of the scene contains, so a traversal reaches such a triangle only by the way.  Where brute force reports exactly FLT_MAX
    on such a ray, the tree's record is that same t or a miss; every other record is compared bit for bit."""
    tri, pos, r = _build("soup1000")
    cam = scenes.random_soup(1000, seed=1100, walls=False)[2]
    for rays in (ray_sets.edge_rays(), scenes.primary_rays(cam, 48, 48)[0], scenes.random_rays(2048, 5, extent=float(np.abs(pos).max()) + 1.0)):
        got, _ = oracle.trace(r["nodes"], r["woop"], r["tri_index"], rays)
        ref = oracle.bruteforce_closest(r["woop"], r["tri_index"], rays)
        saturated = np.isposinf(rays["tmax"]) & (ref["id"] >= 0) & (ref["t"] == pl.FLT_MAX)
        assert ((got["id"][saturated] < 0) | (got["t"][saturated] == pl.FLT_MAX)).all()
        ok = ~saturated
        assert np.array_equal(got["t"].view(np.uint32)[ok], ref["t"].view(np.uint32)[ok])
        assert np.array_equal(got["id"][ok] >= 0, ref["id"][ok] >= 0) and (ref["id"][ok] >= 0).any()
        assert saturated.sum() * 8 < rays.shape[0]


@pytest.mark.parametrize("name", ["cornell", "soup1000", "soup20000"])
def test_radius_8_beats_the_lbvh(name):
    """A condition: the spec tree's binary64 SAH cost at radius 8 is below the oracle's LBVH (leaf size 8).  A numpy prototype of the
    rule gave 12.70 < 20.20, 30.56 < 46.27 and 141.25 < 191.60."""
    tri, pos, r = _build(name)
    lb = oracle.lbvh_build(tri, pos, 8, 0.001)
    mine = op.sah_cost(r["nodes"], r["woop"], dtype=np.float64)["sahCost"]
    theirs = op.sah_cost(lb["nodes"].view(np.int32).reshape(-1, 16), lb["woop"], dtype=np.float64)["sahCost"]
    print("%s: PLOC R=8 %.2f, LBVH leaf 8 %.2f" % (name, mine, theirs))
    assert mine < theirs
