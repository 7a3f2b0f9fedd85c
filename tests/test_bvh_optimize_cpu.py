"""The treelet rule and the SAH cost (tests/np_bvh_optimize.py) on the CPU, and the C-ABI surface of ntr_bvh_optimize /
ntr_bvh_sah_cost without a device: the spec's output is a tree over the same reached slots and the same (leaf link, box) pairs whose
inner boxes are the unions of their nodes' two boxes; unreached slots and fourth link words stay; every rewritten treelet has
c[full] < c_orig and the SAH cost never rises; a hand-derived treelet and a hand-derived two-node SAH cost; the optimised tree
refits, and its traversal equals brute force; the entry points are exported and check their arguments before any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import kat_bvh_optimize as kat
import np_bvh_optimize as op
import np_bvh_refit as rf
import ray_sets

F = np.float32
np_hlbvh = rf.np_hlbvh
SCENES = ("cornell", "soup1500", "soup300", "one", "stacked", "flat", "zero_area", "atrium")
_scene_cache, _tree_cache = {}, {}


def _tri_scene(corners, s=0.25):
    pos = np.array([v for (x, y, z) in corners for v in [(x, y, z), (x + s, y, z), (x, y + s, z)]], F)
    return np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3), pos


def _scene(name):
    """(tri, pos, camera): cornell, soups, atrium and the degenerate scenes of test_persistent_bvh_gpu._scene."""
    if name in _scene_cache:
        return _scene_cache[name]
    cam = scenes.cornell_box()[2]
    if name == "cornell":
        s = scenes.cornell_box()
    elif name == "soup1500":
        s = scenes.random_soup(1500, seed=11)
    elif name == "soup300":
        s = scenes.random_soup(300, seed=2, walls=False)
    elif name == "atrium":
        s = scenes.atrium()
    elif name == "stacked":
        s = _tri_scene([(0.0, 0.0, 0.0)] * 40) + (cam,)
    elif name == "one":
        s = _tri_scene([(1.0, 2.0, 3.0)]) + (cam,)
    elif name == "flat":
        rng = np.random.default_rng(3)
        pos = rng.uniform(-5, 5, (600, 3)).astype(F)
        pos[:, 2] = 0
        s = (np.arange(600, dtype=np.int32).reshape(-1, 3), pos, cam)
    else:
        assert name == "zero_area"
        import test_persistent_bvh_gpu as tp
        s = tuple(tp._scene(name)) + (cam,)
    _scene_cache[name] = s
    return s


def _tree(name, builder):
    if (name, builder) not in _tree_cache:
        tri, pos, _ = _scene(name)
        if builder == "sah":
            h = nt.sah_build(tri, pos)
            _tree_cache[(name, builder)] = (h.nodes.copy(), h.woop.copy(), h.tri_index.copy(), 0.0)
        else:
            b = oracle.lbvh_build(tri, pos, 8, 0.001)
            _tree_cache[(name, builder)] = (b["nodes"], b["woop"], b["tri_index"], 0.001)
    return _tree_cache[(name, builder)]


def _leaf_pairs(ni, reached):
    """The (leaf link, box words) pairs of the reached slots, sorted."""
    rows = []
    for k in (0, 1):
        c = ni[reached, 12 + k]
        leaf = ~op.inner_mask(c, ni.shape[0])
        rows.append(np.concatenate([c[leaf][:, None], ni[reached[leaf]][:, op.BOX_WORDS[k]]], axis=1))
    a = np.concatenate(rows)
    return a[np.lexsort(a.T[::-1])]


def _check_tree(before, after):
    S = before.shape[0]
    r0, r1 = np.concatenate(op.levels_of(before)), np.concatenate(op.levels_of(after))     # levels_of asserts "a tree"
    assert np.array_equal(np.sort(r0), np.sort(r1)), "the reached slots changed"
    assert np.array_equal(_leaf_pairs(before, r0), _leaf_pairs(after, r1)), "the (leaf link, box) pairs changed"
    for k in (0, 1):
        c = after[r1, 12 + k]
        inner = op.inner_mask(c, S)
        par, ch = r1[inner], c[inner].astype(np.int64) // 64
        u = rf._union(after.view(F)[ch][:, op.BOX_WORDS[0]], after.view(F)[ch][:, op.BOX_WORDS[1]])
        assert np.array_equal(after[par][:, op.BOX_WORDS[k]], u.view(np.int32)), "an inner box is not the union of its node's boxes"
    unreached = np.setdiff1d(np.arange(S), r0)
    assert np.array_equal(before[unreached], after[unreached]), "an unreached slot was written"
    assert np.array_equal(before[:, 15], after[:, 15]), "a fourth link word changed"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_spec_output_is_the_same_tree_restructured_and_never_costs_more(name, builder):
    nodes, woop, idx, eps = _tree(name, builder)
    before = nodes.view(np.int32).reshape(-1, 16)
    if name != "atrium":                                   # a slot no link reaches, with bytes that look like a node
        before = np.concatenate([before, before[:1] + 1])
    cost = [op.sah_cost(before, woop, np.float64)["sahCost"]]
    cur = before
    for p in range(3 if name != "atrium" or builder == "lbvh" else 1):
        out = op.optimize(cur, 1, detail=True)
        info = out["passes"][0]
        _check_tree(cur, out["nodes"])
        # rule 6: rewritten iff strictly better; every other treelet keeps all its bytes (its root's record is enough to tell a change,
        # and the whole-buffer comparison below covers a pass that rewrites nothing)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(info["rewritten_mask"], info["c_full"] < info["c_orig"])
            assert not (info["c_full"] > info["c_orig"]).any(), "c_orig is one of the programme's candidates"
        assert info["rewritten"] == int(info["rewritten_mask"].sum()) and info["formed"] == info["roots"].size
        if info["rewritten"] == 0:
            assert np.array_equal(out["nodes"], cur)
        cost.append(op.sah_cost(out["nodes"], woop, np.float64)["sahCost"])
        if not (np.isnan(cost[-1]) or np.isnan(cost[-2])):
            assert cost[-1] <= cost[-2], (name, builder, cost)
        assert info["heightBefore"] == op.sah_cost(cur, woop)["height"] and info["heightAfter"] == op.sah_cost(out["nodes"], woop)["height"]
        cur = out["nodes"]
    assert np.array_equal(op.optimize(before, len(cost) - 1)["nodes"], cur), "passes compose"
    print("%s %s: SAH (float64) %s, ratios %s" % (name, builder, ["%.4f" % c for c in cost], ["%.4f" % (c / cost[0]) for c in cost[1:]]))
    if name == "atrium":
        assert cost[1] < cost[0]


def test_untouched_treelets_are_byte_identical():
    nodes, woop, idx, eps = _tree("soup1500", "lbvh")
    before = nodes.view(np.int32).reshape(-1, 16)
    out = op.optimize(before, 1, detail=True)
    info = out["passes"][0]
    assert 0 < info["rewritten"] < info["formed"]
    # the root record of a treelet that was not rewritten can only change through a rewritten treelet above or below it that holds
    # the slot; a slot that is in no rewritten treelet at all keeps its bytes
    touched = np.zeros(before.shape[0], bool)
    _, height, _, _ = op.topology(before)
    cur = before.copy()
    for h in np.unique(height[info["roots"]]):
        roots = np.sort(info["roots"][height[info["roots"]] == h])
        t = op.treelets(cur, roots)
        sel = t["c"][:, op.FULL] < t["c_orig"]
        touched[roots[sel]] = True
        touched[t["slots"][sel].reshape(-1)] = True
        op.emit(cur, roots, t, sel)
    assert np.array_equal(cur, out["nodes"])
    assert np.array_equal(out["nodes"][~touched], before[~touched])
    assert (out["nodes"][touched, 14] == 0).all()


def _all_topologies(leaves):
    """Every unordered binary tree over `leaves` as (sum of inner x extents, canonical form); leaves are (name, lo, hi)."""
    if len(leaves) == 1:
        n, lo, hi = leaves[0]
        return [(0, n, lo, hi)]
    out = []
    first, rest = leaves[0], leaves[1:]
    for r in range(len(rest)):
        for other in itertools.combinations(rest, r + 1):
            mine = [first] + [x for x in rest if x not in other]
            for (ca, ta, la, ha) in _all_topologies(mine):
                for (cb, tb, lb, hb) in _all_topologies(list(other)):
                    lo, hi = min(la, lb), max(ha, hb)
                    out.append((ca + cb + (hi - lo), (ta, tb), lo, hi))
    return out


def test_known_answer_treelet():
    before, want = kat.before(), kat.after()
    # the derivation's claims, by enumeration in integers, independent of the spec
    tops = _all_topologies([(n, lo, hi) for n, (lo, hi) in sorted(kat.LEAF.items())])
    assert len(tops) == 10395
    best = min(t[0] for t in tops)
    assert 2 * best + 6 == kat.C_FULL and sum(t[0] == best for t in tops) == 2
    t = op.treelets(before, np.array([0]))
    assert [int(x) for x in t["link"][0]] == [kat.LEAF_LINK[n] for n in "GCADFEB"]
    assert list(t["slots"][0]) == [4, 5, 1, 2, 3]
    assert t["c_orig"][0] == kat.C_ORIG and t["c"][0, op.FULL] == kat.C_FULL
    assert [int(t["choice"][0, s]) for s in (127, 57, 56, 40, 70, 68)] == [57, 1, 40, 8, 2, 4]
    out = op.optimize(before, 1)
    assert out["passes"] == [dict(formed=1, rewritten=1, heightBefore=kat.HEIGHT_BEFORE, heightAfter=kat.HEIGHT_AFTER)]
    assert np.array_equal(out["nodes"], want)
    again = op.optimize(want, 2)                           # the optimum is a fixed point: everything ties with itself
    assert [p["rewritten"] for p in again["passes"]] == [0, 0] and np.array_equal(again["nodes"], want)


def test_known_answer_sah_cost():
    ni, w = kat.sah_tree()
    got = op.sah_cost(ni, w)
    assert got["sahCost"].dtype == F and float(got["sahCost"]) == kat.SAH_COST
    assert {k: got[k] for k in kat.SAH_COUNTS} == kat.SAH_COUNTS
    assert float(op.sah_cost(ni[1:], w)["sahCost"]) == kat.SAH_SLOT1     # slot 1 as a root of its own
    assert float(op.sah_cost(ni, w, np.float64)["sahCost"]) == kat.SAH_COST
    nodes, woop, idx, eps = _tree("one", "lbvh")           # a flat triangle alone: 0 / 0, IEEE gives a NaN, returned as it comes
    assert np.isnan(op.sah_cost(nodes, woop)["sahCost"])


def _closest_t(nodes, woop, idx, rays):
    """The traversal's t as brute force reports it: a ray with tmax = inf that misses keeps inf in the traversal, where the brute force
    starts from the largest finite float."""
    ref, _ = oracle.trace(nodes, woop, idx, rays, threads=8)
    return np.where((ref["id"] < 0) & np.isposinf(ref["t"]), np.finfo(F).max, ref["t"]).astype(F).view(np.uint32)


def _assert_brute_force(nodes, woop, idx, rays, what, input_nodes=None):
    """The traversal's closest t equals brute force's bit for bit, on every ray.  With input_nodes (a host SAH tree, whose boxes are
    exact): on every ray on which the INPUT tree's traversal equals brute force.  An axis-parallel ray that runs inside a face of an
    exact box is missed by the slab test (0 * inf) in any tree, optimised or not -- 79 of the 2883 rays on the cornell box, all of
    them edge rays in the walls' planes; the LBVH's epsilon keeps its boxes clear of that, so there every ray is compared."""
    bf = oracle.bruteforce_closest(woop, idx, rays)["t"].view(np.uint32)
    t = _closest_t(nodes, woop, idx, rays)
    if input_nodes is None:
        assert np.array_equal(t, bf), what
        return
    found = _closest_t(input_nodes, woop, idx, rays) == bf
    assert found.mean() > 0.9, what
    assert np.array_equal(t[found], bf[found]), what


@pytest.mark.parametrize("name", ["cornell", "soup1500", "flat", "zero_area", "atrium"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_optimised_tree_refits_and_traces_like_brute_force(name, builder):
    tri, pos, cam = _scene(name)
    nodes, woop, idx, eps = _tree(name, builder)
    out = op.optimize(nodes, 2)
    o8 = out["nodes"].view(np.uint8).reshape(-1)
    rays = np.concatenate([ray_sets.edge_rays(float(np.abs(pos).max())), scenes.primary_rays(cam, 32, 32)[0]])
    _assert_brute_force(o8, woop, idx, rays, (name, builder), nodes if builder == "sah" else None)
    # the refit works on the restructured tree: unmoved vertices give its boxes back, moved ones a tree that still traces
    same = rf.refit(o8, woop, idx, tri, pos, eps)
    assert np.array_equal(same["nodes"].view(F)[:, :12], out["nodes"].view(F)[:, :12]) and np.array_equal(same["nodes"][:, 12:], out["nodes"][:, 12:])
    p = rf.deform(pos, 0.02)
    moved = rf.refit(o8, woop, idx, tri, p, eps)
    plain = rf.refit(nodes, woop, idx, tri, p, eps)["nodes"].view(np.uint8).reshape(-1) if builder == "sah" else None
    _assert_brute_force(moved["nodes"].view(np.uint8).reshape(-1), moved["woop"], idx, rays, (name, builder, "moved"), plain)


# ---- C-ABI surface ------------------------------------------------------------------------------------------------------

def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_entry_points_are_exported_and_bound():
    L = nt.lib()
    for name in ("ntr_bvh_optimize", "ntr_bvh_optimize_scratch_bytes", "ntr_bvh_sah_cost"):
        assert hasattr(L, name)
    assert C.sizeof(nt.BvhOptimizeResult) == 16 + 4 * 32 + 4 and C.sizeof(nt.BvhSahResult) == 24
    assert L.ntr_bvh_optimize_scratch_bytes(None) == -1
    v = C.c_int64(-1)
    assert L.ntr_bvh_optimize_scratch_bytes(C.byref(v)) == 0 and v.value == 0


def test_argument_checks_precede_device_work():
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    good = dict(d_nodes=p, nodes_bytes=128, passes=1)
    for change, word in [(dict(d_nodes=0), "d_nodes"), (dict(nodes_bytes=0), "nodesBytes"), (dict(nodes_bytes=100), "nodesBytes"),
                         (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"), (dict(passes=0), "passes"), (dict(passes=9), "passes"),
                         (dict(passes=-2), "passes")]:
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_optimize(**dict(good, **change))
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    good = dict(d_nodes=p, nodes_bytes=128, d_woop=p, woop_bytes=160)
    for change, word in [(dict(d_nodes=0), "d_nodes"), (dict(nodes_bytes=32), "nodesBytes"), (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"),
                         (dict(d_woop=0), "d_triWoop"), (dict(woop_bytes=0), "triWoopBytes"), (dict(woop_bytes=24), "triWoopBytes")]:
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_sah_cost(**dict(good, **change))
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    assert nt.lib().ntr_bvh_sah_cost(p, 128, p, 160, None, None) == -1 and "result" in nt.lib().ntr_last_error().decode()
    if not _has_device():   # valid arguments and no device: no CPU fallback
        for call in (lambda: nt.bvh_optimize(p, 128, 1), lambda: nt.bvh_sah_cost(p, 128, p, 160)):
            with pytest.raises(nt.NtrError) as e:
                call()
            assert e.value.code in (-2, -3)
        assert not buf.any()
