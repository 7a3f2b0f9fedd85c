"""The spec of ntr_bvh_optimize_batch / ntr_bvh_sah_cost_batch (tests/np_optimize_batch.py) on the CPU: what the restructuring of a
pool's BLASes leaves alone (every byte outside the listed node ranges, all rows, every BLAS's node-0 union box and with it the
top-level tree, every leaf box a later refit writes), that a subset in any order is the per-entry loop, that a BLAS too small for a
treelet never changes, and what it is worth: the recorded SAH costs of refitted, restructured and rebuilt trees, and that the binary64
cost does not rise from pass to pass on any of the recorded inputs."""
import numpy as np
import pytest

from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_optimize as opt
import np_bvh_ploc as pl
import np_bvh_refit as rf
import np_instanced as ni
import np_optimize_batch as ob
import np_ploc_batch as pb
import np_refit_batch as rb
import np_tlas_refit as tr

F = np.float32
SIZES = (1, 2, 6, 7, 8, 63, 65, 300)
GAP_NODES, GAP_ROWS = 3, 5
_cache = {}


def pool():
    """A pool of PLOC BLASes with gaps of 0xAB bytes, refitted to vertices moved by 0.1 so that restructuring finds work.  -> dict(nodes,
    woop, tri_index, ranges, tri, pos (moved), meshes)"""
    if "pool" not in _cache:
        parts = [scenes.random_soup(n, seed=100 + n, walls=False)[:2] for n in SIZES]
        tri, pos, meshes = pb.concat(parts)
        built = pb.build(meshes, tri, pos)
        p = ni.make_pool([(b["nodes"], b["woop"], b["tri_index"]) for b in built["builds"]], gap_nodes=GAP_NODES, gap_rows=GAP_ROWS)
        listed_n, listed_w = np.zeros(p["nodes"].size, bool), np.zeros(p["woop"].size, bool)
        for no, nb, wo, wb in p["ranges"]:
            listed_n[no:no + nb] = True
            listed_w[wo:wo + wb] = True
        p["nodes"][~listed_n] = 0xAB
        p["woop"][~listed_w] = 0xAB
        moved = rf.deform(pos, 0.1)
        entries = [(r, m[0], m[1], 0.0) for r, m in zip(p["ranges"], meshes)]
        r = rb.refit(entries, p["nodes"], p["woop"], p["tri_index"], tri, moved)
        _cache["pool"] = dict(nodes=r["nodes"], woop=r["woop"], tri_index=p["tri_index"], ranges=p["ranges"], tri=tri, pos=moved, meshes=meshes,
                              listed=listed_n)
        for v in (_cache["pool"]["nodes"], _cache["pool"]["woop"], _cache["pool"]["tri_index"]):
            v.setflags(write=False)
    return _cache["pool"]


def optimised(passes=2):
    if ("opt", passes) not in _cache:
        p = pool()
        _cache[("opt", passes)] = ob.optimize(p["ranges"], p["nodes"], passes)
    return _cache[("opt", passes)]


def _union0(nodes, r):
    """The union of the two child boxes of a BLAS's slot 0, as float32 bits (min of the lows, max of the highs: exact)."""
    w = nodes[r[0]:r[0] + 48].view(F)
    lo = np.minimum(w[[0, 2, 8]], w[[4, 6, 10]])
    hi = np.maximum(w[[1, 3, 9]], w[[5, 7, 11]])
    return np.concatenate([lo, hi]).view(np.uint32)


def test_only_the_listed_node_ranges_change():
    p, o = pool(), optimised()
    assert o["nodes"].shape == p["nodes"].shape and o["nodes"].dtype == np.uint8
    assert np.array_equal(o["nodes"][~p["listed"]], p["nodes"][~p["listed"]]) and (o["nodes"][~p["listed"]] == 0xAB).all()
    assert sum(o["rewritten"]) > 0 and not np.array_equal(o["nodes"], p["nodes"])     # and something does change
    # a selection leaves the unlisted BLASes alone as well
    sel = [p["ranges"][k] for k in (7, 5)]
    s = ob.optimize(sel, p["nodes"], 2)["nodes"]
    keep = p["listed"].copy()
    for no, nb, _, _ in sel:
        keep[no:no + nb] = False
    assert np.array_equal(s[keep], p["nodes"][keep]) and np.array_equal(s[~p["listed"]], p["nodes"][~p["listed"]])
    # the rows are not passed at all: the spec's signature has no woop and no tri_index, and the sah spec only reads them
    costs = ob.sah_costs(p["ranges"], o["nodes"], p["woop"])
    assert [c["numTris"] for c in costs] == list(SIZES)


def test_a_subset_in_scrambled_order_equals_the_per_entry_loop():
    p = pool()
    order = (6, 2, 7, 0, 4)
    got = ob.optimize([p["ranges"][k] for k in order], p["nodes"], 3)
    want = p["nodes"].copy()
    for k in order:
        no, nb = p["ranges"][k][:2]
        want[no:no + nb] = opt.optimize(p["nodes"][no:no + nb], 3)["nodes"].reshape(-1).view(np.uint8)
    assert np.array_equal(got["nodes"], want)
    full = optimised(3)
    for k in order:                              # entries share no byte, so every entry is also what the full selection gives it
        no, nb = p["ranges"][k][:2]
        assert np.array_equal(got["nodes"][no:no + nb], full["nodes"][no:no + nb])
    assert got["formed"] == [sum(full["per_entry"][k]["passes"][q]["formed"] for k in order) for q in range(3)]


def test_the_device_tests_one_pass_at_a_time_form_is_the_spec():
    """test_optimize_batch_gpu.py computes the spec for 1, 2 and 8 passes in one sweep of single passes that stops at a fixed point."""
    from test_optimize_batch_gpu import spec_steps
    p = pool()
    steps = spec_steps(p["ranges"], p["nodes"], (1, 2, 8))
    for c in (1, 2, 8):
        o = optimised(c)
        assert np.array_equal(steps[c]["nodes"], o["nodes"]), c
        assert all(steps[c][k] == o[k] for k in ("formed", "rewritten", "heightBefore", "heightAfter")), c
    assert optimised(2)["errBits"] == [0] * len(SIZES)


def test_the_error_bits_of_malformed_entries():
    p = pool()
    h = p["nodes"].copy()
    no7, no5 = p["ranges"][7][0], p["ranges"][5][0]
    h.view(np.int32)[no7 // 4 + 16 * 5 + 12] = 64 * (p["ranges"][7][1] // 64)      # the first slot behind its own BLAS
    h[no5:no5 + 64] = 0                                                             # a zero-filled slot 0: no tree
    o = ob.optimize(p["ranges"], h, 2)
    assert o["errBits"] == [0, 0, 0, 0, 0, ob.ERR_NO_TREE, 0, ob.ERR_LINK]
    no, nb = p["ranges"][5][:2]
    assert np.array_equal(o["nodes"][no:no + nb], h[no:no + nb])
    c = ob.sah_costs([p["ranges"][7]], h, p["woop"])[0]                             # the cost counts 0 where it cannot follow
    assert c["numTris"] < SIZES[7] and np.isfinite(c["sahCost"])


def test_entries_with_fewer_than_seven_leaf_links_do_not_change():
    p, o = pool(), optimised(8)
    for k, n in enumerate(SIZES):
        no, nb = p["ranges"][k][:2]
        formed = sum(q["formed"] for q in o["per_entry"][k]["passes"])
        if n < 7:
            assert formed == 0 and np.array_equal(o["nodes"][no:no + nb], p["nodes"][no:no + nb]), n
        else:
            assert formed > 0, n


def test_node_zero_unions_and_the_top_level_tree_stay():
    p = pool()
    inst = ni.instances(isc.seeded_transforms(19, 3, spread=20.0, mirrored=2), np.arange(19) % len(SIZES))
    tlas = ni.tlas_build(p["nodes"], p["ranges"], inst)
    for passes in (1, 2, 8):
        o = optimised(passes)
        for r in p["ranges"]:
            assert np.array_equal(_union0(o["nodes"], r), _union0(p["nodes"], r)), (passes, r)
        again = tr.refit(tlas["nodes"], tlas["root_link"], tlas["records"], o["nodes"], p["ranges"], inst)
        assert again["err_bits"] == 0
        assert np.array_equal(again["nodes"], np.asarray(tlas["nodes"]).view(np.int32).reshape(-1, 16))
        assert np.array_equal(again["records"], np.asarray(tlas["records"]).view(np.uint32).reshape(-1, 16))


def _leaf_boxes(nodes, r):
    """{leaf link: its six box words} of the reached slots of BLAS r"""
    ni_ = nodes[r[0]:r[0] + r[1]].view(np.int32).reshape(-1, 16)
    out = {}
    for s in np.concatenate(opt.levels_of(ni_)):
        for k in (0, 1):
            if ni_[s, 12 + k] < 0:
                assert int(ni_[s, 12 + k]) not in out
                out[int(ni_[s, 12 + k])] = ni_[s, opt.BOX_WORDS[k]].tobytes()
    return out


def test_a_refit_after_optimising_writes_the_same_leaf_boxes():
    p, o = pool(), optimised()
    entries = [(r, m[0], m[1], 0.0) for r, m in zip(p["ranges"], p["meshes"])]
    again = rf.deform(p["pos"], 0.05)
    a = rb.refit(entries, p["nodes"], p["woop"], p["tri_index"], p["tri"], again)
    b = rb.refit(entries, o["nodes"], p["woop"], p["tri_index"], p["tri"], again)
    assert np.array_equal(a["woop"].view(np.uint32), b["woop"].view(np.uint32))
    assert a["boxes"].tobytes() == b["boxes"].tobytes() and a["stats"] == b["stats"]
    for r in p["ranges"]:
        la, lb = _leaf_boxes(a["nodes"], r), _leaf_boxes(b["nodes"], r)
        assert la == lb and len(la) >= 1


# ---- what it is worth -------------------------------------------------------------------------------------------------------------------
def _refitted(n, seed, a):
    """-> (nodes, woop, tri, moved pos) of the PLOC tree of random_soup(n, seed) refitted (epsilon 0) to deform(pos, a)"""
    key = ("refitted", n, seed, a)
    if key not in _cache:
        tri, pos, _ = scenes.random_soup(n, seed, walls=False)
        b = pl.build(tri, pos, *pl.scene_box(pos), 8)
        moved = rf.deform(pos, a) if a else np.ascontiguousarray(pos, F)
        r = rf.refit(b["nodes"], b["woop"], b["tri_index"], tri, moved, 0.0)
        _cache[key] = (r["nodes"], r["woop"], tri, moved)
    return _cache[key]


# SAH cost (binary32, np_bvh_optimize.sah_cost) at a = 0.1: the refitted tree, after 1, 2 and 4 passes, a fresh PLOC build
RECORDED = {(300, 7): (15.250, 13.245, 12.692, 12.522, 12.161), (1000, 11): (30.552, 27.044, 25.775, 24.886, 24.140)}


@pytest.mark.parametrize("n,seed", sorted(RECORDED))
def test_the_recorded_costs(n, seed):
    nodes, woop, tri, moved = _refitted(n, seed, 0.1)
    fresh = pl.build(tri, moved, *pl.scene_box(moved), 8)
    got = [opt.sah_cost(nodes, woop)["sahCost"]] + [opt.sah_cost(opt.optimize(nodes, k)["nodes"], woop)["sahCost"] for k in (1, 2, 4)] + \
          [opt.sah_cost(fresh["nodes"], fresh["woop"])["sahCost"]]
    assert ["%.3f" % float(c) for c in got] == ["%.3f" % c for c in RECORDED[(n, seed)]]
    # through the pool spec the same numbers come out
    p = ni.make_pool([(nodes, woop, np.zeros(woop.size // 16, np.int32))], gap_nodes=1)
    c = ob.sah_costs(p["ranges"], ob.optimize(p["ranges"], p["nodes"], 2)["nodes"], p["woop"])[0]
    assert c["sahCost"].tobytes() == F(got[2]).tobytes()


@pytest.mark.parametrize("n,seed", [(6, 7), (7, 7), (8, 7), (63, 7), (65, 7), (300, 7), (1000, 11)])
def test_the_binary64_cost_never_rises_from_pass_to_pass(n, seed):
    for a in (0, 0.1, 0.3):
        nodes, woop, _, _ = _refitted(n, seed, a)
        cost = [opt.sah_cost(nodes, woop, np.float64)["sahCost"]]
        for _ in range(4):
            nodes = opt.optimize(nodes, 1)["nodes"]
            cost.append(opt.sah_cost(nodes, woop, np.float64)["sahCost"])
        assert all(np.isfinite(cost)) and all(y <= x for x, y in zip(cost, cost[1:])), (n, a, cost)
        assert np.array_equal(nodes, opt.optimize(_refitted(n, seed, a)[0], 4)["nodes"])       # four single passes are one call of four
