"""The rule of ntr_bvh_reorder on the CPU: the numpy spec's walk equals its closed form; a host tree of ntr_sah_build is a fixed point in
all three buffers; the level-order tree of np_sah_sweep.build, reordered, meets the host tree (links, words 14 and 15 and triIndex
exactly, boxes as values); the rule is idempotent; the hand-derived known answer (kat_bvh_reorder.py); malformed inputs; and the
C-ABI's argument checks, which precede any device work."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import kat_bvh_reorder as kat
import np_bvh_reorder as ro
import np_sah_sweep as sw
import sah_sweep_scenes as ss

F = np.float32
SCENES = ("cornell", "grid", "identical", "one_live", "soup1", "soup2", "dropped_mix", "soup1000", "soup20000")
_cache = {}


def _mesh(name):
    if name == "soup20000":
        return scenes.random_soup(20000, seed=77, walls=False)[:2]
    return ss.scene(name)


def _trees(name, prefs):
    """(host tree, level-order spec tree) as (nodes int32[n, 16], woop uint8, tri_index int32)."""
    if (name, prefs) not in _cache:
        tri, pos = _mesh(name)
        h = nt.sah_build(tri, pos, *prefs)
        host = (h.nodes.view(np.int32).reshape(-1, 16).copy(), h.woop.copy(), h.tri_index.copy())
        s = sw.build(tri, pos, *prefs)
        _cache[(name, prefs)] = (host, (s["nodes"], s["woop"], s["tri_index"]))
    return _cache[(name, prefs)]


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _out(r):
    return r["nodes"], r["woop"], r["tri_index"]


@pytest.mark.parametrize("prefs", ss.LEAF_PREFS)
@pytest.mark.parametrize("name", SCENES)
def test_host_tree_is_a_fixed_point_and_the_level_order_tree_meets_it(name, prefs):
    host, level = _trees(name, prefs)
    r = ro.reorder(*host)                                  # asserts walk == closed form
    assert _same(_out(r), host), "a host tree must come back byte for byte"
    assert r["stats"]["numDroppedSlots"] == 0 and r["bad_links"] == 0 and r["bad_leaves"] == 0
    q = ro.reorder(*level)
    assert q["stats"] == r["stats"]
    gn, hn = q["nodes"], host[0]
    assert gn.shape == hn.shape
    assert np.array_equal(gn[:, 12:], hn[:, 12:]), "links, word 14 or word 15 differ"
    assert np.array_equal(gn[:, :12].view(F), hn[:, :12].view(F)), "box values differ"   # -0 == +0; no NaN boxes in these scenes
    if name != "grid":                                     # the documented -0 / +0 freedom shows on the grid only
        assert np.array_equal(gn, hn)
    assert np.array_equal(q["tri_index"], host[2])
    assert q["woop"].nbytes == host[1].nbytes              # the rows' last bits differ: not compared
    again = ro.reorder(*_out(q))                           # idempotent
    assert _same(_out(again), _out(q))


def test_known_answer():
    ni, w, ti = kat.before()
    want = kat.after()
    r = ro.reorder(ni, w, ti)
    assert np.array_equal(r["nodes"], want[0])
    assert np.array_equal(r["woop"].view(np.uint32).reshape(-1, 4), want[1])
    assert np.array_equal(r["tri_index"], want[2])
    assert r["stats"] == kat.STATS and r["bad_links"] == 0 and r["bad_leaves"] == 0
    # a row-by-row scan would have cut leaf A short at its second row
    assert ro.leaf_length(w[:, 0].tolist(), ~kat.LEAF_ROW["A"]) == (4, False)
    again = ro.reorder(*_out(r))
    assert _same(_out(again), _out(r)) and again["stats"] == dict(kat.STATS, numDroppedSlots=0)


def test_cornell_row_by_row_scan_would_find_false_terminators():
    host, _ = _trees("cornell", (1, 8))
    wx = host[1].view(np.uint32).reshape(-1, 4)[:, 0]
    r = ro.reorder(*host)
    assert (wx == ro.TERM).sum() > r["stats"]["numLeaves"]     # -0.0f in second and third rows of axis-aligned triangles


def test_malformed_links_and_leaves():
    ni, w, ti = kat.before()
    bad = ni.copy()
    bad[6, 12] = 64 * kat.NUM_SLOTS                            # slot 6's empty child: one slot past the end
    bad[3, 12] = ~19                                           # leaf C -> the junk row 19, itself a terminator: fine, 1 row
    bad[5, 12] = ~16                                           # leaf A -> row 16, then 19 (a terminator): 4 rows
    r = ro.reorder(bad, w, ti)
    assert r["bad_links"] == 1 and r["bad_leaves"] == 0 and r["nodes"][3, 12] == 64 * kat.NUM_SLOTS
    bad[3, 12] = ~18
    bad[5, 12] = ~15                                           # rows 15 (x = 0x80000000): a terminator at once
    assert ro.reorder(bad, w, ti)["stats"]["numRows"] == 23 - 3
    bad[5, 12] = ~0                                            # rows 0, 3, 6, 9, 12, 15: ends at 15
    assert ro.reorder(bad, w, ti)["stats"]["numRows"] == 23 - 4 + 16
    w2 = w.copy()
    w2[19, 0] = 1                                              # no terminator after row 16 any more
    bad[5, 12] = ~16
    r = ro.reorder(bad, w2, ti)
    assert r["bad_leaves"] == 1 and r["stats"]["numRows"] == 23 - 3
    row = ~int(r["nodes"][1, 12])
    assert (r["woop"].view(np.uint32).reshape(-1, 4)[row] == ro.TERM).all() and r["tri_index"][row] == 0
    cyc = ni.copy()
    cyc[6, 12] = 64 * 2                                        # slot 6 links back to its parent
    with pytest.raises(AssertionError):
        ro.reorder(cyc, w, ti)


# ---- C-ABI surface ------------------------------------------------------------------------------------------------------

def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_entry_points_are_exported_and_bound():
    L = nt.lib()
    for name in ("ntr_bvh_reorder", "ntr_bvh_reorder_scratch_bytes"):
        assert hasattr(L, name)
    assert C.sizeof(nt.BvhReorderResult) == 48
    assert L.ntr_bvh_reorder_scratch_bytes(None) == -1
    v = C.c_int64(-1)
    assert L.ntr_bvh_reorder_scratch_bytes(C.byref(v)) == 0 and v.value == 0


def test_argument_checks_precede_device_work():
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data                                        # fake non-null "device" pointers: never dereferenced
    good = dict(d_nodes=p, nodes_bytes=128, d_woop=p + 4096, woop_bytes=160, d_idx=p + 8192, idx_bytes=40,
                d_out_nodes=p + 16384, out_nodes_capacity=128, d_out_woop=p + 20480, out_woop_capacity=160,
                d_out_idx=p + 24576, out_idx_capacity=40)
    cases = [(dict(d_nodes=0), "d_nodes"), (dict(d_woop=0), "d_triWoop"), (dict(d_idx=0), "d_triIndex"),
             (dict(d_out_nodes=0), "d_outNodes"), (dict(d_out_woop=0), "d_outTriWoop"), (dict(d_out_idx=0), "d_outTriIndex"),
             (dict(nodes_bytes=0), "nodesBytes"), (dict(nodes_bytes=100), "nodesBytes"), (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"),
             (dict(woop_bytes=0), "triWoopBytes"), (dict(woop_bytes=24), "triWoopBytes"), (dict(idx_bytes=36), "triIndexBytes"),
             (dict(idx_bytes=-4), "triIndexBytes"),
             (dict(out_nodes_capacity=0), "outNodesCapacity"), (dict(out_woop_capacity=0), "outTriWoopCapacity"),
             (dict(out_idx_capacity=0), "outTriIndexCapacity"), (dict(out_nodes_capacity=-64), "outNodesCapacity"),
             # an output range that overlaps an input range: the same buffer, a partial overlap from either side, one byte
             (dict(d_out_nodes=p), "overlaps d_nodes"), (dict(d_out_nodes=p + 64), "overlaps d_nodes"),
             (dict(d_out_nodes=p - 127), "overlaps d_nodes"), (dict(d_out_woop=p + 4096 + 159), "overlaps d_triWoop"),
             (dict(d_out_idx=p + 8192 - 39), "overlaps d_triIndex"), (dict(d_out_woop=p + 100), "overlaps d_nodes"),
             (dict(d_out_nodes=p + 8192 + 8), "overlaps d_triIndex"), (dict(d_out_idx=p + 4096), "overlaps d_triWoop"),
             (dict(d_out_woop=p + 16384), "overlaps d_outNodes")]
    for change, word in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_reorder(**dict(good, **change))
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    a = [good[k] for k in ("d_nodes", "nodes_bytes", "d_woop", "woop_bytes", "d_idx", "idx_bytes", "d_out_nodes", "out_nodes_capacity",
                           "d_out_woop", "out_woop_capacity", "d_out_idx", "out_idx_capacity")]
    assert nt.lib().ntr_bvh_reorder(*a, None, None) == -1 and "result" in nt.lib().ntr_last_error().decode()   # result is required
    # ranges that only touch do not overlap
    touching = dict(good, d_out_nodes=p + 128, d_woop=p + 256, d_out_woop=p + 256 + 160)
    if not _has_device():   # valid arguments and no device: no CPU fallback
        for args in (good, touching):
            with pytest.raises(nt.NtrError) as e:
                nt.bvh_reorder(**args)
            assert e.value.code in (-2, -3)
        assert not buf.any()
