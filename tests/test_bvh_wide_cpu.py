"""The 4-wide BVH without a device: the spec (tests/np_bvh_wide.py) against a hand-derived known answer and its invariants on trees of
every origin; malformed input; the spec's trace against a binary64 brute force with the binary np_tracer on the same tree as the
yardstick; a 2-child-only wide tree steps exactly as the binary tracer; and the argument checks of the five entry points, which precede
any device work -- without a device the compute calls fail loudly."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import kat_bvh_wide as kat
import np_bvh_wide as wd
import np_tracer
import sah_sweep_scenes as ss
import wide_trees as wt

F = np.float32
TREES = ["cornell", "grid", "identical", "soup1000", "one", "nested90", "sah8", "spread"]


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


# ---- the known answer -------------------------------------------------------------------------------------------------------------------
def test_known_answer_word_for_word():
    r = wd.widen(kat.before())
    assert list(r["kept"]) == kat.KEPT
    want = kat.after()
    assert r["nodes"].shape == want.shape
    for w in range(want.shape[0]):
        assert list(r["nodes"][w]) == list(want[w]), (w, r["nodes"][w], want[w])
    assert r["stats"] == kat.STATS and r["bad_links"] == 0
    # the areas the derivation quotes are the rule's: 192 > 12 at the root, then 160 (two levels down) > 12 (one level down)
    nf = kat.before().view(F)
    area = lambda s, k: float(wd.opt.area(nf[s, wd.BOX[k]]))   # noqa: E731
    assert (area(0, 0), area(0, 1), area(1, 1), area(3, 0), area(4, 1)) == (192.0, 12.0, 160.0, 112.0, 96.0)


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def _reached(ni):
    """(reached slots, their leaf links, every box stored in a reached slot as a row of six words) of a binary tree."""
    S = ni.shape[0]
    seen, stack, leaves, boxes = set([0]), [0], [], set()
    while stack:
        s = stack.pop()
        for k in (0, 1):
            c = int(ni[s, 12 + k])
            boxes.add(tuple(int(x) for x in ni[s, wd.BOX[k]]))
            if c < 0:
                leaves.append(c)
            elif wd._is_inner(c, S) and c // 64 not in seen:
                seen.add(c // 64)
                stack.append(c // 64)
    return seen, leaves, boxes


@pytest.mark.parametrize("name", TREES)
def test_invariants(name):
    ni = wt.tree(name)[0]
    r = wt.wide(name)
    w, st = r["nodes"], r["stats"]
    reached, leaves, boxes = _reached(ni)
    # every reached leaf link of the binary tree appears exactly once
    links = w[:, 12:16]
    assert sorted(links[links < 0].tolist()) == sorted(leaves) and st["numLeafLinks"] == len(leaves)
    # every wide child box is a box of the binary tree, bit for bit
    for k in range(4):
        assert set(map(tuple, w[:, wd.WBOX[k]].tolist())) <= boxes, k
    assert sum(st["counts"]) == st["numNodes"] == w.shape[0]
    assert st["counts"] == [int((w[:, 28] == c).sum()) for c in (2, 3, 4)]
    # unreached slots are dropped: every wide node is a reached slot, and the numbering is the slots' order
    assert set(r["kept"].tolist()) <= reached and (np.diff(r["kept"]) > 0).all() and r["kept"][0] == 0
    if name == "spread":
        assert (r["kept"] % 2 == 0).all() and np.array_equal(w, wt.wide("soup64")["nodes"])
    # empty slots hold slot 0's box and link 0; row 7 is the count and zeros
    for k in range(2, 4):
        empty = w[:, 28] <= k
        assert (links[empty, k] == 0).all() and np.array_equal(w[empty][:, wd.WBOX[k]], w[empty][:, wd.WBOX[0]])
    assert (w[:, 29:32] == 0).all() and ((w[:, 28] >= 2) & (w[:, 28] <= 4)).all()
    # inner links name wide nodes, each once, and never the root
    inner = links[links > 0]
    assert (inner % 128 == 0).all() and sorted((inner // 128).tolist()) == list(range(1, w.shape[0]))
    assert 1 <= st["height"] <= max(wd.binary_height(ni), 1)
    assert st["stackBound"] <= 3 * st["height"]


def test_a_tree_of_two_leaves_is_one_two_child_node():
    ni = wt.tree("leaves2")[0]
    assert ni.shape[0] == 1 and (ni[0, 12:14] < 0).all()
    w = wt.wide("leaves2")["nodes"]
    assert w.shape == (1, 32) and w[0, 28] == 2 and wt.wide("leaves2")["stats"]["counts"] == [1, 0, 0]
    same = [k for k in range(16) if k != 14]
    assert np.array_equal(w[0, same], ni[0, same]) and w[0, 14] == 0


# ---- malformed input --------------------------------------------------------------------------------------------------------------------
def test_a_link_outside_the_extent_becomes_an_empty_slot_and_a_layout_error():
    ni = wt.tree("soup64")[0].copy()
    slot = int(np.flatnonzero(ni[:, 12] > 0)[-1])
    for bad_link in (64 * ni.shape[0], 96, 0x70000000):
        bad = ni.copy()
        bad[slot, 12] = bad_link
        with pytest.raises(wd.LayoutError) as e:
            wd.widen(bad)
        r = e.value.result
        assert r["bad_links"] == 1 and np.array_equal(wd.widen(bad, strict=False)["nodes"], r["nodes"])
        links = r["nodes"][:, 12:16]
        assert (links[links > 0] // 128 < r["nodes"].shape[0]).all() and r["stats"]["numLeafLinks"] < 64


def test_a_cycle_terminates_and_a_slot_named_twice_is_kept_once():
    ni = wt.tree("soup64")[0].copy()
    inner = np.flatnonzero((ni[:, 12] > 0) & (ni[:, 13] > 0))
    deep = int(inner[-1])
    ni[deep, 12] = 64 * int(inner[1])          # back up the tree: a cycle, and a second link to that slot
    r = wd.widen(ni)
    links = r["nodes"][:, 12:16]
    assert r["stats"]["numNodes"] == r["kept"].size <= ni.shape[0] and len(set(r["kept"].tolist())) == r["kept"].size
    assert (links[links > 0] // 128 < r["kept"].size).all()
    self_loop = wt.tree("soup64")[0].copy()
    self_loop[0, 12] = 64 * 1
    self_loop[1, 12] = 64 * 1                   # slot 1 names itself
    assert wd.widen(self_loop)["stats"]["numNodes"] >= 1


# ---- the spec's trace ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup1000"])
def test_spec_trace_against_binary64_brute_force(name):
    """8 192 rays (test_instanced_cpu.py's set).  The yardstick is the binary np_tracer on the same tree against the same brute force:
    the wide spec's hit / miss status mismatches are no more than the binary tracer's own.  Measured:
    cornell     869 hit; binary 0 status mismatches, largest relative t error 1.35e-07; wide 0 and 1.35e-07; 0 rays differ in (id, t)
    soup1000  1 496 hit; binary 0 status mismatches, largest relative t error 4.32e-04; wide 0 and 4.32e-04; 0 rays differ in (id, t)"""
    tri, pos = ss.scene(name)
    nodes, woop, idx = wt.tree(name)
    rays = isc.scene_rays((96, 64), 2048)
    assert rays.shape[0] == 8192
    hit_b, t_b = isc.brute_force(pos.astype(np.float64)[tri], rays)
    bid, bt = np_tracer.trace(nodes, woop, idx, rays)
    wid, wtt, _, _ = wd.trace(wt.wide(name)["nodes"], woop, idx, rays)

    def against_brute(hit, tt):
        both = hit & hit_b
        rel = np.abs(tt[both].astype(np.float64) - t_b[both]) / np.abs(t_b[both])
        return int((hit != hit_b).sum()), (float(rel.max()) if rel.size else 0.0)

    b_status, b_err = against_brute(bid >= 0, bt)
    w_status, w_err = against_brute(wid >= 0, wtt)
    differ = int(((wid != bid) | (wtt.view(np.uint32) != bt.view(np.uint32))).sum())
    print("%s: %d rays, %d hit; binary tracer: %d status mismatches, largest relative t error %.3g; wide spec: %d status mismatches, "
          "largest relative t error %.3g; %d rays differ in (id, t) between the two" % (name, rays.shape[0], int(hit_b.sum()), b_status, b_err,
                                                                                      w_status, w_err, differ))
    assert w_status <= b_status, (w_status, b_status)


def test_a_two_child_only_wide_tree_returns_the_binary_tracers_records():
    nodes, woop, idx = wt.tree("leaves2")
    tri, pos = ss.scene("soup2")
    rays = np.concatenate([wt.rays_for("soup1000"), scenes.box_rays(pos, 2048, 5)])
    w = wt.wide("leaves2")["nodes"]
    for any_hit in (False, True):
        eid, et, est = np_tracer.trace(nodes, woop, idx, rays, any_hit=any_hit, return_stats=True)
        live = rays["tmin"] < rays["tmax"]      # (np_tracer has no degenerate-ray rule of its own: the device front end has it)
        gid, gt, _, _, gst = wd.trace(w, woop, idx, rays[live], any_hit, return_stats=True)
        assert np.array_equal(gid, eid[live]) and np.array_equal(gt.view(np.uint32), et[live].view(np.uint32))
        assert (gid >= 0).any()


# ---- the entry points' argument checks ----------------------------------------------------------------------------------------------------
def test_argument_errors_precede_device_work():
    fake = 0x10000
    L = nt.lib()
    assert nt.bvh_widen_capacity(64) == 128 and nt.bvh_widen_capacity(640) == 1280 and nt.bvh_widen_capacity(0x76543200) == 2 * 0x76543200
    for bad in (0, 32, 100, -64, 0x76543240):
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_widen_capacity(bad)
        assert e.value.code == -1
    assert L.ntr_bvh_widen_capacity(64, None) == -1 and L.ntr_bvh_widen_scratch_bytes(None) == -1
    good = dict(d_nodes=fake, nodes_bytes=640, d_wide_nodes=fake + 4096, wide_capacity=1280)
    for change in (dict(d_nodes=0), dict(d_wide_nodes=0), dict(nodes_bytes=0), dict(nodes_bytes=100), dict(nodes_bytes=0x76543240),
                   dict(wide_capacity=1279), dict(wide_capacity=0), dict(d_wide_nodes=fake), dict(d_wide_nodes=fake + 576),
                   dict(d_wide_nodes=fake - 1216)):
        res = nt.BvhWideResult()
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        a = dict(good, **change)
        rc = L.ntr_bvh_widen(a["d_nodes"], a["nodes_bytes"], a["d_wide_nodes"], a["wide_capacity"], C.byref(res), None)
        assert rc == -1 and bytes(res) == bytes(C.sizeof(res)), (change, L.ntr_last_error())
    assert L.ntr_bvh_widen(fake, 640, fake + 4096, 1280, None, None) == -1
    tgood = dict(num_rays=64, any_hit=False, d_rays=fake, d_results=fake, d_wide_nodes=fake, wide_nodes_bytes=1280, d_woop=fake, woop_bytes=1600,
                 d_tri_index=fake)
    for fn in (nt.trace_wide, nt.trace_wide_stats):
        for change in (dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_wide_nodes=0), dict(d_woop=0), dict(d_tri_index=0),
                       dict(wide_nodes_bytes=0), dict(wide_nodes_bytes=64), dict(wide_nodes_bytes=1344), dict(wide_nodes_bytes=0x76543280),
                       dict(woop_bytes=0), dict(woop_bytes=8), dict(woop_bytes=0xFFFFFF10)):
            with pytest.raises(nt.NtrError) as e:
                fn(**dict(tgood, **change))
            assert e.value.code == -1, (fn.__name__, change, str(e.value))
    assert nt.trace_wide(**dict(tgood, num_rays=0)) == 0.0
    assert nt.trace_wide_stats(**dict(tgood, num_rays=0)).as_dict() == dict(numRays=0, numInnerVisits=0, numTriTests=0, numLeafVisits=0, numHits=0)
    assert L.ntr_trace_wide_stats(64, 0, fake, fake, fake, 1280, fake, 1600, fake, 0, None, None) == -1
    if not _has_device():
        res = nt.BvhWideResult()
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        rc = L.ntr_bvh_widen(fake, 640, fake + 4096, 1280, C.byref(res), None)
        assert rc in (-2, -3) and bytes(res) == bytes(C.sizeof(res)), (rc, L.ntr_last_error())
        for fn in (nt.trace_wide, nt.trace_wide_stats):
            with pytest.raises(nt.NtrError) as e:
                fn(**tgood)
            assert e.value.code in (-2, -3)
        assert nt.bvh_widen_scratch_bytes() == 0
