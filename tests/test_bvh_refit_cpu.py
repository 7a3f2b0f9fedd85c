"""The refit rule (tests/np_bvh_refit.py) on the CPU, and the C-ABI surface of ntr_bvh_refit without a device: refitting to unmoved
vertices gives the tree back; after every deformation each leaf box is the min / max of its triangles' moved vertices -/+ epsilon
and each inner box the union of its child's two boxes (all nodes), and the oracle's traversal of the refitted buffers equals brute
force over the same rows; node slots no link reaches, links, terminators and an empty leaf's box come back untouched; the entry
points are exported and check their arguments before any device work."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_bvh_refit as rf

F = np.float32
np_hlbvh = rf.np_hlbvh
SCENES = ("cornell", "soup1500", "atrium")
DEFORMATIONS = (0.0, 0.02, 0.3, "collapse")
_scene_cache, _tree_cache = {}, {}


def _scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = {"cornell": scenes.cornell_box, "soup1500": lambda: scenes.random_soup(1500, seed=11),
                              "atrium": scenes.atrium}[name]()
    return _scene_cache[name]


def _tree(name, builder):
    """(nodes uint8, woop uint8, tri_index int32, epsilon) of a host SAH tree (epsilon 0) or the oracle's LBVH (epsilon 0.001)."""
    if (name, builder) not in _tree_cache:
        tri, pos, _ = _scene(name)
        if builder == "sah":
            h = nt.sah_build(tri, pos)
            _tree_cache[(name, builder)] = (h.nodes.copy(), h.woop.copy(), h.tri_index.copy(), 0.0)
        else:
            b = oracle.lbvh_build(tri, pos, 8, 0.001)
            _tree_cache[(name, builder)] = (b["nodes"], b["woop"], b["tri_index"], 0.001)
    return _tree_cache[(name, builder)]


def _device_rows(woop, tri_index, tri, pos):
    """The Woop buffer with every triangle's rows replaced by the device builders' rows (np_hlbvh.woop_rows), found from triIndex and
    the terminators alone: a row group starts where the previous one ended."""
    w = woop.view(np.uint32).reshape(-1, 4).copy()
    rows12 = np_hlbvh.woop_rows(np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)).view(np.uint32)
    r = 0
    while r < w.shape[0]:
        if w[r, 0] == rf.TERM:
            r += 1
            continue
        w[r:r + 3] = rows12[tri_index[r]].reshape(3, 4)
        r += 3
    return w.reshape(-1).view(np.uint8)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_unmoved_vertices_give_the_tree_back(name, builder):
    tri, pos, _ = _scene(name)
    nodes, woop, idx, eps = _tree(name, builder)
    out = rf.refit(nodes, woop, idx, tri, pos, eps)
    before = nodes.view(np.int32).reshape(-1, 16)
    assert np.array_equal(out["nodes"][:, 12:], before[:, 12:]), "link words changed"
    assert np.array_equal(out["nodes"].view(F)[:, :12], before.view(F)[:, :12]), "box words differ as floats"
    # measured: they are byte-equal too (the builders fold min / max in an order that ends on the same signed zeros)
    assert np.array_equal(out["nodes"], before), "box words differ in their bytes"
    if builder == "lbvh":
        assert np.array_equal(out["woop"], woop), "Woop rows changed"
    else:   # the host's woopify is not woop_rows.h: the rows become the device rows
        assert np.array_equal(out["woop"], _device_rows(woop, idx, tri, pos))
    n_inner = before.shape[0]
    assert out["stats"] == dict(numNodes=n_inner, numLeaves=n_inner + 1, numRows=woop.nbytes // 16)
    mn, mx = oracle.scene_bbox(pos)
    assert np.array_equal(out["scene_box"], np.concatenate([mn - F(eps), mx + F(eps)]).astype(F))


def _check_boxes(out_nodes, woop_u8, idx, tri, pos, eps):
    """Every leaf box and every inner box of every reached node, by plain float minimum / maximum (the coordinates compared with ==)."""
    ni = out_nodes
    nf = ni.view(F)
    w = woop_u8.view(np.uint32).reshape(-1, 4)
    levels = rf.levels_of(ni)
    reached = np.concatenate(levels)
    checked = 0
    for k in (0, 1):
        c = ni[reached, 12 + k].astype(np.int64)
        par, ch = reached[c > 0], c[c > 0] // 64
        got = nf[par][:, rf.BOX_WORDS[k]]
        a, b = nf[ch][:, rf.BOX_WORDS[0]], nf[ch][:, rf.BOX_WORDS[1]]
        assert np.array_equal(got[:, rf.LO], np.minimum(a[:, rf.LO], b[:, rf.LO]))
        assert np.array_equal(got[:, rf.HI], np.maximum(a[:, rf.HI], b[:, rf.HI]))
        checked += par.size
    leaf_node, leaf_k, of_leaf, rows = rf.leaf_rows(ni, w, levels)
    order = np.argsort(of_leaf, kind="stable")
    of_leaf, rows = of_leaf[order], rows[order]
    starts = np.flatnonzero(np.concatenate([[True], of_leaf[1:] != of_leaf[:-1]]))
    v = pos[tri[idx[rows]]]                                            # [m, 3, 3]
    lo = np.minimum.reduceat(v.min(axis=1), starts, axis=0)
    hi = np.maximum.reduceat(v.max(axis=1), starts, axis=0)
    leaves = of_leaf[starts]
    for k in (0, 1):
        sel = leaf_k[leaves] == k
        got = nf[leaf_node[leaves][sel]][:, rf.BOX_WORDS[k]]
        assert np.array_equal(got[:, rf.LO], (lo[sel] - F(eps)).astype(F))
        assert np.array_equal(got[:, rf.HI], (hi[sel] + F(eps)).astype(F))
        checked += int(sel.sum())
    assert checked == 2 * reached.size - (leaf_node.size - leaves.size)   # every child slot but the empty leaves'
    return leaf_node.size - leaves.size


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_deformed_boxes_hold_the_moved_triangles_and_trace_equals_brute_force(name, builder):
    tri, pos, cam = _scene(name)
    nodes, woop, idx, eps = _tree(name, builder)
    rays = np.concatenate([scenes.primary_rays(cam, 48, 48)[0], scenes.random_rays(256, 5, extent=float(np.abs(pos).max()))])
    for how in DEFORMATIONS:
        p = rf.moved(pos, how)
        out = rf.refit(nodes, woop, idx, tri, p, eps)
        assert np.array_equal(out["nodes"][:, 12:], nodes.view(np.int32).reshape(-1, 16)[:, 12:])
        assert _check_boxes(out["nodes"], out["woop"], idx, tri, p, eps) == 0
        ref, _ = oracle.trace(out["nodes"].view(np.uint8).reshape(-1), out["woop"], idx, rays, threads=8)
        bf = oracle.bruteforce_closest(out["woop"], idx, rays)
        assert np.array_equal(ref["t"].view(np.uint32), bf["t"].view(np.uint32)), (name, builder, how)
        if how != "collapse":
            assert (ref["id"] >= 0).any()


def _assert_topology_untouched(before_nodes, before_woop, out, reached):
    b = before_nodes.view(np.int32).reshape(-1, 16)
    assert np.array_equal(out["nodes"][:, 12:], b[:, 12:])
    unreached = np.setdiff1d(np.arange(b.shape[0]), reached)
    assert np.array_equal(out["nodes"][unreached], b[unreached])
    w0, w1 = before_woop.view(np.uint32).reshape(-1, 4), out["woop"].view(np.uint32).reshape(-1, 4)
    levels = rf.levels_of(b)
    _, _, _, rows = rf.leaf_rows(b, w0, levels)
    written = np.zeros(w0.shape[0], bool)
    for j in range(3):
        written[rows + j] = True
    assert np.array_equal(w0[~written], w1[~written]), "a row outside the leaves' row groups changed"
    return unreached


def test_appended_zero_slot_is_returned_untouched():
    tri, pos, _ = scenes.random_soup(700, seed=5)
    b = oracle.lbvh_build(tri, pos, 8, 0.001)
    nodes = np.concatenate([b["nodes"], np.zeros(64, np.uint8)])
    p = rf.deform(pos, 0.02)
    out = rf.refit(nodes, b["woop"], b["tri_index"], tri, p, 0.001)
    plain = rf.refit(b["nodes"], b["woop"], b["tri_index"], tri, p, 0.001)
    assert not out["nodes"][-1].any()
    assert np.array_equal(out["nodes"][:-1], plain["nodes"]) and np.array_equal(out["woop"], plain["woop"])
    assert np.array_equal(out["scene_box"], plain["scene_box"]) and out["stats"] == plain["stats"]
    unreached = _assert_topology_untouched(nodes, b["woop"], out, np.concatenate(rf.levels_of(out["nodes"])))
    assert list(unreached) == [nodes.size // 64 - 1]


def test_known_answer_tree_with_its_oversize_leaf():
    import kat_lbvh as kl
    tri, pos = kl.scene()
    b = oracle.lbvh_build(tri, pos, kl.LEAF_SIZE, kl.EPSILON)
    same = rf.refit(b["nodes"], b["woop"], b["tri_index"], tri, pos, kl.EPSILON)
    assert np.array_equal(same["nodes"].view(np.uint8).reshape(-1), b["nodes"]) and np.array_equal(same["woop"], b["woop"])
    assert kl.compare(same["nodes"].view(np.uint8).reshape(-1), same["woop"], b["tri_index"], "refit") == (kl.NUM_INNER, kl.NUM_LEAVES)
    p = rf.deform(pos, 0.02)
    out = rf.refit(b["nodes"], b["woop"], b["tri_index"], tri, p, kl.EPSILON)
    reached = np.concatenate(rf.levels_of(out["nodes"]))
    _assert_topology_untouched(b["nodes"], b["woop"], out, reached)
    assert _check_boxes(out["nodes"], out["woop"], b["tri_index"], tri, p, kl.EPSILON) == 0
    sizes = np.bincount(rf.leaf_rows(out["nodes"], out["woop"].view(np.uint32).reshape(-1, 4), rf.levels_of(out["nodes"]))[2])
    assert sizes.max() > kl.LEAF_SIZE   # the level-0 node's leaves hold more than leafSize triangles


def test_empty_leaf_of_a_one_triangle_tree_keeps_its_box():
    pos = np.array([[1, 2, 3], [1.25, 2, 3], [1, 2.25, 3]], F)
    tri = np.array([[0, 1, 2]], np.int32)
    b = oracle.lbvh_build(tri, pos, 8, 0.001)
    ni = b["nodes"].view(np.int32).reshape(-1, 16)
    assert ni.shape[0] == 1 and ni[0, 12] < 0 and ni[0, 13] < 0
    p = rf.deform(pos, 0.3)
    out = rf.refit(b["nodes"], b["woop"], b["tri_index"], tri, p, 0.001)
    assert _check_boxes(out["nodes"], out["woop"], b["tri_index"], tri, p, 0.001) == 1       # one empty leaf
    w = b["woop"].view(np.uint32).reshape(-1, 4)
    empty = 0 if w[~ni[0, 12], 0] == rf.TERM else 1
    assert np.array_equal(out["nodes"][0, rf.BOX_WORDS[empty]], ni[0, rf.BOX_WORDS[empty]])
    full = out["nodes"].view(F)[0, rf.BOX_WORDS[empty ^ 1]]
    assert np.array_equal(out["scene_box"], np.concatenate([full[rf.LO], full[rf.HI]]))
    assert out["stats"] == dict(numNodes=1, numLeaves=2, numRows=5)


# ---- C-ABI surface ------------------------------------------------------------------------------------------------------

def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_refit_entry_points_are_exported_and_bound():
    L = nt.lib()
    assert hasattr(L, "ntr_bvh_refit") and hasattr(L, "ntr_bvh_refit_scratch_bytes")
    assert C.sizeof(nt.BvhRefitResult) == 20
    assert L.ntr_bvh_refit_scratch_bytes(None) == -1
    v = C.c_int64(-1)
    assert L.ntr_bvh_refit_scratch_bytes(C.byref(v)) == 0 and v.value == 0


def test_refit_argument_checks_precede_device_work():
    """Every check answers NTR_ERR_INVALID with a message naming the argument; the pointers are never dereferenced (they are not
    device pointers), so this runs with or without a device."""
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    good = dict(d_nodes=p, nodes_bytes=128, d_woop=p, woop_bytes=160, d_idx=p, idx_bytes=40, num_tris=3, d_tri=p, num_verts=9, d_pos=p,
                epsilon=0.0)
    cases = [(dict(d_nodes=0), "d_nodes"), (dict(nodes_bytes=0), "nodesBytes"), (dict(nodes_bytes=100), "nodesBytes"),
             (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"), (dict(d_woop=0), "d_triWoop"), (dict(woop_bytes=24), "triWoopBytes"),
             (dict(woop_bytes=0), "triWoopBytes"), (dict(d_idx=0), "d_triIndex"), (dict(idx_bytes=36), "triIndexBytes"),
             (dict(num_tris=0), "numTris"), (dict(d_tri=0), "d_triVtxIndex"), (dict(num_verts=0), "numVerts"), (dict(d_pos=0), "d_vtxPos"),
             (dict(epsilon=-1e-3), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(epsilon=float("inf")), "epsilon")]
    for change, word in cases:
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.bvh_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    if not _has_device():   # valid arguments and no device: no CPU fallback
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_refit(**good)
        assert e.value.code in (-2, -3)
        assert not buf.any()
