"""The in-place refit of 4-wide trees without a device: the numpy rule (tests/np_wide_refit.py) is tied to the rules it stands on.  Every
box of a refitted wide tree is, word for word, the box of the refitted binary tree at the slot's source (np_bvh_wide.expand names it),
for the pool's BLASes and for the top level; the refit of a fresh widening with unmoved vertices or unchanged instances returns every
buffer unchanged; padding slots copy slot 0; the smallest trees behave as the rule says; the two-level wide trace over refitted buffers
hits triangles where they are now; and the two entry points refuse every argument error before any device work."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import instanced_scenes as isc
import np_bvh_optimize as opt
import np_bvh_refit as rf
import np_bvh_wide as bw
import np_instanced as ni
import np_instanced_wide as niw
import np_ploc_batch as pb
import np_refit_batch as rb
import np_tlas_refit as tr
import np_tracer
import np_wide_refit as wr

F = np.float32
HOWS = (0.02, 0.3, "collapse")
WBOX = wr.WBOX
_cache = {}


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _woop_equal(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a.view(F)) & np.isnan(b.view(F)))).all())


def _tree(kind, n):
    """(nodes uint8, woop uint8, tri_index int32, tri, pos) of a PLOC tree (one triangle per leaf) or an LBVH tree (leafSize 8)."""
    if (kind, n) not in _cache:
        tri, pos = scenes.random_soup(n, seed=100 + n, walls=False)[:2]
        tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
        if kind == "ploc":
            b = pb.build(pb.concat([(tri, pos)])[2], tri, pos)
        else:
            b = oracle.lbvh_build(tri, pos, 8, 0.001)
        _cache[(kind, n)] = (np.ascontiguousarray(b["nodes"]).view(np.uint8).reshape(-1), np.ascontiguousarray(b["woop"]).view(np.uint8).reshape(-1),
                             np.ascontiguousarray(b["tri_index"], np.int32), tri, pos)
    return _cache[(kind, n)]


def _sources(nodes, kept):
    """Per wide node, np_bvh_wide.expand's entry list [(link, source slot, source child)] over the binary tree `nodes`."""
    ni_ = bw._as_nodes(nodes)
    nf = ni_.view(F)
    areas = np.stack([opt.area(nf[:, bw.BOX[0]]), opt.area(nf[:, bw.BOX[1]])], axis=1)
    return [bw.expand(ni_, areas, int(b)) for b in kept]


def _assert_boxes_at_sources(wide_after, binary_after, sources, what):
    wf = np.ascontiguousarray(wide_after).reshape(-1).view(F).reshape(-1, 32)
    wi = wf.view(np.int32)
    bf = np.ascontiguousarray(binary_after).reshape(-1).view(F).reshape(-1, 16)
    for w, E in enumerate(sources):
        assert wi[w, bw.WCOUNT] == len(E)
        for k, (_, s, ck) in enumerate(E):
            assert wf[w, WBOX[k]].tobytes() == bf[s, bw.BOX[ck]].tobytes(), (what, w, k)
        for k in range(len(E), 4):                                                       # rule 6
            assert wi[w, bw.WLINK + k] == 0 and wf[w, WBOX[k]].tobytes() == wf[w, WBOX[0]].tobytes(), (what, w, k)


# ---- 1. the refitted wide tree is the refitted binary tree at its sources ---------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("ploc", 1), ("ploc", 2), ("ploc", 3), ("ploc", 5), ("ploc", 40), ("ploc", 300), ("lbvh", 9), ("lbvh", 400)])
def test_wide_boxes_equal_the_refitted_binary_tree_at_their_sources(kind, n):
    nodes, woop, idx, tri, pos = _tree(kind, n)
    W = bw.widen(nodes)
    sources = _sources(nodes, W["kept"])
    for how in HOWS:
        p = rf.moved(pos, how)
        for eps in (0.0, 0.001):
            T = rf.refit(nodes, woop, idx, tri, p, eps)
            for rewrite in (True, False):
                out = wr.refit_wide_blas(W["nodes"], woop, idx, tri, p, eps, rewrite)
                what = (kind, n, how, eps, rewrite)
                assert out["err_bits"] == 0
                _assert_boxes_at_sources(out["nodes"], T["nodes"], sources, what)
                assert out["root_box"].tobytes() == T["scene_box"].tobytes(), what
                # rule 1: links and the count row; rule 2: the rows are the binary refit's, or untouched
                assert np.array_equal(out["nodes"][:, 12:16], W["nodes"][:, 12:16]) and np.array_equal(out["nodes"][:, 28:], W["nodes"][:, 28:])
                assert _woop_equal(out["woop"], T["woop"]) if rewrite else np.array_equal(out["woop"], woop), what
                assert out["stats"] == dict(numNodes=W["stats"]["numNodes"], numLeafLinks=W["stats"]["numLeafLinks"],
                                            numRows=T["stats"]["numRows"]), what


# ---- 2. a fresh widening is a fixed point ---------------------------------------------------------------------------------------------
def _ploc_pool():
    if "pool" not in _cache:
        sizes = (1, 2, 3, 4, 5, 40, 1, 300)
        tri, pos, meshes = pb.concat([scenes.random_soup(n, seed=31 + 7 * k + n, walls=False)[:2] for k, n in enumerate(sizes)])
        b = pb.build(meshes, tri, pos)
        _cache["pool"] = (tri, pos, meshes, b, niw.widen_pool(b))
    return _cache["pool"]


def _wide_entries(pool, wpool, meshes, eps=0.0):
    return [(w[0], w[1], r[2], r[3], m[0], m[1], eps) for w, r, m in zip(wpool["ranges"], pool["ranges"], meshes)]


def test_refit_of_a_fresh_widening_with_unmoved_vertices_changes_nothing():
    tri, pos, meshes, b, wp = _ploc_pool()
    entries = _wide_entries(b, wp, meshes)
    out = wr.refit_wide_pool(entries, wp["nodes"], b["woop"], b["tri_index"], tri, pos, True)
    assert np.array_equal(out["nodes"], wp["nodes"]) and _woop_equal(out["woop"], b["woop"]) and out["err_bits"] == 0
    assert out["first_bad_entry"] == -1
    assert out["stats"] == dict(numNodes=wp["stats"]["numNodes"], numLeafLinks=wp["stats"]["numLeafLinks"], numRows=b["woop"].size // 16)
    same = rb.refit([(r, m[0], m[1], 0.0) for r, m in zip(b["ranges"], meshes)], b["nodes"], b["woop"], b["tri_index"], tri, pos)
    assert out["boxes"].tobytes() == same["boxes"].tobytes()
    # a subset in another order touches nothing else, and moved vertices change exactly the listed ranges
    moved = rf.moved(pos, 0.3)
    sub = [entries[7], entries[0], entries[5]]
    part = wr.refit_wide_pool(sub, wp["nodes"], b["woop"], b["tri_index"], tri, moved, True)
    mask_n, mask_w = np.zeros(wp["nodes"].size, bool), np.zeros(b["woop"].size, bool)
    for no, nb, wo, wb, _, _, _ in sub:
        mask_n[no:no + nb] = True
        mask_w[wo:wo + wb] = True
    assert np.array_equal(part["nodes"][~mask_n], wp["nodes"][~mask_n]) and np.array_equal(part["woop"][~mask_w], b["woop"].view(np.uint8)[~mask_w])
    assert not np.array_equal(part["nodes"][mask_n], wp["nodes"][mask_n]) and part["boxes"].shape == (3, 6)


def _scene(name):
    """np_instanced_wide's scene over PLOC BLASes with one shared index and vertex array: the refits' input."""
    if ("scene", name) not in _cache:
        sc = isc.scene(name)
        pool = isc.pool_of(sc["names"])
        tri, pos, meshes = pb.concat([isc.blas(nm)[:2] for nm in sc["names"]])
        inst = ni.instances(sc["transforms"], sc["blas"])
        t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
        wpool = niw.widen_pool(pool)
        wt = niw.widen_tlas(t["nodes"], t["root_link"], inst, pool["ranges"], wpool["ranges"])
        _cache[("scene", name)] = (sc, pool, tri, pos, meshes, inst, t, wpool, wt)
    return _cache[("scene", name)]


@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_refit_of_a_fresh_wide_tlas_with_unchanged_instances_changes_nothing(name):
    sc, pool, tri, pos, meshes, inst, t, wpool, wt = _scene(name)
    out = wr.refit_wide_tlas(wt["nodes"], wt["root_link"], wt["records"], wpool["nodes"], pool["ranges"], wpool["ranges"], inst)
    assert np.array_equal(out["nodes"], wt["nodes"]) and np.array_equal(out["records"], wt["records"]) and out["err_bits"] == 0
    same = tr.refit(t["nodes"], t["root_link"], t["records"], pool["nodes"], pool["ranges"], inst)
    assert out["scene_box"].tobytes() == same["scene_box"].tobytes()
    assert out["stats"] == dict(numNodes=wt["stats"]["numNodes"], numLeaves=inst.shape[0])


# ---- 3. the top level at its sources: moved instances over a refitted pool ----------------------------------------------------------
def _refitted_scene(name, how=0.05, which=0):
    """BLAS `which` deformed (binary and wide pool refitted, rows rewritten) and every instance moved -> the buffers after both refits"""
    sc, pool, tri, pos, meshes, inst, t, wpool, wt = _scene(name)
    p = pos.copy()
    m = meshes[which]
    verts = np.unique(tri[m[0]:m[0] + m[1]])
    p[verts] = rf.moved(pos[verts], how)
    entries = _wide_entries(pool, wpool, meshes)
    sel = [entries[which]]
    wide = wr.refit_wide_pool(sel, wpool["nodes"], pool["woop"], pool["tri_index"], tri, p, True)
    binary = rb.refit([(pool["ranges"][which], m[0], m[1], 0.0)], pool["nodes"], pool["woop"], pool["tri_index"], tri, p)
    assert _woop_equal(wide["woop"], binary["woop"]) and wide["boxes"].tobytes() == binary["boxes"].tobytes()
    # every instance moved a little, so that the scene stays in front of the camera
    moved_tf = inst["objectToWorld"].copy()
    moved_tf[:, 3] += np.linspace(-0.5, 0.5, inst.shape[0]).astype(F)
    moved_tf[:, 7] += F(0.25)
    new = ni.instances(moved_tf, inst["blas"])
    wtl = wr.refit_wide_tlas(wt["nodes"], wt["root_link"], wt["records"], wide["nodes"], pool["ranges"], wpool["ranges"], new)
    btl = tr.refit(t["nodes"], t["root_link"], t["records"], binary["nodes"], pool["ranges"], new)
    return dict(p=p, wide=wide, binary=binary, inst=new, wtl=wtl, btl=btl)


@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_wide_tlas_boxes_equal_the_refitted_binary_tlas_at_their_sources(name):
    sc, pool, tri, pos, meshes, inst, t, wpool, wt = _scene(name)
    r = _refitted_scene(name)
    W = bw.widen(t["nodes"])
    assert np.array_equal(W["nodes"], wt["nodes"])
    _assert_boxes_at_sources(r["wtl"]["nodes"], r["btl"]["nodes"], _sources(t["nodes"], W["kept"]), name)
    assert r["wtl"]["scene_box"].tobytes() == r["btl"]["scene_box"].tobytes() and r["wtl"]["err_bits"] == 0
    assert np.array_equal(r["wtl"]["nodes"][:, 12:16], wt["nodes"][:, 12:16]) and np.array_equal(r["wtl"]["nodes"][:, 28:], wt["nodes"][:, 28:])
    fresh = niw.widen_tlas(t["nodes"], t["root_link"], r["inst"], pool["ranges"], wpool["ranges"])
    assert np.array_equal(r["wtl"]["records"], fresh["records"])
    # an instance that switched its BLAS: the record and the leaf box follow it
    if len(pool["ranges"]) > 1:
        sw = r["inst"].copy()
        sw["blas"][0] = (sw["blas"][0] + 1) % len(pool["ranges"])
        a = wr.refit_wide_tlas(wt["nodes"], wt["root_link"], wt["records"], r["wide"]["nodes"], pool["ranges"], wpool["ranges"], sw)
        b = tr.refit(t["nodes"], t["root_link"], t["records"], r["binary"]["nodes"], pool["ranges"], sw)
        _assert_boxes_at_sources(a["nodes"], b["nodes"], _sources(t["nodes"], W["kept"]), (name, "switched"))
        assert a["records"][0, 12] == wpool["ranges"][sw["blas"][0]][0] and a["records"][0, 14] == wpool["ranges"][sw["blas"][0]][1]


# ---- 4. small trees ----------------------------------------------------------------------------------------------------------------------
def test_one_triangle_blas_keeps_its_empty_leaf_and_two_triangles_fill_two_slots():
    nodes, woop, idx, tri, pos = _tree("ploc", 1)
    W = bw.widen(nodes)
    wi = W["nodes"]
    assert wi.shape[0] == 1 and wi[0, bw.WCOUNT] == 2 and (wi[0, 12:14] < 0).all()
    w32 = woop.view(np.uint32).reshape(-1, 4)
    empty = 0 if w32[~wi[0, 12], 0] == rf.TERM else 1
    p = rf.moved(pos, "collapse")
    out = wr.refit_wide_blas(wi, woop, idx, tri, p, 0.0)
    assert np.array_equal(out["nodes"][0, WBOX[empty]], wi[0, WBOX[empty]])              # the empty leaf keeps its box words
    point = np.array([0.25, 0.25, -1.5, -1.5, 3.0, 3.0], F)
    assert out["nodes"].view(F)[0, WBOX[1 - empty]].tobytes() == point.tobytes()
    for k in (2, 3):
        assert out["nodes"][0, WBOX[k]].tobytes() == out["nodes"][0, WBOX[0]].tobytes() and out["nodes"][0, 12 + k] == 0
    assert out["stats"] == dict(numNodes=1, numLeafLinks=2, numRows=5)
    nodes, woop, idx, tri, pos = _tree("ploc", 2)
    W = bw.widen(nodes)
    out = wr.refit_wide_blas(W["nodes"], woop, idx, tri, rf.moved(pos, 0.3), 0.0)
    assert W["nodes"].shape[0] == 1 and out["stats"] == dict(numNodes=1, numLeafLinks=2, numRows=8)
    v = rf.moved(pos, 0.3)[tri].reshape(-1, 3)
    assert np.array_equal(out["root_box"], np.concatenate([v.min(axis=0), v.max(axis=0)]))


def test_one_instance_has_no_node_and_only_record_0_is_written():
    sc, pool, tri, pos, meshes, inst, t, wpool, wt = _scene("three")
    one = inst[1:2].copy()
    records = np.full((3, 16), 0xABABABAB, np.uint32)
    out = wr.refit_wide_tlas(np.zeros((0, 32), np.int32), ~0, records[:1], wpool["nodes"], pool["ranges"], wpool["ranges"], one)
    same = tr.refit(np.zeros((0, 16), np.int32), ~0, records[:1], pool["nodes"], pool["ranges"], one)
    assert out["nodes"].shape == (0, 32) and out["records"].shape == (1, 16) and out["stats"] == dict(numNodes=0, numLeaves=1)
    assert out["scene_box"].tobytes() == same["scene_box"].tobytes()
    assert np.array_equal(out["records"], niw.widen_tlas(None, ~0, one, pool["ranges"], wpool["ranges"])["records"])
    # a blas index out of range: bit 1, the empty extent, no scene box
    one["blas"] = 7
    out = wr.refit_wide_tlas(np.zeros((0, 32), np.int32), ~0, records[:1], wpool["nodes"], pool["ranges"], wpool["ranges"], one)
    assert out["err_bits"] == 1 and not out["records"][0, 12:].any() and not out["scene_box"].any()


def test_a_malformed_tree_is_never_followed_and_keeps_its_topology():
    nodes, woop, idx, tri, pos = _tree("ploc", 40)
    W = bw.widen(nodes)["nodes"]
    p = rf.moved(pos, 0.3)
    good = wr.refit_wide_blas(W, woop, idx, tri, p, 0.0)
    inner = np.argwhere(W[:, 12:16] > 0)
    n, k = (int(x) for x in inner[len(inner) // 2])
    for value in (0x7FFFFF80, W[n, 12 + k] + 64, 128 * W.shape[0], int(W[inner[0][0], 12 + inner[0][1]])):   # outside, misaligned, the extent, named twice
        if value == W[n, 12 + k]:
            continue
        bad = W.copy()
        bad[n, 12 + k] = value
        out = wr.refit_wide_blas(bad, woop, idx, tri, p, 0.0)
        assert out["err_bits"] == 1 and not out["root_box"].any(), hex(value)
        assert np.array_equal(out["nodes"][:, 12:16], bad[:, 12:16]) and np.array_equal(out["nodes"][:, 28:], bad[:, 28:])
    bad = W.copy()
    bad[n, bw.WCOUNT] = 5
    assert wr.refit_wide_blas(bad, woop, idx, tri, p, 0.0)["err_bits"] == 1
    # rows, triangle and vertex indices
    leaf = np.argwhere(W[:, 12:16] < 0)[3]
    row = ~int(W[leaf[0], 12 + leaf[1]])
    t2 = idx.copy()
    t2[row] = 40
    assert wr.refit_wide_blas(W, woop, t2, tri, p, 0.0)["err_bits"] == 4
    tri2 = tri.copy()
    tri2[idx[row], 1] = p.shape[0]
    assert wr.refit_wide_blas(W, woop, idx, tri2, p, 0.0)["err_bits"] == 8
    cut = woop[:16 * (row + 2)]
    out = wr.refit_wide_blas(W, cut, idx[:row + 2], tri, p, 0.0)
    assert out["err_bits"] & 2
    # in a batch every other entry is refitted completely and the lowest bad entry is named
    tri_, pos_, meshes, b, wp = _ploc_pool()
    entries = _wide_entries(b, wp, meshes)
    nodes2 = wp["nodes"].copy()
    first_inner = np.argwhere(nodes2.view(np.int32).reshape(-1, 32)[entries[7][0] // 128:, 12:16] > 0)[0]
    nodes2.view(np.int32).reshape(-1, 32)[entries[7][0] // 128 + first_inner[0], 12 + first_inner[1]] = 0x7FFFFF80
    moved = rf.moved(pos_, 0.3)
    ok = wr.refit_wide_pool(entries, wp["nodes"], b["woop"], b["tri_index"], tri_, moved)
    out = wr.refit_wide_pool(entries, nodes2, b["woop"], b["tri_index"], tri_, moved)
    assert out["first_bad_entry"] == 7 and out["err_bits"] == 1
    lo, wo = entries[7][0], entries[7][2]                   # the last entry: everything before it belongs to the others
    assert np.array_equal(out["nodes"][:lo], ok["nodes"][:lo]) and _woop_equal(out["woop"][:wo], ok["woop"][:wo])
    assert out["boxes"][:7].tobytes() == ok["boxes"][:7].tobytes()
    assert good["err_bits"] == 0


# ---- 5. the trace over refitted buffers -----------------------------------------------------------------------------------------------
def _triangle_rows(woop_u32):
    """first row of every triangle of a BLAS's rows, found from the terminators alone"""
    rows, r = [], 0
    while r < woop_u32.shape[0]:
        if woop_u32[r, 0] == rf.TERM:
            r += 1
        else:
            rows.append(r)
            r += 3
    return np.array(rows, np.int64)


def test_trace_over_refitted_wide_buffers_hits_the_moved_triangles():
    name = "three"
    sc, pool, tri, pos, meshes, inst, t, wpool, wt = _scene(name)
    r = _refitted_scene(name, how=0.05, which=1)
    rays = isc.scene_rays(primary=(24, 12), random=128)
    spool = dict(nodes=r["binary"]["nodes"], woop=r["wide"]["woop"], tri_index=pool["tri_index"], ranges=pool["ranges"])
    w32 = r["wide"]["woop"].view(np.uint32).reshape(-1, 4)
    wf = w32.view(F)
    hits = 0
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst, _ = niw.trace(r["wtl"]["nodes"], wt["root_link"], r["wtl"]["records"], spool, r["wide"]["nodes"], rays, any_hit)
        for q in np.flatnonzero(rid >= 0):
            i = int(rinst[q])
            b = int(r["inst"]["blas"][i])
            first, num = meshes[b][0], meshes[b][1]
            assert 0 <= rid[q] < num
            wo, wb = pool["ranges"][b][2] // 16, pool["ranges"][b][3] // 16
            rows = _triangle_rows(w32[wo:wo + wb]) + wo
            a = rows[pool["tri_index"][rows] == rid[q]]
            assert a.size >= 1
            a = int(a[0])
            # the rows are woop_rows.h of the triangle at its new position
            exp = wr.np_hlbvh.woop_rows(tri[first + rid[q]][None, :], r["p"]).view(np.uint32).reshape(3, 4)
            assert _woop_equal(w32[a:a + 3], exp)
            # np_tracer's Woop test of that triangle with the new rows, for the ray in the instance's object space
            m = r["wtl"]["records"].view(F)[i, :12]
            one = np.ones(1, F)
            o = ni.xform(m, rays["ox"][q:q + 1], rays["oy"][q:q + 1], rays["oz"][q:q + 1], 1)
            d = ni.xform(m, rays["dx"][q:q + 1], rays["dy"][q:q + 1], rays["dz"][q:q + 1], 0)
            z = wf[a:a + 1]
            with np.errstate(all="ignore"):
                Oz = z[:, 3] - o[0] * z[:, 0] - o[1] * z[:, 1] - o[2] * z[:, 2]
                tt = Oz * (F(1) / np_tracer._dot4(z, d[0], d[1], d[2], np.zeros(1, F)))
            assert tt.astype(F).tobytes() == rt[q:q + 1].tobytes(), (any_hit, q)
            assert one.size and rays["tmin"][q] < rt[q] <= rays["tmax"][q]
            hits += 1
    assert hits > 50


# ---- 6. the entry points' argument checks ---------------------------------------------------------------------------------------------
def test_symbols_structures_and_the_scratch_queries():
    L = nt.lib()
    for name in ("ntr_pool_wide_refit", "ntr_pool_wide_refit_scratch_bytes", "ntr_tlas_wide_refit", "ntr_tlas_wide_refit_scratch_bytes"):
        assert hasattr(L, name)
    assert C.sizeof(nt.WideRefitEntry) == 48 and C.sizeof(nt.WideRefitResult) == 48
    for name in ("ntr_pool_wide_refit_scratch_bytes", "ntr_tlas_wide_refit_scratch_bytes"):
        assert getattr(L, name)(None) == -1 and name.encode() in L.ntr_last_error()
    if not _has_device():
        assert nt.pool_wide_refit_scratch_bytes() == 0 and nt.tlas_wide_refit_scratch_bytes() == 0
    e = nt.WideRefitEntry(128, 256, 16, 32, 3, 5, 0.5)
    assert (e.wideNodesOffset, e.wideNodesBytes, e.triWoopOffset, e.triWoopBytes, e.firstTri, e.numTris, e.epsilon, e.pad) == (128, 256, 16, 32, 3, 5, 0.5, 0)


def test_pool_wide_refit_argument_errors_are_decided_before_device_work():
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data
    # three wide BLASes of 2, 1 and 1 nodes over meshes of 5, 1 and 3 triangles as ntr_ploc_build_batch lays the rows out
    _, _, _, ranges = pb.capacity([5, 1, 3])
    wide = [(0, 256), (256, 128), (384, 128)]
    entries = [(w[0], w[1], r[2], r[3], f, n, 0.0) for w, r, f, n in zip(wide, ranges, (0, 5, 6), (5, 1, 3))]
    woop_bytes = ranges[-1][2] + ranges[-1][3]
    good = dict(entries=entries, d_wide_pool_nodes=fake, wide_pool_nodes_bytes=512, d_pool_woop=fake, pool_woop_bytes=woop_bytes, d_pool_idx=fake,
                num_tris_total=9, d_tri=fake, num_verts=20, d_pos=fake)

    def entry(k, **change):
        out = [list(x) for x in entries]
        for key, v in change.items():
            out[k][dict(no=0, nb=1, wo=2, wb=3, first=4, n=5, eps=6)[key]] = v
        return [tuple(x) for x in out]

    cases = [dict(entries=[]), dict(d_wide_pool_nodes=0), dict(d_pool_woop=0), dict(d_pool_idx=0), dict(d_tri=0), dict(d_pos=0),
             dict(num_tris_total=0), dict(num_verts=0), dict(rewrite_rows=2), dict(rewrite_rows=-1),
             dict(wide_pool_nodes_bytes=0), dict(wide_pool_nodes_bytes=512 + 64), dict(wide_pool_nodes_bytes=0xFFFFFF00 + 128),
             dict(pool_woop_bytes=0), dict(pool_woop_bytes=woop_bytes + 4), dict(pool_woop_bytes=0xFFFFFF00 + 16),
             dict(d_wide_pool_nodes=fake + 4), dict(d_pool_woop=fake + 8),
             dict(entries=entry(1, no=256 + 64)), dict(entries=entry(1, nb=192)), dict(entries=entry(0, nb=0)), dict(entries=entry(0, no=-128)),
             dict(entries=entry(2, nb=256)), dict(entries=entry(2, no=512)),
             dict(entries=entry(0, nb=0x76543200 + 128), wide_pool_nodes_bytes=0xFFFFFF00),
             dict(entries=entry(1, wo=ranges[1][2] + 8)), dict(entries=entry(1, wb=0)), dict(entries=entry(1, wb=24)), dict(entries=entry(0, wo=-16)),
             dict(entries=entry(2, wb=ranges[2][3] + 16)), dict(entries=entry(2, wo=woop_bytes)),
             dict(entries=entry(1, n=0)), dict(entries=entry(0, first=-1)), dict(entries=entry(2, first=7)), dict(num_tris_total=8),
             dict(entries=entry(1, eps=-1e-3)), dict(entries=entry(2, eps=float("nan"))), dict(entries=entry(0, eps=float("inf"))),
             dict(entries=entries + [entries[1]]), dict(entries=entry(1, no=128)), dict(entries=entry(1, wo=ranges[2][2] + 16))]
    for change in cases:
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.pool_wide_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and "ntr_pool_wide_refit" in str(e.value), (change, str(e.value))
    for change in (dict(entries=entries + [entries[1]]), dict(entries=entry(1, wo=ranges[2][2] + 16))):
        with pytest.raises(nt.NtrError) as e:
            nt.pool_wide_refit(**dict(good, **change))
        assert "overlap" in str(e.value), str(e.value)
    L = nt.lib()
    arr = (nt.WideRefitEntry * 3)(*[nt.WideRefitEntry(*x) for x in entries])
    res = nt.WideRefitResult()
    tail = (fake, 512, fake, woop_bytes, fake, 9, fake, 20, fake, 1, None)
    for count, a in ((3, None), ((1 << 20) + 1, arr), (0, arr), (-1, arr)):
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        assert L.ntr_pool_wide_refit(count, C.cast(a, C.c_void_p), *tail, C.byref(res), None) == -1
        assert bytes(res) == bytes(C.sizeof(res)) and b"ntr_pool_wide_refit" in L.ntr_last_error()
        assert L.ntr_pool_wide_refit(count, C.cast(a, C.c_void_p), *tail, None, None) == -1
    if not _has_device():   # valid arguments and no device: no CPU fallback, after the argument checks
        for blocking in (True, False):
            for rewrite in (True, False):
                with pytest.raises(nt.NtrError) as e:
                    nt.pool_wide_refit(**good, rewrite_rows=rewrite, blocking=blocking)
                assert e.value.code in (-2, -3)
    assert not buf.any()


def test_tlas_wide_refit_argument_errors_are_decided_before_device_work():
    fake, fake2 = 0x10000, 0x4000000
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    wide = [(0, 1280, 10, 5), (1280, 128, 1, 1)]
    good = dict(num_instances=5, d_instances=fake, ranges=ranges, wide_ranges=wide, d_wide_pool_nodes=fake, wide_pool_nodes_bytes=1408,
                d_wide_tlas_nodes=fake2, wide_tlas_nodes_bytes=256, root_link=0, d_wide_records=fake2 + 4096, records_cap=320)
    bad_wide = [[(64, 1280, 10, 5), wide[1]], [(0, 1000, 10, 5), wide[1]], [(0, 0, 0, 0), wide[1]], [wide[0], (1408, 128, 1, 1)],
                [(-128, 1280, 10, 5), wide[1]], [wide[0], (1280, 256, 1, 1)]]
    cases = [dict(num_instances=0), dict(d_instances=0), dict(d_instances=fake + 4), dict(ranges=[], wide_ranges=[]), dict(d_wide_pool_nodes=0),
             dict(d_wide_pool_nodes=fake + 8), dict(wide_pool_nodes_bytes=0), dict(wide_pool_nodes_bytes=1400), dict(wide_pool_nodes_bytes=0xFFFFFF80),
             dict(d_wide_tlas_nodes=0), dict(wide_tlas_nodes_bytes=0), dict(wide_tlas_nodes_bytes=200), dict(wide_tlas_nodes_bytes=0x76543280),
             dict(root_link=128), dict(root_link=~0), dict(root_link=~3), dict(d_wide_records=0), dict(d_wide_records=fake2 + 8), dict(records_cap=319),
             dict(num_instances=1), dict(num_instances=1, root_link=~0), dict(num_instances=1, root_link=0, wide_tlas_nodes_bytes=0),
             dict(ranges=[(0, 640, 8, 1600), ranges[1]]), dict(ranges=[(0, 640, -16, 1600), ranges[1]])] + [dict(wide_ranges=w) for w in bad_wide]
    for change in cases:
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_wide_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and "ntr_tlas_wide_refit" in str(e.value), (change, str(e.value))
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in ranges])
    warr = (nt.WideBlasRange * 2)(*[nt.WideBlasRange(*w) for w in wide])
    res = nt.TlasRefitResult()
    for a, w in ((None, warr), (arr, None)):
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        rc = L.ntr_tlas_wide_refit(5, fake, 2, C.cast(a, C.c_void_p), C.cast(w, C.c_void_p), fake, 1408, fake2, 256, 0, fake2 + 4096, 320, None,
                                   C.byref(res), None)
        assert rc == -1 and bytes(res) == bytes(C.sizeof(res))
    if not _has_device():
        for call in (lambda b: nt.tlas_wide_refit(**good, blocking=b),
                     lambda b: nt.tlas_wide_refit(**dict(good, num_instances=1, root_link=~0, d_wide_tlas_nodes=0, wide_tlas_nodes_bytes=0,
                                                         records_cap=64), blocking=b)):
            for blocking in (True, False):
                with pytest.raises(nt.NtrError) as e:
                    call(blocking)
                assert e.value.code in (-2, -3), str(e.value)
