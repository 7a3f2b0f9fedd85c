"""The rule of deformation motion blur (tests/np_bvh_motion.py) on the CPU, and the C-ABI surface of ntr_bvh_motion_refit and
ntr_trace_bvh_motion without a device: motion_refit's pieces are the two keys' np_bvh_refit.refit and the vertex rows the rule states,
with the terminator in w; the posed box contains the posed triangle and the posed parent its children, exactly, at seeded times; at
the shutter's ends the trace equals np_tracer's over either key's refitted tree, inside it np_tracer's over the posed static tree and
brute force over the posed rows on every ray; a trace that ignores the time would fail; the entry points check their arguments before
any device work.  Trees are the oracle's LBVH; every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from oracle import oracle

import bvh_motion_cases as mc
import np_bvh_motion as bm
import np_bvh_refit as rf
import np_tracer

F = np.float32
_trees = {}


def _tree(name):
    if name not in _trees:
        tri, pos = mc.scene(name)
        b = oracle.lbvh_build(tri, pos, 8, 0.001)
        _trees[name] = (b["nodes"], b["woop"], b["tri_index"])
    return _trees[name]


def _spec(name, how, eps):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name)
    return mc.spec_of((name, "oracle-lbvh"), nodes, woop, idx, tri, pos, how, eps)


def _leaves(ni):
    """(node, k, first row) of every leaf child of a reached slot."""
    out = []
    for lv in rf.levels_of(ni):
        for s in lv:
            for k in (0, 1):
                if ni[s, 12 + k] < 0:
                    out.append((int(s), k, int(~ni[s, 12 + k])))
    return out


def _expected_vertex_rows(nodes, woop, idx, tri, pos):
    """The vertex rows by a walk of its own: leaf by leaf, row group by row group, up to the Woop terminator."""
    ni = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)
    w = np.ascontiguousarray(woop).view(np.uint32).reshape(-1, 4)
    out = np.zeros_like(w)
    for _, _, r in _leaves(ni):
        while w[r, 0] != rf.TERM:
            for j in range(3):
                out[r + j, :3] = pos[tri[idx[r], j]].view(np.uint32)
            r += 3
        out[r] = (0, 0, 0, rf.TERM)
    return out


# ---- 1. the refit's pieces ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_motion_refit_is_the_two_refits_and_the_vertex_rows(name):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name)
    for how in mc.DEFORMATIONS:
        for eps in mc.EPSILONS:
            m, pos1 = _spec(name, how, eps)
            r0, r1 = rf.refit(nodes, woop, idx, tri, pos, eps), rf.refit(nodes, woop, idx, tri, pos1, eps)
            assert np.array_equal(m["nodes0"], r0["nodes"]) and np.array_equal(m["woop"], r0["woop"]) and m["stats"] == r0["stats"]
            assert np.array_equal(m["nodes1"], r1["nodes"])
            assert np.array_equal(m["nodes1"][:, 12:], nodes.view(np.int32).reshape(-1, 16)[:, 12:])          # the links are the input's
            assert np.array_equal(m["vrows0"], _expected_vertex_rows(nodes, woop, idx, tri, pos))
            assert np.array_equal(m["vrows1"], _expected_vertex_rows(nodes, woop, idx, tri, pos1))
            assert m["vrows0"].shape == (woop.nbytes // 16, 4)
            # a terminator of the Woop rows that a leaf reaches is a terminator of the vertex rows, in w, and nowhere else is w set
            assert np.array_equal(m["vrows0"][:, 3] != 0, m["vrows1"][:, 3] != 0)
            assert set(np.unique(m["vrows0"][:, 3])) <= {0, rf.TERM}
            b0, b1 = r0["scene_box"], r1["scene_box"]
            assert np.array_equal(m["scene_box"][:3], np.minimum(b0[:3], b1[:3])) and np.array_equal(m["scene_box"][3:], np.maximum(b0[3:], b1[3:]))


def test_a_negative_zero_vertex_x_does_not_end_the_leaf():
    tri, pos = mc.scene("one")
    pos = pos.copy()
    pos[tri[0, 0]] = (-0.0, 2.0, 3.0)
    b = oracle.lbvh_build(tri, pos, 8, 0.001)
    pos1 = rf.deform(pos, 0.02)
    pos1[tri[0, 0], 0] = -0.0
    m = bm.motion_refit(b["nodes"], b["woop"], b["tri_index"], tri, pos, pos1, 0.001)
    ni = m["nodes0"]
    leaf = [r for (_, _, r) in _leaves(ni) if m["vrows0"][r, 3] != rf.TERM]
    assert len(leaf) == 1 and m["vrows0"][leaf[0], 0] == rf.TERM and m["vrows0"][leaf[0], 3] == 0     # x IS the terminator's word
    rays = np.zeros(2, nt.RAY_DTYPE)
    c = pos[tri[0]].astype(np.float64).mean(axis=0)
    rays[0] = (c[0], c[1], c[2] - 1, 0, 0, 0, 1, 10)
    rays[1] = (c[0], c[1], c[2] + 1, 0, 0, 0, -1, 10)
    for time in (0.0, 0.5, 1.0):
        ids, t, u, v, st = mc.spec_trace(m, b["tri_index"], rays, time=time, stats=True)
        assert (ids == 0).all() and st["numTriTests"] == 2, time


# ---- 2. containment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_posed_boxes_contain_posed_triangles_and_children_exactly(name):
    rng = np.random.default_rng(17)
    for how, eps in ((0.02, 0.0), (0.3, 0.001), ("collapse", 0.0), (0.0, 0.0)):
        m, _ = _spec(name, how, eps)
        ni = m["nodes0"]
        f0, f1 = m["nodes0"].view(F), m["nodes1"].view(F)
        v0, v1 = m["vrows0"].view(F), m["vrows1"].view(F)
        leaves = _leaves(ni)
        inner = [(int(s), k, int(ni[s, 12 + k]) // 64) for lv in rf.levels_of(ni) for s in lv for k in (0, 1) if ni[s, 12 + k] > 0]
        for t in rng.random(16).astype(F):
            box = bm.deform_lerp(f0[:, :12], f1[:, :12], t)
            verts = bm.deform_lerp(v0[:, :3], v1[:, :3], t)
            for s, k, r in leaves:
                b = box[s, rf.BOX_WORDS[k]]
                while m["vrows0"][r, 3] != rf.TERM:
                    tv = verts[r:r + 3]
                    assert (b[rf.LO] <= tv).all() and (tv <= b[rf.HI]).all(), (how, eps, float(t), s, k, r)
                    r += 3
            for s, k, c in inner:
                b = box[s, rf.BOX_WORDS[k]]
                for ck in (0, 1):
                    cb = box[c, rf.BOX_WORDS[ck]]
                    assert (b[rf.LO] <= cb[rf.LO]).all() and (cb[rf.HI] <= b[rf.HI]).all(), (how, eps, float(t), s, k, c)


# ---- 3. the ends -------------------------------------------------------------------------------------------------------------------
def _static(nodes, woop, idx, rays, any_hit=False):
    return np_tracer.trace(nodes, woop, idx, rays, any_hit=any_hit)


@pytest.mark.parametrize("name", mc.SCENES)
def test_ends_equal_the_static_trace_over_either_key(name):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name)
    rays = np.concatenate([mc.rays_of(name, "box")[:1024], mc.rays_of(name, "edge")])
    m, pos1 = _spec(name, 0.02, 0.001)
    key1 = rf.refit(nodes, woop, idx, tri, pos1, 0.001)
    per_key = []
    for time, (kn, kw) in ((0.0, (m["nodes0"], m["woop"])), (1.0, (key1["nodes"], key1["woop"]))):
        for any_hit in (False, True):
            ref = _static(kn, kw, idx, rays, any_hit)
            got = mc.spec_trace(m, idx, rays, any_hit, time=time)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (time, any_hit)
            if not any_hit:
                per_key.append(got)
    # per-ray times of exactly 0 and 1 mixed in one batch, and the values that clamp to them
    times = np.tile(np.array([0.0, 1.0, np.nan, 2.0, -1.0, -0.0, np.inf, -np.inf], F), rays.shape[0] // 8 + 1)[:rays.shape[0]]
    which = np.tile(np.array([0, 1, 0, 1, 0, 0, 1, 0]), rays.shape[0] // 8 + 1)[:rays.shape[0]]
    got = mc.spec_trace(m, idx, rays, times=times, time=0.37)   # the scalar is not read when times are given
    for k in range(4):
        ref = np.where(which == 0, per_key[0][k].view(np.uint32), per_key[1][k].view(np.uint32))
        assert np.array_equal(got[k].view(np.uint32), ref), k


# ---- 4. inside the shutter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_inside_the_shutter_equals_the_posed_static_tree_and_brute_force(name):
    """No ray is left out: brute force over the posed rows gives the spec's t on every one of the 4 096 rays."""
    tri, pos = mc.scene(name)
    _, _, idx = _tree(name)
    rays = mc.rays_of(name, "box")
    for how, eps, times in ((0.02, 0.0, mc.TIMES), (0.3, 0.001, mc.TIMES), (0.02, 0.001, (0.37,)), (0.3, 0.0, (0.37,))):
        m, pos1 = _spec(name, how, eps)
        for time in times:
            pn, pw = bm.posed_static_tree(m, idx, tri, pos, pos1, time)
            got = mc.spec_trace(m, idx, rays, time=time)
            ref = _static(pn, pw, idx, rays)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (how, eps, time)
            bf = oracle.bruteforce_closest(pw, idx, rays)
            assert np.array_equal(got[1].view(np.uint32), bf["t"].view(np.uint32)), (how, eps, time)
            print("%s %s %s t=%s: %d hits of %d" % (name, how, eps, time, int((got[0] >= 0).sum()), rays.shape[0]))


# ---- 5. sensitivity ----------------------------------------------------------------------------------------------------------------
def test_the_middle_of_the_shutter_differs_from_both_keys():
    _, _, idx = _tree("soup1500")
    rays = mc.rays_of("soup1500", "box")
    m, _ = _spec("soup1500", 0.02, 0.001)
    mid, k0, k1 = (mc.spec_trace(m, idx, rays, time=t) for t in (0.5, 0.0, 1.0))
    d0 = (mid[0] != k0[0]) | (mid[1].view(np.uint32) != k0[1].view(np.uint32))
    d1 = (mid[0] != k1[0]) | (mid[1].view(np.uint32) != k1[1].view(np.uint32))
    print("records at t = 0.5 that differ from key 0: %d, from key 1: %d, from both: %d of %d" % (d0.sum(), d1.sum(), (d0 & d1).sum(), rays.shape[0]))
    assert (d0 & d1).any()


def test_deform_lerp_has_no_same_word_shortcut_and_keeps_the_ends():
    rng = np.random.default_rng(23)
    a = rng.uniform(-10, 10, 1 << 16).astype(F)
    t = rng.random(1 << 16).astype(F)
    out = bm.deform_lerp(a, a, t)
    assert (out != a).any() and np.abs(out - a).max() <= np.spacing(np.abs(a)).max() * 2       # a static word may wobble, by an ulp or so
    b = rng.uniform(-10, 10, 1 << 16).astype(F)
    assert np.array_equal(bm.deform_lerp(a, b, F(0)).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(bm.deform_lerp(a, b, F(1)).view(np.uint32), b.view(np.uint32))
    assert bm.deform_lerp(F(-0.0), F(5), F(0)).view(np.uint32) == 0x80000000
    lo0, lo1 = np.minimum(a, b), np.minimum(a, b) - F(0.5)
    assert (bm.deform_lerp(lo0, lo1, t) <= bm.deform_lerp(a, b, t)).all()


# ---- 6. C-ABI surface --------------------------------------------------------------------------------------------------------------
def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_entry_points_are_exported_and_bound():
    L = nt.lib()
    for s in ("ntr_bvh_motion_refit", "ntr_bvh_motion_refit_scratch_bytes", "ntr_trace_bvh_motion", "ntr_trace_bvh_motion_stats"):
        assert hasattr(L, s)
    assert C.sizeof(nt.BvhMotion) == 40
    assert L.ntr_bvh_motion_refit_scratch_bytes(None) == -1
    v = C.c_int64(-1)
    assert L.ntr_bvh_motion_refit_scratch_bytes(C.byref(v)) == 0 and v.value == 0


def _refit_args(buf):
    p = buf.ctypes.data
    p += (-p) % 256
    return dict(d_nodes0=p, nodes_bytes=128, d_nodes1=p + 256, d_woop=p + 512, woop_bytes=160, d_idx=p + 768, idx_bytes=40,
                d_vert_rows0=p + 1024, d_vert_rows1=p + 1280, num_tris=3, d_tri=p + 1536, num_verts=9, d_pos0=p + 1792, d_pos1=p + 2048,
                epsilon=0.0, d_scene_box=p + 2304)


def test_motion_refit_argument_checks_precede_device_work():
    buf = np.zeros(8192, np.uint8)
    good = _refit_args(buf)
    p = good["d_nodes0"]
    cases = [(dict(d_nodes0=0), "d_nodes0"), (dict(nodes_bytes=0), "nodesBytes"), (dict(nodes_bytes=100), "nodesBytes"),
             (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"), (dict(d_woop=0), "d_triWoop"), (dict(woop_bytes=24), "triWoopBytes"),
             (dict(woop_bytes=0), "triWoopBytes"), (dict(d_idx=0), "d_triIndex"), (dict(idx_bytes=36), "triIndexBytes"),
             (dict(num_tris=0), "numTris"), (dict(d_tri=0), "d_triVtxIndex"), (dict(num_verts=0), "numVerts"), (dict(d_pos0=0), "d_vtxPos0"),
             (dict(epsilon=-1e-3), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(epsilon=float("inf")), "epsilon"),
             # the four new buffers: null, or overlapping another buffer of the call
             (dict(d_nodes1=0), "d_nodes1"), (dict(d_vert_rows0=0), "d_vertRows0"), (dict(d_vert_rows1=0), "d_vertRows1"),
             (dict(d_pos1=0), "d_vtxPos1"),
             (dict(d_nodes1=p), "overlaps"), (dict(d_nodes1=p + 64), "overlaps"), (dict(d_nodes1=good["d_woop"] - 64), "overlaps"),
             (dict(d_vert_rows0=good["d_woop"]), "overlaps"), (dict(d_vert_rows1=good["d_vert_rows0"] + 144), "overlaps"),
             (dict(d_vert_rows1=good["d_idx"] + 32), "overlaps"), (dict(d_vert_rows0=good["d_tri"] + 16), "overlaps"),
             (dict(d_pos1=good["d_pos0"] + 104), "overlaps"), (dict(d_pos1=good["d_scene_box"] + 20), "overlaps"),
             (dict(d_pos1=good["d_nodes1"] + 124), "overlaps")]
    for change, word in cases:
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.bvh_motion_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    if not _has_device():   # valid arguments and no device: no CPU fallback
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_motion_refit(**good)
        assert e.value.code in (-2, -3)
        assert not buf.any()


def test_motion_trace_argument_checks_precede_device_work():
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    p += (-p) % 16

    def call(fn=nt.trace_bvh_motion, num_rays=8, d_rays=p, d_results=p, d_nodes0=p, nodes_bytes=128, vert_rows_bytes=160, d_idx=p, motion="good",
             d_nodes1=p, d_v0=p, d_v1=p, d_times=0, **kw):
        mo = nt.BvhMotion(d_nodes1, d_v0, d_v1, d_times, 0.5) if motion == "good" else motion
        return fn(num_rays, False, d_rays, d_results, d_nodes0, nodes_bytes, vert_rows_bytes, d_idx, mo, **kw)

    cases = [(dict(num_rays=-1), "numRays"), (dict(d_rays=0), "null ray or result"), (dict(d_results=0), "null ray or result"),
             (dict(d_nodes0=0), "null BVH buffer"), (dict(d_idx=0), "null BVH buffer"), (dict(d_nodes1=0), "null BVH buffer"),
             (dict(d_v0=0), "null BVH buffer"), (dict(d_v1=0), "null BVH buffer"), (dict(motion=None), "null motion"),
             (dict(nodes_bytes=0), "nodesBytes"), (dict(nodes_bytes=100), "nodesBytes"), (dict(nodes_bytes=0x76543200 + 64), "nodesBytes"),
             (dict(vert_rows_bytes=0), "vertRowsBytes"), (dict(vert_rows_bytes=24), "vertRowsBytes"),
             (dict(vert_rows_bytes=0xFFFFFF00 + 16), "vertRowsBytes"), (dict(d_times=p + 2), "4-byte aligned")]
    for fn in (nt.trace_bvh_motion, nt.trace_bvh_motion_stats):
        for change, word in cases:
            with pytest.raises(nt.NtrError) as e:
                call(fn, **change)
            assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    assert call(num_rays=0) == 0.0                                       # NTR_OK with 0 seconds, whatever else is passed
    assert call(num_rays=0, d_rays=0, motion=None, timed=False) is None
    assert call(nt.trace_bvh_motion_stats, num_rays=0).numRays == 0
    if not _has_device():
        for fn in (nt.trace_bvh_motion, nt.trace_bvh_motion_stats):
            with pytest.raises(nt.NtrError) as e:
                call(fn)
            assert e.value.code in (-2, -3)
        assert not buf.any()
