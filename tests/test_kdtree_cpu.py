"""The kd-tree path without a device: the spatial-median build byte for byte against the restatement (tests/np_kdtree.py),
Woop rows shared with the BVH, invariants of the SAH build, the checks of ntr_host_kdtree_wrap, and the argument checks of
ntr_trace_kdtree that precede any device work."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import _capi, scenes

import np_kdtree

EMPTY = -2147483648


def coplanar_grid(n=24):
    """An n x n grid of unit quads in the plane z = 0 (every triangle flat on one axis, every split plane on their edges)."""
    xs = np.arange(n + 1, dtype=np.float32)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    pos = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32)], axis=1).astype(np.float32)
    tris = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            tris += [(a, b, c), (a, c, d)]
    return np.array(tris, dtype=np.int32), pos


def degenerate_and_axis_aligned():
    """Axis-aligned triangles, slivers, triangles collapsed to a line or a point, and duplicates."""
    rng = np.random.default_rng(5)
    v = []
    for k in range(60):
        c = rng.integers(-8, 8, size=3).astype(np.float32)
        a = k % 3
        p = np.array([c, c, c], dtype=np.float32)
        p[1, (a + 1) % 3] += 2.0
        p[2, (a + 2) % 3] += 2.0
        v.append(p)                                             # axis-aligned
        v.append(np.array([c, c + 1.0, c + 2.0], np.float32))  # collapsed to a line
        v.append(np.array([c, c, c], np.float32))              # collapsed to a point
        v.append(p.copy())                                      # duplicate
    pos = np.concatenate(v).astype(np.float32)
    return np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3), pos


def _scene(name):
    if name == "cornell":
        tri, pos, _ = scenes.cornell_box()
    elif name == "soup1500":
        tri, pos, _ = scenes.random_soup(1500, seed=11)
    elif name == "soup_nowalls":
        tri, pos, _ = scenes.random_soup(3000, seed=12, walls=False)
    elif name == "grid":
        tri, pos = coplanar_grid()
    elif name == "degenerate":
        tri, pos = degenerate_and_axis_aligned()
    elif name == "root_leaf":
        tri, pos, _ = scenes.random_soup(1, seed=2, walls=False)
    else:
        raise KeyError(name)
    return tri, pos


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("scene", ["cornell", "soup1500", "grid", "degenerate", "root_leaf"])
def test_spatial_median_bytes(scene, max_leaf):
    tri, pos = _scene(scene)
    kd = nt.kdtree_build(tri, pos, "SpatialMedianKDTree", max_leaf)
    ref = np_kdtree.spatial_median(tri, pos, max_leaf)
    assert np.array_equal(kd.nodes, ref["nodes"])
    assert np.array_equal(kd.tri_index, ref["tri_index"])
    assert _same_bits(kd.scene_min, ref["scene_min"]) and _same_bits(kd.scene_max, ref["scene_max"])
    assert _same_bits(np.float32(kd.delta), ref["delta"])
    for k, v in ref["stats"].items():
        assert kd.info[k] == v, (k, kd.info[k], v)
    assert kd.woop.nbytes == (tri.shape[0] * 48 + 4095) // 4096 * 4096


def test_root_leaf_layout():
    tri, pos = _scene("root_leaf")
    for builder in ("SpatialMedianKDTree", "SAHKDTree"):
        kd = nt.kdtree_build(tri, pos, builder)
        assert kd.nodes.shape == (1, 4)
        assert kd.nodes[0, 0] == ~0 and kd.nodes[0, 1] == EMPTY and kd.nodes[0, 3] == 0
        assert _same_bits(kd.nodes[0, 2:3].view(np.float32), kd.scene_max[:1])
        assert list(kd.tri_index) == [0, EMPTY]
        assert kd.info["maxDepth"] == 1 and kd.info["numInnerNodes"] == 1 and kd.info["numLeafNodes"] == 2


@pytest.mark.parametrize("builder", ["SpatialMedianKDTree", "SAHKDTree"])
def test_woop_rows_equal_the_bvh_rows(builder):
    tri, pos = _scene("soup1500")
    kd = nt.kdtree_build(tri, pos, builder)
    bvh = nt.sah_build(tri, pos)
    bw = bvh.woop.view(np.uint32).reshape(-1, 4)
    kw = kd.woop.view(np.uint32).reshape(-1, 4)
    idx = bvh.tri_index
    # a Compact BVH's triIndex runs parallel to its Woop rows: a triangle's first row carries its id; leaves end in a 0x80000000 row
    seen = set()
    r = 0
    while r < bw.shape[0]:
        if bw[r, 0] == 0x80000000:
            r += 1
            continue
        t = int(idx[r])
        assert np.array_equal(bw[r:r + 3], kw[3 * t:3 * t + 3]), t
        seen.add(t)
        r += 3
    assert seen == set(range(tri.shape[0]))
    assert not kw[3 * tri.shape[0]:].any()


def _sah_limit(n):
    return int(np.float32(1.2) * np.float32(np.float32(np.log(np.float32(n))) / np.float32(np.log(np.float32(2.0)))) + np.float32(2.0))


@pytest.mark.parametrize("scene", ["soup1500", "soup_nowalls", "grid", "degenerate", "atrium"])
def test_sah_invariants(scene):
    if scene == "atrium":
        tri, pos, _ = scenes.atrium()
    else:
        tri, pos = _scene(scene)
    a = nt.kdtree_build(tri, pos, "SAHKDTree")
    b = nt.kdtree_build(tri, pos, "SAHKDTree")
    for f in ("nodes", "woop", "tri_index", "scene_min", "scene_max"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    n = tri.shape[0]
    assert a.info["maxDepth"] <= max(_sah_limit(n), 1)
    st = np_kdtree.kdtree_stats(a.nodes, a.tri_index)
    for k, v in st.items():
        assert a.info[k] == v, (k, a.info[k], v)
    # indices in range, lists terminated, every node reached once (kdtree_wrap performs the same walk)
    w = nt.host_kdtree_wrap(a.nodes, a.woop, a.tri_index, a.scene_min, a.scene_max)
    assert w.info["numInnerNodes"] == a.nodes.shape[0]
    assert set(np.unique(a.tri_index[a.tri_index != EMPTY]).tolist()) <= set(range(n))
    if scene != "atrium":   # the SAT walk is quadratic in the worst case; atrium is covered by the GPU agreement test
        assert np_kdtree.coverage_violations(a.nodes, a.tri_index, a.scene_min, a.scene_max, tri, pos) == []


def test_spatial_median_coverage():
    tri, pos = _scene("soup1500")
    kd = nt.kdtree_build(tri, pos, "SpatialMedianKDTree")
    assert np_kdtree.coverage_violations(kd.nodes, kd.tri_index, kd.scene_min, kd.scene_max, tri, pos) == []


def _wrap(nodes, tri_index, woop_tris=4, smin=(0, 0, 0), smax=(1, 1, 1)):
    woop = np.zeros(woop_tris * 12, dtype=np.float32)
    return nt.host_kdtree_wrap(np.asarray(nodes, dtype=np.int32), woop, np.asarray(tri_index, dtype=np.int32), smin, smax)


def test_wrap_accepts_a_built_tree_and_rejects_bad_ones():
    tri, pos = _scene("soup1500")
    kd = nt.kdtree_build(tri, pos, "SAHKDTree")
    w = nt.host_kdtree_wrap(kd.nodes, kd.woop, kd.tri_index, kd.scene_min, kd.scene_max)
    assert np.array_equal(w.nodes, kd.nodes) and np.array_equal(w.tri_index, kd.tri_index) and np.array_equal(w.woop, kd.woop)
    assert _same_bits(np.float32(w.delta), np.float32(kd.delta))
    ok = [[~0, EMPTY, 0, 0]]
    _wrap(ok, [1, EMPTY])
    bad = {
        "child out of range": ([[1, EMPTY, 0, 0]], [0, EMPTY]),
        "missing terminator": ([[~0, EMPTY, 0, 0]], [0, 1]),
        "list offset out of range": ([[~5, EMPTY, 0, 0]], [0, EMPTY]),
        "triangle id out of range": ([[~0, EMPTY, 0, 0]], [4, EMPTY]),
        "cycle": ([[1, EMPTY, 0, 0], [0, EMPTY, 0, 0]], [0, EMPTY]),
        "self loop": ([[0, EMPTY, 0, 0]], [0, EMPTY]),
        "axis 3": ([[~0, EMPTY, 0, 3 << 28]], [0, EMPTY]),
    }
    for what, (nodes, idx) in bad.items():
        with pytest.raises(nt.NtrError) as e:
            _wrap(nodes, idx)
        assert e.value.code == -4, what
    # a chain of 64 inner nodes is accepted, 65 is beyond the kernel's stack
    for depth, ok_ in ((64, True), (65, False)):
        chain = [[i + 1, EMPTY, 0, 0] for i in range(depth - 1)] + [[~0, EMPTY, 0, 0]]
        if ok_:
            assert _wrap(chain, [0, EMPTY]).info["maxDepth"] == 64
        else:
            with pytest.raises(nt.NtrError) as e:
                _wrap(chain, [0, EMPTY])
            assert e.value.code == -4
    with pytest.raises(nt.NtrError) as e:   # sizes
        nt.host_kdtree_wrap(np.zeros(0, np.int32), np.zeros(12, np.float32), np.array([EMPTY], np.int32), (0, 0, 0), (1, 1, 1))
    assert e.value.code == -1


def test_build_arguments():
    tri, pos = _scene("soup1500")
    with pytest.raises(nt.NtrError) as e:
        nt.kdtree_build(tri[:0], pos, "SAHKDTree")
    assert e.value.code == -1
    with pytest.raises(nt.NtrError):
        nt.kdtree_build(tri, pos, "NoSuchKDTree")
    with pytest.raises(nt.NtrError):
        nt.kdtree_build(tri, pos, "SpatialMedianKDTree", 0)
    bad = tri.copy()
    bad[3, 1] = pos.shape[0]
    with pytest.raises(nt.NtrError):
        nt.kdtree_build(bad, pos, "SAHKDTree")


def test_trace_argument_checks_precede_device_work():
    lib = nt.lib()
    f3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    g3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    p = C.c_void_p(0x1000)
    sec = C.c_float(-1.0)

    def call(n, smin=f3, smax=g3, rays=p, res=p, nodes=p, nb=16, woop=p, wb=48, idx=p, ib=8):
        return lib.ntr_trace_kdtree(n, 0, smin, smax, rays, res, nodes, nb, woop, wb, idx, ib, None, C.byref(sec))

    assert call(0) == 0 and sec.value == 0.0                       # the empty batch: nothing to do
    assert call(0, nodes=None) == 0
    assert call(-1) == -1
    assert call(4, nodes=None) == -1 and b"No kd-tree" in lib.ntr_last_error()
    assert call(4, woop=None) == -1
    assert call(4, idx=None) == -1
    assert call(4, rays=None) == -1
    assert call(4, res=None) == -1
    assert call(4, smin=None) == -1
    assert call(4, nb=8) == -1
    assert call(4, nb=24) == -1
    assert call(4, wb=32) == -1
    assert call(4, wb=50) == -1
    assert call(4, ib=6) == -1
    assert call(4, ib=0) == -1
    assert "ntr_trace_kdtree" in {s[0] for s in _capi.SYMBOLS}
