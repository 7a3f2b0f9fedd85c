"""The device kd-tree build's spec on its own (tests/np_kdtree_binned.py), no GPU: a known-answer scene, the termination thresholds,
flat and degenerate scenes, coverage, acceptance by ntr_host_kdtree_wrap, traces equal to brute force, and the C-ABI's parameter
checks, which fail before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import np_kdtree
import np_kdtree_binned as kb

F = np.float32
EMPTY = -2147483648


def _bits(x):
    return int(np.array([x], F).view(np.int32)[0])


def _tri_at(x, y, z, s=0.25):
    return [(x, y, z), (x + s, y, z), (x, y + s, z)]


def _scene(corners):
    pos = np.array([v for c in corners for v in _tri_at(*c)], F)
    tri = np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3)
    return tri, pos


def _known_answer_scene():
    # 20 triangles of side 0.25 in the plane z = 0: ids 0..9 at x = 0, y = 0..9; ids 10..19 at x = 8, y = 0..9.  A 21st point
    # pins the z extent: the last triangle of each column is lifted to z = 0..1 by its third vertex.
    corners = [(0.0, float(i), 0.0) for i in range(10)] + [(8.0, float(i), 0.0) for i in range(10)]
    tri, pos = _scene(corners)
    pos[3 * 9 + 2, 2] = 1.0
    pos[3 * 19 + 2, 2] = 1.0
    return tri, pos


def test_known_answer_root_split():
    # Scene box: x [0, 8.25], y [0, 9.25], z [0, 1]; root area A = 2 * (8.25 * 9.25 + 9.25 * 1 + 1 * 8.25) = 187.625.  The root has
    # 20 > 16 references and splits.
    # x planes k = 0..10 at 8.25 * (k+1)/12 all lie between the columns (0.6875 .. 7.5625): nL = nR = 10, and areaL + areaR =
    #   2 * (8.25 * 9.25 + 2 * 9.25 * 1 + 8.25 * 1) = 206.125 whatever the position, so s = 2061.25.
    # y plane k = 16 (axis 1, the 6th) at 0 + 9.25 * (6/12 = 0.5) = 4.625 lies between rows 4 (y 4..4.25) and 5: nL = nR = 10 and
    #   areaL = areaR = 2 * (8.25 * 4.625 + 4.625 * 1 + 1 * 8.25) = 102.0625, so s = 2041.25 < 2061.25.  The other y planes cut
    #   unevenly (one side holds more rows, or a row straddles), and z planes keep 18 or 20 references on a side: all dearer.
    # ratio = (1 + 2041.25 / 187.625) / 20 = 0.594 <= 0.9: no failure.  Both children hold 10 <= 16 references: leaves.
    tri, pos = _known_answer_scene()
    lv = []
    r = kb.build(tri, pos, trace_levels=lv)
    assert r["scene_min"].tolist() == [0.0, 0.0, 0.0] and r["scene_max"].tolist() == [8.25, 9.25, 1.0]
    root = lv[0]
    assert not root["leaf"][0] and root["plane"][0] == 16
    assert root["split"][0] == F(4.625)
    assert r["nodes"][0, 2] == _bits(4.625) and r["nodes"][0, 3] == 1 << 28
    assert (root["nl"][0], root["nr"][0]) == (10, 10)
    # both children have 10 <= 16 references: leaves, listed in level order with ascending ids
    assert r["nodes"].shape == (1, 4)
    assert r["nodes"][0, 0] == ~0 and r["nodes"][0, 1] == ~11
    assert r["tri_index"].tolist() == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14, EMPTY, 5, 6, 7, 8, 9, 15, 16, 17, 18, 19, EMPTY]
    st = r["stats"]
    assert (st["numInnerNodes"], st["numLeafNodes"], st["numEmptyLeaves"], st["numTriRefs"], st["maxDepth"]) == (1, 2, 0, 20, 1)
    # recompute the plane costs independently (the reference's expressions, binary32 per operation)
    lo, hi = r["scene_min"], r["scene_max"]
    d = hi - lo
    costs = []
    v = pos[tri]
    for k in range(32):
        a = min(k // 11, 2)
        p = F(lo[a] + (hi[a] - lo[a]) * (F(1 + k % 11) / F(12)))
        nl = int(np.sum((p - v[:, :, a].min(axis=1)) > -F(1e-8)))
        nr = int(np.sum((p - v[:, :, a].max(axis=1)) < F(1e-8)))
        dl, dr = d.copy(), d.copy()
        dl[a], dr[a] = p - lo[a], hi[a] - p
        ar = lambda e: F((F(e[0] * e[1]) + F(e[1] * e[2]) + F(e[2] * e[0])) * F(2))  # noqa: E731
        costs.append(F(ar(dl) * F(nl) + ar(dr) * F(nr)))
    assert costs[16] == F(2041.25) and all(c == F(2061.25) for c in costs[:11])
    assert int(np.argmin(costs)) == 16 and sorted(costs)[1] > costs[16]


def test_threshold_16_and_17():
    corners = [(float(i % 5) * 2, float(i // 5) * 2, 0.0) for i in range(17)]
    tri, pos = _scene(corners)
    r16 = kb.build(tri[:16], pos)
    # 16 <= triLimit: the root-leaf tree
    assert r16["nodes"].tolist() == [[~0, EMPTY, _bits(r16["scene_max"][0]), 0]]
    assert r16["tri_index"].tolist() == list(range(16)) + [EMPTY]
    r17 = kb.build(tri, pos)
    # 17 > triLimit: a real split, both children hold references (not the root-leaf form with its empty child 1)
    assert r17["stats"]["numInnerNodes"] >= 1 and r17["nodes"][0, 1] != EMPTY
    assert sorted(set(r17["tri_index"].tolist()) - {EMPTY}) == list(range(17))


def test_failrq_stop_on_stacked_triangles():
    # 40 identical triangles: every plane either straddles all of them or leaves one side empty of area -> ratio > 0.9
    tri, pos = _scene([(0.0, 0.0, 0.0)] * 40)
    lv = []
    r = kb.build(tri, pos, trace_levels=lv)
    assert lv[0]["leaf"][0]
    assert r["nodes"].tolist() == [[~0, EMPTY, _bits(r["scene_max"][0]), 0]]
    assert r["tri_index"].tolist() == list(range(40)) + [EMPTY]
    # with failureCount 1 the first failure does not stop the root
    r1 = kb.build(tri, pos, dict(failureCount=1), trace_levels=[])
    assert r1["stats"]["numInnerNodes"] >= 1


def test_depth_cap():
    tri, pos, _ = scenes.random_soup(600, seed=5)
    for k2 in (-5.0, 2.0):
        r = kb.build(tri, pos, dict(depthK1=0.0, depthK2=k2))
        md = kb.max_depth(tri.shape[0], 0.0, k2)
        assert r["stats"]["maxDepth"] <= max(md, 1)
    r = kb.build(tri, pos, dict(depthK1=0.0, depthK2=4.0))
    assert r["stats"]["maxDepth"] == 4


def test_flat_and_degenerate():
    rng = np.random.default_rng(3)
    pos = rng.uniform(-5, 5, (300, 3)).astype(F)
    pos[:, 2] = 0
    tri = np.arange(300, dtype=np.int32).reshape(-1, 3)
    r = kb.build(tri, pos)
    assert r["scene_min"][2] == 0 and r["scene_max"][2] == 0
    assert not np_kdtree.coverage_violations(r["nodes"], r["tri_index"], r["scene_min"], r["scene_max"], tri, pos)
    # degenerate triangles: points and segments among ordinary ones; a line-shaped scene (zero area cells)
    tri2, pos2, _ = scenes.random_soup(200, seed=9)
    pos2 = pos2.copy()
    pos2[tri2[:20, 1]] = pos2[tri2[:20, 0]]
    pos2[tri2[:10, 2]] = pos2[tri2[:10, 0]]
    r2 = kb.build(tri2, pos2)
    assert sorted(set(r2["tri_index"].tolist()) - {EMPTY}) == list(range(tri2.shape[0]))
    line = np.zeros((60, 3), F)
    line[:, 0] = np.arange(60, dtype=F)
    r3 = kb.build(np.arange(60, dtype=np.int32).reshape(-1, 3) % 60, line)
    assert sorted(set(r3["tri_index"].tolist()) - {EMPTY}) == list(range(20))


def test_no_finite_cost_is_a_leaf():
    tri, pos = _scene([(float(i) * 1e19, float(i % 3) * 1e19, float(i % 5) * 1e19) for i in range(30)])
    lv = []
    r = kb.build(tri, pos, trace_levels=lv)
    assert lv[0]["leaf"][0]
    assert r["nodes"].shape == (1, 4) and r["nodes"][0, 1] == EMPTY


@pytest.mark.parametrize("scene", ["cornell", "soup1500"])
def test_coverage_wrap_and_brute_force(scene):
    tri, pos, cam = scenes.cornell_box() if scene == "cornell" else scenes.random_soup(1500, seed=11)
    r = kb.build(tri, pos)
    assert not np_kdtree.coverage_violations(r["nodes"], r["tri_index"], r["scene_min"], r["scene_max"], tri, pos)
    h = nt.host_kdtree_wrap(r["nodes"], r["woop"], r["tri_index"], r["scene_min"], r["scene_max"])
    for key in ("numInnerNodes", "numLeafNodes", "numEmptyLeaves", "numTriRefs", "maxDepth"):
        assert h.info[key] == r["stats"][key], key
    # every leaf lists ascending ids
    for _, _, ids in np_kdtree.leaf_cells(r["nodes"], r["tri_index"], r["scene_min"], r["scene_max"]):
        assert ids == sorted(ids)
    # records against brute force over the same Woop rows, outside the differences DESIGN.md 6c allows (triangles in zero-width
    # cells; near-equal t)
    rays = np.concatenate([scenes.primary_rays(cam, 48, 48)[0], scenes.box_rays(pos, 2048, 13)])
    got = np_kdtree.trace(r["nodes"], r["woop"], r["tri_index"], r["scene_min"], r["scene_max"], rays)
    # brute force: the CPU oracle's closest hits through a SAH BVH of the same scene
    from oracle import oracle
    bvh = nt.sah_build(tri, pos)
    ref, _ = oracle.trace(bvh.nodes, bvh.woop, bvh.tri_index, rays, any_hit=False)
    # the allowed differences of DESIGN.md 6c, as the SAH kd-tree's agreement test states them
    from test_kdtree_gpu import classify_disagreements
    other, agree, counts = classify_disagreements(got, ref, rays, h, tri, pos)
    assert other.size == 0, (counts, other[:5])
    assert agree >= 0.999, counts


def test_params_rejected_before_the_device():
    lib = nt.lib()
    h = C.c_void_p()
    fake = C.c_void_p(16)     # never dereferenced: the checks come first
    bad = [dict(triLimit=0), dict(failureCount=-1), dict(triMaxLimit=-1), dict(depthK1=float("nan")), dict(ci=float("inf")),
           dict(ct=float("nan")), dict(failRq=float("inf")), dict(depthK2=float("-inf")), dict(depthK1=10.0), dict(depthK2=65.0)]
    for kw in bad:
        p = nt.kdtree_device_params(**kw)
        assert lib.ntr_kdtree_device_build(1000, fake, 3, fake, C.byref(p), C.byref(h), None) == -1, kw
        assert h.value is None
    p = nt.kdtree_device_params()
    assert (p.triLimit, p.triMaxLimit, p.failureCount) == (16, 16, 0)
    assert np.allclose([p.depthK1, p.depthK2, p.ci, p.ct, p.failRq], [1.2, 2.0, 1.0, 1.0, 0.9])
    assert lib.ntr_kdtree_device_build(0, fake, 3, fake, None, C.byref(h), None) == -1
    assert lib.ntr_kdtree_device_build(4, None, 3, fake, None, C.byref(h), None) == -1
    assert lib.ntr_kdtree_device_build(4, fake, 3, None, None, C.byref(h), None) == -1
    assert lib.ntr_kdtree_device_build(4, fake, 3, fake, None, None, None) == -1
    with pytest.raises(nt.NtrError):
        nt.kdtree_device_build(1, 3, 1, 3, dict(triLimit=0))
    # the depth limit: 1.2 * log2(2^20) + 2 = 26, within the stack; 3.2 * 20 + 2 = 66 is not
    assert kb.max_depth(1 << 20) == 26
    p = nt.kdtree_device_params(depthK1=3.2)
    assert lib.ntr_kdtree_device_build(1 << 20, fake, 3, fake, C.byref(p), C.byref(h), None) == -1


def test_atrium_spec_runs_quickly():
    import time
    tri, pos, _ = scenes.atrium()
    t0 = time.time()
    r = kb.build(tri, pos, woop=False)
    dt = time.time() - t0
    assert dt < 40.0, dt
    st = r["stats"]
    assert st["numTriRefs"] >= tri.shape[0] and st["maxDepth"] <= kb.max_depth(tri.shape[0])
