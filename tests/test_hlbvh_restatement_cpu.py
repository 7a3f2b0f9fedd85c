"""The HLBVH restatement (tests/np_hlbvh.py) on hand-built scenes, its invariants, and the argument checks of ntr_hlbvh_build.

Scenes use an explicit scene box [0, 1024]^3, so the Morton grid step is exactly 1 and a cluster of hlbvhBits = b is a cube of 2^b
grid cells along each axis."""
import ctypes as C

import numpy as np
import pytest

import np_hlbvh as H
import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

BOX = (np.zeros(3, np.float32), np.full(3, 1024.0, np.float32))


def tris_at(points, size=1.0, z=None):
    """One small right triangle in the xy plane per point (corner at the point)."""
    pos, tri = [], []
    for i, p in enumerate(points):
        p = np.asarray(p, np.float32)
        pos += [p + (size, 0, 0), p + (0, size, 0), p]
        tri.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(tri, np.int32), np.array(pos, np.float32)


def children(r, node):
    return r["tree"][node][:2]


def leaf_ranges(r):
    out = []
    for ch in r["tree"].values():
        out += [(c[1], c[2]) for c in ch[:2] if c[0] == "leaf"]
    return sorted(out)


def test_line_sah_plane_differs_from_morton_split():
    # Five single-triangle clusters on the x axis at x = 8, 400, 480, 560, 1000 (y = z = 100).  Morton's top split is the highest
    # differing code bit, x = 512: {8, 400, 480} | {560, 1000}.  Binned SAH over the root box [0, 1024] (step 128): the cluster mids
    # fall into x bins 0, 3, 3, 4, 7; on y and z every cluster is in one bin (no finite cost there).  Costs of the x planes, with a
    # cluster box of 1 x 1 x 0 (area 2) and a span box of w x 1 x 0 (area 2w):
    #   plane 0 {8} | 4 clusters over [400, 1001]:  1 * 2 + 4 * 2 * 601 = 4810
    #   plane 2/3 {8,400,480} | {560,1000}:       3 * 2 * 473 + 2 * 2 * 441 = 4602  (plane 2 comes first and wins the tie with 3)
    #   plane 3 is the same split as plane 2; plane 4..6 {8..560} | {1000}: 4 * 2 * 553 + 2 = 4426
    # so SAH cuts off the far cluster at x = 1000 (first of the equal planes 4, 5, 6 wins), unlike Morton.
    tri, pos = tris_at([(8, 100, 100), (400, 100, 100), (480, 100, 100), (560, 100, 100), (1000, 100, 100)])
    r = H.hlbvh_build(tri, pos, 4, leaf_size=1, epsilon=0.0, bbox=BOX)
    assert r["num_clusters"] == 5 and r["top_nodes"] == 4
    node, axis, (left, right) = r["structure"][0]
    assert node == 0 and axis == 0
    assert left == [0, 1, 2, 3] and right == [4]
    lb = oracle.lbvh_build(tri, pos, 1, 0.0, bbox=BOX)
    assert H.canonical_hash(r) != oracle.bvh_canonical_hash(lb["nodes"], lb["woop"], lb["tri_index"])
    # the next level: {8} | {400, 480, 560}: 1 * 2 + 3 * 2 * 161 = 968 beats every other plane of the box [8, 561]
    node1, axis1, (l1, r1) = r["structure"][1]
    assert axis1 == 0 and l1 == [0] and r1 == [1, 2, 3]


def test_split_missed_odd_cluster_count():
    # three clusters of bits 4 (16-cell cubes) at x = 1, 17, 33: every mid is in bin 0 of the root box on every axis -> no plane has two
    # non-empty sides -> object split, cntR = 3 // 2 = 1, cntL = 2, the two LOWEST Morton clusters go left, axis word 0.
    tri, pos = tris_at([(33, 1, 1), (1, 1, 1), (17, 1, 1)])
    r = H.hlbvh_build(tri, pos, 4, leaf_size=1, epsilon=0.0, bbox=BOX)
    assert r["num_clusters"] == 3
    node, axis, (left, right) = r["structure"][0]
    assert axis == 0 and left == [0, 1] and right == [2]
    assert r["tree"][0][2] == 0
    # the left child's task box is the occupied bin's box (all three clusters): x in [1, 34], step 33 / 8 -> the two clusters split
    _, axis1, (l1, r1) = r["structure"][1]
    assert (l1, r1) == ([0], [1])
    assert sorted(r["tri_sorted"][[s for s, _ in leaf_ranges(r)]].tolist()) == [0, 1, 2]


def test_flat_scene_nan_bins_go_to_bin_zero():
    # a floor: every z is 0, so the task box is flat in z and (mid - lo) / step = 0 / 0 = NaN -> bin 0 for every cluster
    rng = np.random.default_rng(5)
    pts = np.zeros((40, 3), np.float32)
    pts[:, :2] = rng.integers(0, 1000, size=(40, 2))
    tri, pos = tris_at(pts)
    lo = pos.min(axis=0)
    hi = pos.max(axis=0)
    assert lo[2] == hi[2] == 0
    r = H.hlbvh_build(tri, pos, 2, leaf_size=2, epsilon=0.001)
    starts = r["cluster_starts"]
    cl_lo, cl_hi = H.cluster_boxes(tri, pos, r["tri_sorted"], starts)
    _, _, _, _, bins = H.find_split(cl_lo, cl_hi, lo, hi)
    assert (bins[:, 2] == 0).all() and len(set(bins[:, 0])) > 1
    check_invariants(tri, pos, r, 2)


def test_bin_index_conversion_rule():
    inf = np.float32(np.inf)
    assert H.bin_index(np.float32(np.nan)) == 0
    assert H.bin_index(inf) == 7 and H.bin_index(-inf) == 0
    assert H.bin_index(np.float32(6.999)) == 6 and H.bin_index(np.float32(7.0)) == 7 and H.bin_index(np.float32(1e30)) == 7
    assert H.bin_index(np.float32(-0.0)) == 0 and H.bin_index(np.float32(-0.5)) == 0


def test_one_cluster_is_one_bottom_tree():
    # every triangle in one 2^9-cell cube: one cluster; the tree is the bottom-level tree of the whole range (no self-referencing root)
    rng = np.random.default_rng(1)
    tri, pos = tris_at(rng.integers(0, 500, size=(30, 3)))
    r = H.hlbvh_build(tri, pos, 9, leaf_size=2, epsilon=0.0, bbox=BOX)
    assert r["num_clusters"] == 1 and r["top_nodes"] == 0 and r["bottom_roots"] == [(0, 0, 30)]
    check_invariants(tri, pos, r, 2)


def test_bits_zero_five_triangles():
    # hlbvhBits = 0: predFalse, every triangle is a cluster and a leaf of one triangle; no bottom level
    tri, pos = tris_at([(10, 10, 10), (900, 10, 10), (10, 900, 10), (10, 10, 900), (500, 500, 500)])
    r = H.hlbvh_build(tri, pos, 0, leaf_size=1, epsilon=0.0, bbox=BOX)
    assert r["num_clusters"] == 5 and r["top_nodes"] == 4 and r["num_inner"] == 4 and r["num_leaves"] == 5
    assert r["bottom_roots"] == []
    assert leaf_ranges(r) == [(i, i + 1) for i in range(5)]


def test_equal_code_run_depth_rule_differs_from_lbvh():
    # 40 identical triangles plus one far away, hlbvhBits = 1, leafSize 2: the run's cluster is a bottom root at level 3 * 1 - 1 = 2,
    # so after 3 median levels the depth rule makes leaves of 5 triangles; the LBVH keeps splitting down to leaves of <= 2
    tri, pos = tris_at([(100, 100, 100)] * 40 + [(900, 900, 900)])
    r = H.hlbvh_build(tri, pos, 1, leaf_size=2, epsilon=0.0, bbox=BOX)
    sizes = sorted(e - s for s, e in leaf_ranges(r))
    assert sizes == [1] + [5] * 8
    lb = oracle.lbvh_build(tri, pos, 2, 0.0, bbox=BOX)
    assert max(lb["num_leaves"], 0) > 9
    assert H.canonical_hash(r) != oracle.bvh_canonical_hash(lb["nodes"], lb["woop"], lb["tri_index"])
    check_invariants(tri, pos, r, 2)


def test_sign_of_zero_never_reaches_a_decision():
    rng = np.random.default_rng(9)
    pts = rng.integers(0, 50, size=(60, 3)).astype(np.float32)
    pts[:, 2] = 0.0
    tri, pos = tris_at(pts)
    neg = pos.copy()
    neg[neg == 0] = np.float32(-0.0)
    for bits in (0, 2):
        a = H.hlbvh_build(tri, pos, bits, leaf_size=1, epsilon=0.0)
        b = H.hlbvh_build(tri, neg, bits, leaf_size=1, epsilon=0.0)
        assert a["structure"] == b["structure"]
        assert leaf_ranges(a) == leaf_ranges(b)


def check_invariants(tri, pos, r, leaf_size):
    n = tri.shape[0]
    nodes = r["nodes"].view(np.int32).reshape(-1, 16)
    woop = r["woop"].view(np.uint32).reshape(-1, 4)
    seen = []
    for i, ch in r["tree"].items():
        for k, c in enumerate(ch[:2]):
            if c[0] == "leaf":
                s, e = c[1], c[2]
                assert e > s
                out = ~nodes[i, 12 + k]
                seen += r["tri_index"][out:out + 3 * (e - s):3].tolist()
                assert woop[out + 3 * (e - s), 0] == 0x80000000
            else:
                j = c[1]
                f, g = nodes[i].view(np.float32), nodes[j].view(np.float32)
                box = [f[0 + 4 * k], f[1 + 4 * k], f[2 + 4 * k], f[3 + 4 * k], f[8 + 2 * k], f[9 + 2 * k]]
                union = [min(g[0], g[4]), max(g[1], g[5]), min(g[2], g[6]), max(g[3], g[7]), min(g[8], g[10]), max(g[9], g[11])]
                assert np.array_equal(np.array(box, np.float32), np.array(union, np.float32))
    assert sorted(seen) == list(range(n))
    assert r["num_inner"] == r["num_leaves"] - 1
    assert r["woop"].nbytes == (3 * n + r["num_leaves"]) * 16 and r["tri_index"].shape[0] == 3 * n + r["num_leaves"]
    assert r["nodes"].nbytes == 64 * r["num_inner"]
    capn, capw, capi = nt.lbvh_capacity(n)
    assert r["nodes"].nbytes <= capn and r["woop"].nbytes <= capw and r["tri_index"].nbytes <= capi


@pytest.mark.parametrize("bits", [0, 1, 3, 5, 8])
@pytest.mark.parametrize("seed", [1, 2])
def test_invariants_random_soups(bits, seed):
    tri, pos, _ = scenes.random_soup(700 if bits else 300, seed=seed)
    for leaf_size in (1, 4):
        r = H.hlbvh_build(tri, pos, bits, leaf_size=leaf_size)
        check_invariants(tri, pos, r, leaf_size)
        res, _ = oracle.trace(r["nodes"], r["woop"], r["tri_index"], scenes.random_rays(256, seed))
        bf = oracle.bruteforce_closest(r["woop"], r["tri_index"], scenes.random_rays(256, seed))
        assert np.array_equal(res["t"].view(np.uint32), bf["t"].view(np.uint32))


def test_capacity_worst_case_bits0_leafsize1():
    tri, pos, _ = scenes.random_soup(500, seed=4)
    r = H.hlbvh_build(tri, pos, 0, leaf_size=1)
    n = tri.shape[0]
    assert r["num_leaves"] == n and r["num_inner"] == n - 1
    check_invariants(tri, pos, r, 1)


def test_bits10_and_small_n_are_the_lbvh():
    tri, pos, _ = scenes.random_soup(900, seed=3)
    r = H.hlbvh_build(tri, pos, 10)
    lb = oracle.lbvh_build(tri, pos, 8, 0.001)
    assert H.canonical_hash(r) == oracle.bvh_canonical_hash(lb["nodes"], lb["woop"], lb["tri_index"])
    small_t, small_p = tri[:6], pos
    r = H.hlbvh_build(small_t, small_p, 4)
    lb = oracle.lbvh_build(small_t, small_p, 8, 0.001)
    assert r["lbvh_path"] and H.canonical_hash(r) == oracle.bvh_canonical_hash(lb["nodes"], lb["woop"], lb["tri_index"])


# ---- argument checks of ntr_hlbvh_build (they come before any device call) ----
def _call(bits=4, res=True, cap_short=0):
    L = nt.lib()
    n = 100
    capn, capw, capi = nt.lbvh_capacity(n)
    mn = (C.c_float * 3)(0, 0, 0)
    mx = (C.c_float * 3)(1, 1, 1)
    r = nt.HlbvhResult()
    fake = C.c_void_p(0x1000)
    return L.ntr_hlbvh_build(n, fake, 300, fake, mn, mx, 8, C.c_float(0.001), bits, fake, capn - cap_short, fake, capw, fake, capi,
                             C.byref(r) if res else None, None)


def test_capi_argument_errors():
    assert _call(bits=11) == -1
    assert _call(bits=-1) == -1
    assert _call(res=False) == -1
    assert _call(cap_short=64) == -1
    assert b"capacity" in nt.lib().ntr_last_error()
