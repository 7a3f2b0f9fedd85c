"""The HLBVH restatement (tests/np_hlbvh.py) on hand-built scenes, its invariants, and the argument checks of ntr_hlbvh_build.

Scenes use an explicit scene box [0, 1024]^3, so the Morton grid step is exactly 1 and a cluster of hlbvhBits = b is a cube of 2^b
grid cells along each axis."""
import ctypes as C

import numpy as np
import pytest

import hlbvh_scenes as S
import np_hlbvh as H
import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

BOX = S.BOX
tris_at = S.tris_at


def build(name):
    """(tri, pos, spec tree) of a hand-built scene of hlbvh_scenes.py (its bits, leaf size, epsilon and box)."""
    tri, pos = S.scene(name)[:2]
    return tri, pos, S.spec(name)


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
    tri, pos, r = build("dec_line_sah")
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
    tri, pos, r = build("dec_missed_odd")
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
    tri, pos, r = build("dec_flat_nan")
    lo = pos.min(axis=0)
    hi = pos.max(axis=0)
    assert lo[2] == hi[2] == 0
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
    tri, pos, r = build("dec_one_cluster")
    assert r["num_clusters"] == 1 and r["top_nodes"] == 0 and r["bottom_roots"] == [(0, 0, 30)]
    check_invariants(tri, pos, r, 2)


def test_bits_zero_five_triangles():
    # hlbvhBits = 0: predFalse, every triangle is a cluster and a leaf of one triangle; no bottom level
    tri, pos, r = build("dec_bits_zero")
    assert r["num_clusters"] == 5 and r["top_nodes"] == 4 and r["num_inner"] == 4 and r["num_leaves"] == 5
    assert r["bottom_roots"] == []
    assert leaf_ranges(r) == [(i, i + 1) for i in range(5)]


def test_equal_code_run_depth_rule_differs_from_lbvh():
    # 40 identical triangles plus one far away, hlbvhBits = 1, leafSize 2: the run's cluster is a bottom root at level 3 * 1 - 1 = 2,
    # so after 3 median levels the depth rule makes leaves of 5 triangles; the LBVH keeps splitting down to leaves of <= 2
    tri, pos, r = build("dec_equal_code")
    sizes = sorted(e - s for s, e in leaf_ranges(r))
    assert sizes == [1] + [5] * 8
    lb = oracle.lbvh_build(tri, pos, 2, 0.0, bbox=BOX)
    assert max(lb["num_leaves"], 0) > 9
    assert H.canonical_hash(r) != oracle.bvh_canonical_hash(lb["nodes"], lb["woop"], lb["tri_index"])
    check_invariants(tri, pos, r, 2)


def test_sign_of_zero_never_reaches_a_decision():
    tri, pos = S.scene("dec_zero_pos")[:2]
    neg = S.scene("dec_zero_neg")[1]
    assert np.array_equal(pos, neg) and not np.array_equal(pos.view(np.uint32), neg.view(np.uint32))
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


# ---- the named scenes of hlbvh_scenes.py: each reaches what it claims (asserted from the restatement's outputs) ----
def _lengths(r):
    st = r["cluster_starts"]
    return st[:-1], st[1:]


def _crossing(r, m):
    """Clusters with start < m <= end - 1."""
    s, e = _lengths(r)
    return np.flatnonzero((s < m) & (m <= e - 1))


def _off_grid_crossers(r, missed, block=S.SCAN_BLOCK):
    """Tasks of level >= 1 whose range of cluster positions starts off a multiple of `block` and crosses one."""
    return [d for d in r["decisions"] if d["level"] >= 1 and d["missed"] == missed and d["beg"] % block != 0
            and d["beg"] // block != (d["end"] - 1) // block]


def _workgroup_tasks(r, level, w, block=S.BIN_BLOCK):
    """(tasks overlapping workgroup w of hl_fill_bins at a level, live positions, done positions) of the partitioned cluster array."""
    a, b = w * block, min((w + 1) * block, r["num_clusters"])
    live = np.zeros(b - a, bool)
    tasks = 0
    for beg, end in S.level_tasks(r, level):
        lo, hi = max(beg, a), min(end, b)
        if lo < hi:
            tasks += 1
            live[lo - a:hi - a] = True
    return tasks, int(live.sum()), int((~live).sum())


def _pre_head(n, heads, last_alone):
    def check(r, sc):
        st = r["cluster_starts"]
        assert sc[0].shape[0] == n and n in (S.HEAD_BLOCK - 1, S.HEAD_BLOCK, S.HEAD_BLOCK + 1, 2 * S.HEAD_BLOCK + 1)
        assert set(heads) <= set(st.tolist())
        assert (int(st[-2]) == n - 1) == last_alone          # the thread that holds n - 1 writes clsStart[C]
    return check


def test_head_scenes_end_in_different_slots_of_a_thread():
    # position n - 1 falls into three of the HEAD_THREAD = 4 slots of its thread across the head scenes
    assert {(S.scene(k)[0].shape[0] - 1) % S.HEAD_THREAD for k in S.SCENES if k.startswith("head_")} == {0, 2, 3}


def _pre_cluster_box(r, sc):
    s, e = _lengths(r)
    ln = e - s
    C = S.BOX_CHUNK
    for L in (15, 16, 17, 1):
        for off in (0, C - 1, 1):
            assert ((ln == L) & (s % C == off)).any(), (L, off)
    # whole chunks of one wave inside one cluster
    whole = (e // C) - ((s + C - 1) // C)
    assert ((whole >= 3) & (s // S.BOX_WAVE == (e - 1) // S.BOX_WAVE)).any()
    two_waves = _crossing(r, S.BOX_WAVE)
    two_groups = _crossing(r, S.BOX_BLOCK)
    assert two_waves.size == 1 and two_groups.size == 1 and r["cluster_starts"][-1] > S.BOX_BLOCK
    # a chunk with three or more whole clusters whose first cluster starts at its p0 and ends inside it (the plain-store branch) ...
    first_at_p0 = [k for k in range(s.shape[0]) if s[k] % C == 0 and e[k] < s[k] + C
                   and ((s >= s[k]) & (e <= s[k] + C)).sum() >= 3]
    assert first_at_p0
    # ... beside a chunk whose first cluster started before its p0 and ends inside it (the atomic branch)
    started_earlier = [k for k in range(s.shape[0]) if s[k] % C != 0 and s[k] // C != (e[k] - 1) // C and e[k] % C != 0]
    assert started_earlier
    # long clusters: the six extreme extents lie in different chunks, so a lost segment changes the box
    k = int(two_groups[0])
    tri, pos = sc[0], sc[1]
    v = pos[tri[r["tri_sorted"][s[k]:e[k]]]]
    where = set(np.argmin(v.min(axis=1), axis=0).tolist()) | set(np.argmax(v.max(axis=1), axis=0).tolist())
    assert len({(int(s[k]) + w) // C for w in where}) >= 2
    assert min(where) + s[k] < S.BOX_BLOCK <= max(where) + s[k]


def _pre_bins(c, multi):
    def check(r, sc):
        assert r["num_clusters"] == c and c in (S.BIN_BLOCK - 1, S.BIN_BLOCK, S.BIN_BLOCK + 1)
        assert _workgroup_tasks(r, 0, 0)[0] == 1                 # level 0: one task per workgroup, the LDS bins
        if multi:                                                # several tasks and done clusters beside live ones: global atomics
            found = [lv for lv in range(1, r["top_levels"]) if _workgroup_tasks(r, lv, 0)[0] >= 2 and _workgroup_tasks(r, lv, 0)[2] >= 1
                     and _workgroup_tasks(r, lv, 0)[1] >= 1]
            assert found
    return check


def _pre_part(c, crossing):
    def check(r, sc):
        assert r["num_clusters"] == c and c in (S.SCAN_BLOCK - 1, S.SCAN_BLOCK, S.SCAN_BLOCK + 1, 2 * S.SCAN_BLOCK + 1)
        assert bool(_off_grid_crossers(r, missed=False)) == crossing
        if c == 2 * S.SCAN_BLOCK + 1:
            crossed = {m for d in _off_grid_crossers(r, False) for m in (S.SCAN_BLOCK, 2 * S.SCAN_BLOCK) if d["beg"] < m < d["end"]}
            assert crossed == {S.SCAN_BLOCK, 2 * S.SCAN_BLOCK}
            # below the root: a workgroup of 256 clusters all of one task (LDS bins) and one that holds several tasks
            groups = [_workgroup_tasks(r, 1, w) for w in range((c + S.BIN_BLOCK - 1) // S.BIN_BLOCK)]
            assert any(t == 1 and live == S.BIN_BLOCK for t, live, _ in groups) and any(t >= 2 for t, _, _ in groups)
    return check


def _pre_levels(k):
    def check(r, sc):
        assert r["top_levels"] == k and k in (S.HL_CHUNK - 1, S.HL_CHUNK, 2 * S.HL_CHUNK, 2 * S.HL_CHUNK + 1)
    return check


def _pre_missed(c):
    def check(r, sc):
        assert r["num_clusters"] == c and all(d["missed"] for d in r["decisions"]) and len(r["decisions"]) == c - 1
        assert all(d["cnt_l"] == (d["end"] - d["beg"]) - (d["end"] - d["beg"]) // 2 for d in r["decisions"])
        assert any((d["end"] - d["beg"]) % 2 for d in r["decisions"])
        if c > S.SCAN_BLOCK:
            assert _off_grid_crossers(r, missed=True)
        if c > 2 * S.SCAN_BLOCK:
            assert any(d["beg"] < 2 * S.SCAN_BLOCK < d["end"] for d in _off_grid_crossers(r, True))
        assert c in (S.BIN_BLOCK + 1, S.SCAN_BLOCK + 1, 2 * S.SCAN_BLOCK + 1)
        if c == S.BIN_BLOCK + 1:      # the scene of exactly HL_CHUNK + 1 levels: ceil(log2(257)) halvings
            assert r["top_levels"] == S.HL_CHUNK + 1
    return check


def _pre_leaf_exact(r, sc):
    leaf = sc[3]
    s, e = _lengths(r)
    assert set((e - s).tolist()) == {leaf, leaf + 1}
    leaves = set(leaf_ranges(r))
    roots = {(a, b) for _, a, b in r["bottom_roots"]}
    for a, b in zip(s.tolist(), e.tolist()):
        assert ((a, b) in leaves) == (b - a == leaf) and ((a, b) in roots) == (b - a == leaf + 1)


def _pre_forced(r, sc):
    bits, leaf = sc[2], sc[3]
    assert max(e - s for s, e in leaf_ranges(r)) > leaf
    s, e = _lengths(r)
    assert (e - s).max() > leaf * 2 ** (3 * bits)


def _pre_hostile(r, sc):
    assert 300 <= sc[0].shape[0] <= 1500 and r["num_clusters"] >= 2


def _missed_odd(r, sc):
    assert any(d["missed"] and (d["end"] - d["beg"]) % 2 == 1 and d["level"] == 0 for d in r["decisions"])


def _scale(exp):
    def check(r, sc):
        _pre_hostile(r, sc)
        m = np.abs(sc[1]).max()
        assert 10.0 ** (exp - 1) < m < 10.0 ** (exp + 1) and sc[4] == pytest.approx(0.001 * 10.0 ** exp, rel=1e-3)
    return check


def _pre_zeros(r, sc):
    _pre_hostile(r, sc)
    bits = sc[1].view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any() and sc[4] == 0.0


def _pre_repeated(r, sc):
    _pre_hostile(r, sc)
    assert (sc[0][:, 1] == sc[0][:, 2]).any()


def _pre_small_box(r, sc):
    _pre_hostile(r, sc)
    lo, hi = sc[5]
    assert (sc[1] < lo).any() and (sc[1] > hi).any()
    tri, pos = sc[0], sc[1]
    mid = (pos[tri].min(axis=1) + pos[tri].max(axis=1)) / 2
    assert ((mid < lo).any(axis=1) | (mid > hi).any(axis=1)).sum() > 50      # box centres outside the box: their codes clamp


def _nan_inf(r, sc):
    d = r["decisions"][0]
    assert not d["missed"] and d["axis"] == 0 and d["cnt_l"] == 2 and sc[5][0][0] == sc[5][1][0]


PRECONDITIONS = {
    "head_n1023": _pre_head(1023, (), False), "head_n1024": _pre_head(1024, (1023,), True),
    "head_n1025": _pre_head(1025, (1023, 1024), True), "head_n2049": _pre_head(2049, (1023, 1024, 1025), False),
    "cluster_box": _pre_cluster_box,
    "bins_c255": _pre_bins(255, False), "bins_c256": _pre_bins(256, False), "bins_c257": _pre_bins(257, True),
    "part_c1023": _pre_part(1023, False), "part_c1024": _pre_part(1024, False), "part_c1025": _pre_part(1025, True),
    "part_c2049": _pre_part(2049, True),
    "levels_7": _pre_levels(7), "levels_8": _pre_levels(8), "levels_16": _pre_levels(16),
    "levels_17": _pre_levels(17),
    "dec_line_sah": lambda r, sc: None, "dec_missed_odd": _missed_odd, "dec_flat_nan": lambda r, sc: None, "dec_nan_inf": _nan_inf,
    "dec_one_cluster": lambda r, sc: None, "dec_bits_zero": lambda r, sc: None, "dec_equal_code": _pre_forced,
    "dec_zero_pos": lambda r, sc: None, "dec_zero_neg": lambda r, sc: None,
    "missed_257": _pre_missed(257), "missed_1025": _pre_missed(1025), "missed_2049": _pre_missed(2049),
    "leaf_exact": _pre_leaf_exact,
    "n_eq_leaf": lambda r, sc: (r["lbvh_path"] and sc[0].shape[0] == sc[3]) or pytest.fail("not the LBVH path"),
    "n_eq_leaf_plus1": lambda r, sc: (not r["lbvh_path"] and sc[0].shape[0] == sc[3] + 1) or pytest.fail("not the cluster path"),
    "level0_forced": _pre_forced,
    "bits9": lambda r, sc: (sc[2] == 9 and 2 <= r["num_clusters"] <= 8 and len(r["bottom_roots"]) >= 2) or pytest.fail("bits 9"),
    "host_blobs": _pre_hostile, "host_quads": _pre_hostile, "host_slivers": _pre_hostile,
    "host_1e-30": _scale(-30), "host_1e-14": _scale(-14), "host_1e17": _scale(17), "host_1e25": _scale(25),
    "host_zeros": _pre_zeros, "host_repeated": _pre_repeated, "host_small_box": _pre_small_box,
}


def test_every_named_scene_has_a_precondition():
    # the six decision scenes without an entry of their own are asserted by the hand-built tests at the top of this file
    assert set(PRECONDITIONS) == set(S.SCENES)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_named_scene_reaches_its_claim(name):
    sc, r = S.scene(name), S.spec(name)
    PRECONDITIONS[name](r, sc)
    if not r["lbvh_path"]:
        check_invariants(sc[0], sc[1], r, sc[3])
        # the additive decision record agrees with `structure`
        assert [(d["node"], d["axis"], d["cnt_l"]) for d in r["decisions"]] == [(nd, ax, len(p[0])) for nd, ax, p in r["structure"]]
        assert all(d["end"] - d["beg"] == len(p[0]) + len(p[1]) for d, (_, _, p) in zip(r["decisions"], r["structure"]))
    if name in S.UNIT_SCALE:
        rays = S.aimed_rays(sc[0], sc[1], 256, 3)
        res, _ = oracle.trace(r["nodes"], r["woop"], r["tri_index"], rays)
        bf = oracle.bruteforce_closest(r["woop"], r["tri_index"], rays)
        assert np.array_equal(res["t"].view(np.uint32), bf["t"].view(np.uint32))
        assert (res["id"] >= 0).any()


# ---- discrimination: one-point changes of the rule, applied to the restatement, change the tree of the scenes that pin them ----
def _lt_where_it_can(bins_a, b):
    """`bin < split` for `bin <= split`, at every task where that leaves both children a cluster.  A device that sent `bin < split`
    left would still take cntL from the sweep; where the two disagree about an empty side there is no tree to compare, so the change
    is applied where it yields one (any task whose winning plane is not the first occupied bin)."""
    left = bins_a < b
    return left if left.any() and not left.all() else bins_a <= b


def _mutants(bits):
    cl = H.clusters
    m = {"cnt_r": ("missed_cnt_right", lambda n: (n + 1) // 2),
         "lt": ("left_of_plane", _lt_where_it_can),
         "nan7": ("NAN_BIN", 7)}
    if bits >= 1:      # at bits 0 there is no bottom level, so a restatement with merged clusters has no tree to compare
        m["shift+3"] = ("clusters", lambda keys, b: cl(keys, b + 1))
        m["shift-3"] = ("clusters", lambda keys, b: cl(keys, b - 1))
    return m


# Which change each scene tells from the rule BY ITS CANONICAL HASH (a changed restatement that raises tells nothing and fails the
# test).  Not every scene can see every change: NaN bins matter only where NaN and another bin meet on one axis, cntR only where a
# split is missed over an odd count, `bin < split` only where a winning plane is not the first occupied bin, the key shift only where
# it moves a cluster border.  dec_bits_zero sees none of them (five clusters whose winning planes are all first bins; bits 0 has no
# key shift): what it pins is asserted by test_bits_zero_five_triangles.  Every change is pinned by at least one scene (test below).
KILLS = {
    "dec_line_sah": ("lt",), "dec_missed_odd": ("cnt_r", "shift+3"), "dec_flat_nan": ("lt",), "dec_nan_inf": ("nan7", "lt"),
    "dec_one_cluster": ("shift-3",), "dec_bits_zero": (), "dec_equal_code": ("shift-3",), "dec_zero_pos": ("lt",),
    "dec_zero_neg": ("lt",), "missed_257": ("cnt_r",), "missed_1025": ("cnt_r",), "missed_2049": ("cnt_r",),
}


def test_every_rule_change_is_pinned():
    assert set(KILLS) == set(S.DECISION)
    assert {m for v in KILLS.values() for m in v} == {"cnt_r", "lt", "nan7", "shift+3", "shift-3"}


@pytest.mark.parametrize("name", [k for k, v in KILLS.items() if v])
def test_decision_scenes_tell_the_rule_from_its_neighbours(name, monkeypatch):
    tri, pos, bits, leaf, eps, bbox = S.scene(name)
    base = H.canonical_hash(S.spec(name))
    mutants = _mutants(bits)
    originals = {a: getattr(H, a) for a, _ in mutants.values()}
    for m in KILLS[name]:
        attr, value = mutants[m]
        with monkeypatch.context() as mp:
            mp.setattr(H, attr, value)
            got = H.canonical_hash(H.hlbvh_build(tri, pos, bits, leaf_size=leaf, epsilon=eps, bbox=bbox))
        assert got != base, (name, m)
    assert all(getattr(H, a) is v for a, v in originals.items())      # the rule is back in place


def test_line_sah_root_under_bin_lt_split():
    # the root's winning plane 4 has the bins 0, 3, 3, 4 on its left: `bin < split` sends 3 | 2 instead of 4 | 1
    tri, pos, bits, leaf, eps, bbox = S.scene("dec_line_sah")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(H, "left_of_plane", _lt_where_it_can)
        r = H.hlbvh_build(tri, pos, bits, leaf_size=leaf, epsilon=eps, bbox=bbox)
    assert r["structure"][0][2] == [[0, 1, 2], [3, 4]] and S.spec("dec_line_sah")["structure"][0][2] == [[0, 1, 2, 3], [4]]


# ---- the mismatch report of the GPU tier, on two restatement trees ----
def test_first_difference_names_the_node():
    tri, pos, bits, leaf, eps, bbox = S.scene("dec_missed_odd")
    good = S.spec("dec_missed_odd")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(H, "missed_cnt_right", lambda n: (n + 1) // 2)
        bad = H.hlbvh_build(tri, pos, bits, leaf_size=leaf, epsilon=eps, bbox=bbox)
    assert S.first_difference(good, good) is None
    msg = S.first_difference(bad, good)      # cntR = 2: the root's children are leaf | node instead of node | leaf
    assert msg.startswith("first difference at root:") and "['leaf', 'node']" in msg and "['node', 'leaf']" in msg
    # a difference below the root is named by its path: under `bin < split` dec_nan_inf keeps its root and changes below it
    tri, pos, bits, leaf, eps, bbox = S.scene("dec_nan_inf")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(H, "left_of_plane", _lt_where_it_can)
        bad = H.hlbvh_build(tri, pos, bits, leaf_size=leaf, epsilon=eps, bbox=bbox)
    msg = S.first_difference(bad, S.spec("dec_nan_inf"))
    assert msg.split(":")[0] in ("first difference at L", "first difference at R", "first difference at RL", "first difference at RR")
    # buffers that end early are reported, not raised
    cut = dict(nodes=good["nodes"][:64], woop=good["woop"], tri_index=good["tri_index"])
    assert "left the device's buffers" in S.first_difference(cut, good)
