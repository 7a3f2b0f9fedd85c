"""Named scenes of the HLBVH tests (test_hlbvh_restatement_cpu.py, test_hlbvh_gpu.py): each one is placed on a seam of the device
builder's kernels or on a decision of the rule.  What a scene is meant to reach is stated in its `claim` and asserted from the
restatement's outputs by test_hlbvh_restatement_cpu.py (PRECONDITIONS there); the GPU tier builds the same scenes on the device.

The seams (ntrace_amd/csrc/hlbvh_kernels.hip):
  HEAD_THREAD / HEAD_BLOCK   hl_head_count / hl_head_emit: 4 positions per thread, 1024 per workgroup
  BOX_CHUNK / BOX_WAVE / BOX_BLOCK   hl_cluster_box: 16 positions per thread, 1024 per wave, 4096 per workgroup
  BIN_BLOCK                  hl_fill_bins: 256 clusters per workgroup (LDS bins when its live clusters share one task)
  SCAN_BLOCK                 hl_left_count / hl_partition: 1024 clusters per scan block
  HL_CHUNK                   host loop: 8 top levels per read-back

Exact scenes use the box [0, 1024]^3: grid step 1, a cluster of hlbvhBits = b is a cube of 2^b cells.  Morton codes of points
(x, 0, 0) grow with x, so clusters strung along the x axis come out in the order of x and their lengths can be chosen one by one
(`line_scene`); the layout is still read back from the restatement and asserted, never assumed."""
import functools

import numpy as np

import np_hlbvh as H

F = np.float32
BOX = (np.zeros(3, F), np.full(3, 1024.0, F))
HEAD_THREAD, HEAD_BLOCK = 4, 1024
BOX_CHUNK, BOX_WAVE, BOX_BLOCK = 16, 1024, 4096
BIN_BLOCK = 256
SCAN_BLOCK = 1024
HL_CHUNK = 8


def tris_at(points, size=1.0):
    """One small right triangle in the xy plane per point (corner at the point)."""
    pos, tri = [], []
    for i, p in enumerate(points):
        p = np.asarray(p, np.float32)
        pos += [p + (size, 0, 0), p + (0, size, 0), p]
        tri.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(tri, np.int32), np.array(pos, np.float32)


def boxed_tris(lo, hi):
    """One triangle per row whose raw vertex box is exactly [lo, hi]."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    v = np.stack([lo, np.stack([hi[:, 0], lo[:, 1], hi[:, 2]], 1), np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], 1)], 1)
    return np.arange(3 * lo.shape[0], dtype=np.int32).reshape(-1, 3), v.reshape(-1, 3).astype(F)


def line_scene(lengths, bits, seed):
    """Cluster k holds lengths[k] triangles whose box centres lie in the cell (k * 2^bits, 0, 0): equal codes inside a cluster (the
    stable sort keeps them in triangle order, and the triangles of all clusters are interleaved), clusters in the order of k.  Every
    triangle has its own extents; the six extreme extents of a cluster sit at six places spread along it, so a segment of a long
    cluster that a fold loses changes the cluster's box."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    K = lengths.shape[0]
    assert K * (1 << bits) <= 1024
    cl = rng.permutation(np.repeat(np.arange(K), lengths))
    n = cl.shape[0]
    order = np.argsort(cl, kind="stable")
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    d = rng.uniform(0.05, 0.3, size=(n, 6))
    for e in range(6):
        at = ((e + 0.5) / 6 * lengths[cl]).astype(np.int64)
        d[rank == at, e] = 0.45
    centre = np.zeros((n, 3)) + 0.5
    centre[:, 0] += cl * (1 << bits)
    return boxed_tris(centre - d[:, :3], centre + d[:, 3:])


def fill_to(total, lo, hi, rng):
    """Cluster lengths in lo..hi that sum to `total`."""
    out = []
    while total > 0:
        k = int(min(total, rng.integers(lo, hi + 1)))
        out.append(k)
        total -= k
    return out


def soup_in_box(n, seed, hi=1000):
    rng = np.random.default_rng(seed)
    return tris_at(rng.integers(0, hi, size=(n, 3)), size=0.5)


def _head(n):
    rng = np.random.default_rng(n)
    if n == 1023:      # the last position lies inside a longer cluster
        ln = fill_to(1018, 3, 7, rng) + [5]
    elif n == 1024:    # the last position (1023) is a head of its own
        ln = fill_to(1023, 3, 7, rng) + [1]
    elif n == 1025:    # heads at 1023 and 1024, the last one alone in the second workgroup
        ln = fill_to(1023, 3, 7, rng) + [1, 1]
    else:              # heads at 1023, 1024 and 1025; the last cluster crosses 2048
        ln = fill_to(1023, 3, 7, rng) + [1, 1, 7] + fill_to(2049 - 1032 - 9, 4, 7, rng) + [9]
    assert sum(ln) == n
    return line_scene(ln, 1, seed=n) + (1, 4, 0.0, BOX)


def _cluster_box():
    rng = np.random.default_rng(16)
    ln = []

    def pad(to):
        cur = sum(ln)
        assert to >= cur
        if to > cur:
            ln.append(to - cur)
    for L in (15, 16, 17, 1):          # each length starting at, one before and one after a multiple of 16
        for off in (0, -1, 1):
            pad((sum(ln) // 16 + 2) * 16 + off)
            ln.append(L)
    pad(512)
    ln.extend([5, 4, 4, 3])            # chunk [512, 528): its first cluster starts at p0 and ends inside it; three more whole ones
    ln.extend([3, 100])                # [528, 531) then a cluster over several whole chunks of one wave: [531, 631)
    ln.extend([2, 2, 2, 2, 2, 2, 2, 2])
    ln.extend(fill_to(1000 - sum(ln), 3, 6, rng))
    ln.append(60)                      # [1000, 1060) crosses 1024: two waves
    ln.extend(fill_to(4090 - sum(ln), 150, 250, rng))
    ln.append(20)                      # [4090, 4110) crosses 4096: two workgroups
    ln.extend([3, 1])
    return line_scene(ln, 1, seed=16) + (1, 4, 0.0, BOX)


def _levels_halving(count):
    # bits 0, triangles at x = 1000 * 2^-k: every level's SAH plane peels a few clusters off the far end
    pts = [(1000.0 * 2.0 ** -k, 1.0, 1.0) for k in range(count)]
    return tris_at(pts, size=2.0 ** -60) + (0, 1, 0.0, BOX)


def _identical(count, bits=0, leaf_size=1):
    return tris_at([(100, 100, 100)] * count) + (bits, leaf_size, 0.0, BOX)


def _hostile(kind, seed, scale=1.0, eps_rel=0.001, zeros=False, repeated=False, small_box=False, bits=4, leaf_size=4):
    rng = np.random.default_rng(seed)
    n = 900
    if kind == "soup":
        c = rng.uniform(-1, 1, size=(n, 1, 3))
        p = c + rng.normal(0, 0.03, size=(n, 3, 3))
    elif kind == "blobs":      # deep trees, duplicate Morton codes
        centers = rng.uniform(-1, 1, size=(6, 3))
        c = centers[rng.integers(0, 6, size=n)][:, None, :] + rng.normal(0, 1e-3, size=(n, 1, 3))
        p = c + rng.normal(0, 1e-4, size=(n, 3, 3))
    elif kind == "quads":      # coplanar quads on a grid, z in steps of 1/4
        m = 20
        gx, gy = np.meshgrid(np.linspace(-1, 1, m + 1), np.linspace(-1, 1, m + 1))
        z = np.round(rng.uniform(-1, 1, size=gx.shape) * 4) / 4
        v = np.stack([gx, gy, z], -1)
        a, b, cc, d = v[:-1, :-1], v[1:, :-1], v[1:, 1:], v[:-1, 1:]
        p = np.concatenate([np.stack([a, b, cc], 2).reshape(-1, 3, 3), np.stack([a, cc, d], 2).reshape(-1, 3, 3)])
    else:                      # long thin slivers
        c = rng.uniform(-1, 1, size=(n, 1, 3))
        d = rng.normal(size=(n, 1, 3))
        p = c + d * np.array([0.0, 1.0, 1.0])[None, :, None] * 0.3 + rng.normal(0, 1e-4, size=(n, 3, 3))
    pos = (p.reshape(-1, 3) * scale).astype(F)
    if zeros:
        mask = rng.random(pos.shape) < 0.05
        pos[mask] = np.where(rng.random(mask.sum()) < 0.5, F(0.0), F(-0.0))
    tri = np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3)
    if repeated:
        k = rng.integers(0, tri.shape[0], size=tri.shape[0] // 20)
        tri[k, 2] = tri[k, 1]
    bbox = None
    if small_box:              # the scene box covers the middle half of the geometry: codes outside it clamp
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        bbox = ((lo + (hi - lo) * F(0.25)).astype(F), (hi - (hi - lo) * F(0.25)).astype(F))
    return tri, pos, bits, leaf_size, float(F(eps_rel * scale)), bbox


def _sign_of_zero(negative):
    rng = np.random.default_rng(9)
    pts = rng.integers(0, 50, size=(60, 3)).astype(np.float32)
    pts[:, 2] = 0.0
    tri, pos = tris_at(pts)
    if negative:
        pos = pos.copy()
        pos[pos == 0] = np.float32(-0.0)
    return tri, pos, 2, 1, 0.0, None


def _nan_beside_inf():
    # The caller's box is flat in x at 100.  Two triangles have their box centre at x = 100 exactly (0 / 0 = NaN -> bin 0), four at
    # x = 900 (+inf -> bin 7); y in 500..505 falls into one bin of the root and z is equal, so only the x planes have a finite cost: the
    # root splits 2 | 4 by a plane.  Were NaN bin 7, every cluster would share a bin and the root would be an object split 3 | 3.  Below the
    # root every split is a plane in y, so the tree does not depend on the order of the (degenerate) Morton codes.
    lo = np.array([(99, 500 + k, 10) for k in range(2)] + [(899, 502 + k, 10) for k in range(4)], F)
    hi = lo + np.array([2, 0.5, 1], F)
    box = (np.array([100, 0, 0], F), np.array([100, 1024, 1024], F))
    return boxed_tris(lo, hi) + (0, 1, 0.0, box)


def _flat_floor():
    rng = np.random.default_rng(5)
    pts = np.zeros((40, 3), np.float32)
    pts[:, :2] = rng.integers(0, 1000, size=(40, 2))
    return tris_at(pts) + (2, 2, 0.001, None)


# name -> (maker, claim)
SCENES = {
    # ---- head scan: hl_head_count / hl_head_emit ----
    "head_n1023": (lambda: _head(1023), "n = 1024 - 1; the last position lies inside a longer cluster"),
    "head_n1024": (lambda: _head(1024), "n = 1024; position 1023, the last of the workgroup, is a head of its own and writes clsStart[C]"),
    "head_n1025": (lambda: _head(1025), "n = 1024 + 1; heads at 1023 and 1024; the last position is a head alone in its workgroup"),
    "head_n2049": (lambda: _head(2049), "n = 2 * 1024 + 1; heads at 1023, 1024 and 1025; the last cluster crosses 2048"),
    # ---- cluster boxes: hl_cluster_box ----
    "cluster_box": (_cluster_box, "clusters of 15, 16, 17 and 1 at, before and after a multiple of 16; one over whole chunks of a wave; one "
                                  "across 1024 and one across 4096; a chunk of four whole clusters, the first at its p0"),
    # ---- bins: hl_fill_bins ----
    "bins_c255": (lambda: soup_in_box(255, 255) + (0, 1, 0.0, BOX), "C = 256 - 1: one partly filled workgroup"),
    "bins_c256": (lambda: soup_in_box(256, 256) + (0, 1, 0.0, BOX), "C = 256: one full workgroup"),
    "bins_c257": (lambda: soup_in_box(257, 257) + (0, 1, 0.0, BOX), "C = 256 + 1; a level whose first workgroup holds several tasks and "
                                                                     "done clusters beside live ones"),
    # ---- partition: hl_left_count / hl_partition ----
    "part_c1023": (lambda: soup_in_box(1023, 1023) + (0, 1, 0.0, BOX), "C = 1024 - 1: one scan block"),
    "part_c1024": (lambda: soup_in_box(1024, 1024) + (0, 1, 0.0, BOX), "C = 1024: one full scan block"),
    "part_c1025": (lambda: soup_in_box(1025, 1025) + (0, 1, 0.0, BOX), "C = 1024 + 1; a plane-split task starts off the block grid and "
                                                                        "crosses 1024"),
    "part_c2049": (lambda: soup_in_box(2049, 2049) + (0, 1, 0.0, BOX), "C = 2 * 1024 + 1; plane-split tasks off the grid cross 1024 and "
                                                                        "2048; a workgroup of 256 inside one task and one with several"),
    # ---- level chunks: the host loop reads back every HL_CHUNK = 8 levels ----
    "levels_7": (lambda: _levels_halving(17), "top_levels = 8 - 1"),
    "levels_8": (lambda: _levels_halving(20), "top_levels = 8: the first read-back sees live tasks, the second chunk runs empty"),
    "levels_16": (lambda: _levels_halving(47), "top_levels = 2 * 8"),
    "levels_17": (lambda: _levels_halving(52), "top_levels = 2 * 8 + 1"),
    # ---- decisions (the hand-built scenes of test_hlbvh_restatement_cpu.py) ----
    "dec_line_sah": (lambda: tris_at([(8, 100, 100), (400, 100, 100), (480, 100, 100), (560, 100, 100), (1000, 100, 100)])
                     + (4, 1, 0.0, BOX), "the SAH plane differs from the Morton split"),
    "dec_missed_odd": (lambda: tris_at([(33, 1, 1), (1, 1, 1), (17, 1, 1)]) + (4, 1, 0.0, BOX), "a missed split over three clusters"),
    "dec_flat_nan": (_flat_floor, "a flat task box: NaN bins on z"),
    "dec_nan_inf": (_nan_beside_inf, "a root box flat in x: NaN bins (0) beside +inf bins (7) decide a plane split"),
    "dec_one_cluster": (lambda: tris_at(np.random.default_rng(1).integers(0, 500, size=(30, 3))) + (9, 2, 0.0, BOX),
                        "one cluster is one bottom-level tree"),
    "dec_bits_zero": (lambda: tris_at([(10, 10, 10), (900, 10, 10), (10, 900, 10), (10, 10, 900), (500, 500, 500)])
                      + (0, 1, 0.0, BOX), "bits 0: every triangle a cluster and a leaf"),
    "dec_equal_code": (lambda: tris_at([(100, 100, 100)] * 40 + [(900, 900, 900)]) + (1, 2, 0.0, BOX),
                       "an equal-code run of 40 > leaf_size * 2^(3 * bits) = 16: level 0 forces leaves of 5"),
    "dec_zero_pos": (lambda: _sign_of_zero(False), "a floor at z = +0"),
    "dec_zero_neg": (lambda: _sign_of_zero(True), "the same floor with every zero negative"),
    # ---- missed split at scale: the pure object split across workgroups and scan blocks ----
    "missed_257": (lambda: _identical(257), "every task misses; C = 256 + 1; top_levels = 8 + 1"),
    "missed_1025": (lambda: _identical(1025), "every task misses; the right child of the root starts off the grid and crosses 1024"),
    "missed_2049": (lambda: _identical(2049), "every task misses; object-split ranges cross 1024 and 2048"),
    # ---- leaf against bottom root ----
    "leaf_exact": (lambda: line_scene([4, 5] * 24 + [5, 4], 1, seed=4) + (1, 4, 0.0, BOX),
                   "clusters of exactly leaf_size and leaf_size + 1 triangles"),
    "n_eq_leaf": (lambda: soup_in_box(8, 8) + (4, 8, 0.001, BOX), "n = leaf_size: the LBVH path"),
    "n_eq_leaf_plus1": (lambda: soup_in_box(9, 9) + (4, 8, 0.001, BOX), "n = leaf_size + 1: the smallest cluster build"),
    "level0_forced": (lambda: tris_at([(100, 100, 100)] * 70 + [(x, 900, 900) for x in range(0, 1000, 37)]) + (2, 1, 0.0, BOX),
                      "an equal-code run of 70 > 1 * 2^6: the median levels end in forced leaves of two"),
    "bits9": (lambda: soup_in_box(600, 9, hi=1024) + (9, 4, 0.001, BOX), "bits 9: at most 8 clusters, 27 bottom levels"),
    # ---- hostile but finite geometry ----
    "host_blobs": (lambda: _hostile("blobs", 31), "clustered blobs"),
    "host_quads": (lambda: _hostile("quads", 32, bits=3), "the coplanar quad grid"),
    "host_slivers": (lambda: _hostile("slivers", 33), "slivers"),
    "host_1e-30": (lambda: _hostile("soup", 34, scale=1e-30), "scale 1e-30"),
    "host_1e-14": (lambda: _hostile("soup", 35, scale=1e-14), "scale 1e-14"),
    "host_1e17": (lambda: _hostile("soup", 36, scale=1e17), "scale 1e17"),
    "host_1e25": (lambda: _hostile("soup", 37, scale=1e25), "scale 1e25"),
    "host_zeros": (lambda: _hostile("soup", 38, zeros=True, eps_rel=0.0), "coordinates snapped to +-0, epsilon 0"),
    "host_repeated": (lambda: _hostile("slivers", 39, repeated=True, bits=2), "triangles with a repeated vertex"),
    "host_small_box": (lambda: _hostile("soup", 40, small_box=True), "a scene box smaller than the geometry: codes clamp"),
}
UNIT_SCALE = ("cluster_box", "part_c1025", "leaf_exact", "host_blobs", "host_quads", "host_slivers", "host_zeros", "host_repeated",
              "host_small_box")
DECISION = tuple(k for k in SCENES if k.startswith("dec_") or k.startswith("missed_"))


@functools.lru_cache(maxsize=None)
def scene(name):
    """(tri, pos, bits, leaf_size, epsilon, bbox) of a named scene; inputs are checked to be finite and in range."""
    tri, pos, bits, leaf_size, eps, bbox = SCENES[name][0]()
    tri = np.ascontiguousarray(tri, np.int32)
    pos = np.ascontiguousarray(pos, np.float32)
    assert np.isfinite(pos).all() and tri.min() >= 0 and tri.max() < pos.shape[0], name
    assert bbox is None or (np.isfinite(bbox[0]).all() and np.isfinite(bbox[1]).all())
    tri.setflags(write=False)
    pos.setflags(write=False)
    return tri, pos, bits, leaf_size, eps, bbox


def claim(name):
    return SCENES[name][1]


@functools.lru_cache(maxsize=None)
def spec(name):
    """The restatement's tree of a named scene, computed once per process and shared (do not modify)."""
    return build_spec(name)


def build_spec(name):
    """The restatement's tree of a named scene, built anew."""
    tri, pos, bits, leaf_size, eps, bbox = scene(name)
    return H.hlbvh_build(tri, pos, bits, leaf_size=leaf_size, epsilon=eps, bbox=bbox)


def aimed_rays(tri, pos, count, seed):
    """Seeded rays for a scene of any shape: origins around its box, half aimed at a triangle's centroid (so that a thin scene is
    hit), half in random directions through the box; tmax 2 in units of the direction, which reaches past the target."""
    import ntrace_amd as nt
    rng = np.random.default_rng(seed)
    p = pos.astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3 * max(float(np.abs(p).max()), 1e-30))
    o = lo + rng.uniform(-0.5, 1.5, size=(count, 3)) * ext
    target = lo + rng.uniform(0, 1, size=(count, 3)) * ext
    k = rng.integers(0, tri.shape[0], size=count)
    cent = p[tri[k]].mean(axis=1)
    aim = rng.random(count) < 0.5
    target[aim] = cent[aim]
    d = target - o
    rays = np.zeros(count, dtype=nt.RAY_DTYPE)
    for i, a in enumerate("xyz"):
        rays["o" + a], rays["d" + a] = o[:, i].astype(F), d[:, i].astype(F)
    rays["tmin"] = 0.0
    rays["tmax"] = 2.0
    return rays


def level_tasks(r, level):
    """(beg, end) of the top-level tasks of one level, in positions of the partitioned cluster array."""
    return [(d["beg"], d["end"]) for d in r["decisions"] if d["level"] == level]


def _canon(words):
    """uint32 words with every NaN alike, as the canonical hash reads them."""
    w = np.array(words, np.uint32)
    nan = ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)
    return np.where(nan, np.uint32(0x7FC00000), w)


def first_difference(got, ref):
    """Walks two Compact trees from the root in the canonical order (child 0 before child 1) and describes the first node at which
    they differ: its left / right path, both sides' child kinds, leaf triangle ids and the twelve box words.  None if no node differs."""
    def side(t):
        return t["nodes"].view(np.int32), t["woop"].view(np.uint32).reshape(-1, 4), np.asarray(t["tri_index"]).view(np.int32)

    def leaf(t, ref_word):
        _, woop, idx = t
        ids, rows, i = [], [], ~int(ref_word)
        while woop[i, 0] != 0x80000000:
            ids.append(int(idx[i]))
            rows.append(_canon(woop[i:i + 3].reshape(-1)))
            i += 3
        return ids, rows

    a, b = side(got), side(ref)
    stack = [("root", 0, 0)]
    try:
        while stack:
            path, oa, ob = stack.pop()
            na, nb = a[0][oa // 4:oa // 4 + 16], b[0][ob // 4:ob // 4 + 16]
            kinds = [["leaf" if n[12 + k] < 0 else "node" for k in range(2)] for n in (na, nb)]
            leaves = [[leaf(t, n[12 + k])[0] if n[12 + k] < 0 else None for k in range(2)] for t, n in ((a, na), (b, nb))]
            same = kinds[0] == kinds[1] and np.array_equal(_canon(na[:12].view(np.uint32)), _canon(nb[:12].view(np.uint32)))
            same = same and na[14] == nb[14] and leaves[0] == leaves[1]
            for k in range(2):
                if same and na[12 + k] < 0:
                    ra, rb = leaf(a, na[12 + k])[1], leaf(b, nb[12 + k])[1]
                    same = all(np.array_equal(x, y) for x, y in zip(ra, rb))
            if not same:
                def show(n, kd, lv):
                    return "children %s axis %d leaf ids %s box words %s" % (kd, n[14], lv, ["%08x" % w for w in n[:12].view(np.uint32)])
                return "first difference at %s:\n  device: %s\n  spec:   %s" % (path, show(na, kinds[0], leaves[0]), show(nb, kinds[1], leaves[1]))
            for k in (1, 0):
                if na[12 + k] >= 0:
                    stack.append((path + ".LR"[k + 1] if path != "root" else "LR"[k], int(na[12 + k]), int(nb[12 + k])))
    except IndexError:
        return "the walk left the device's buffers below %s" % path
    return None
