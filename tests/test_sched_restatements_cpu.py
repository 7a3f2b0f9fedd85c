"""The numpy restatements of the scheduling layer (np_sched.py) against independent derivations: fma32 against exact rational
arithmetic, sched_order against a brute-force sort, top_table against a recursive walk, pool_k on its boundary cases and every
block_incoherence branch on hand-built rays.  The GPU tests (test_sched_kernels_gpu.py) then hold the kernels to these restatements."""
from fractions import Fraction

import numpy as np
import pytest

import ntrace_amd as nt
import np_sched as S
from kat_vectors import two_leaf_bvh
from ntrace_amd import scenes


def round_f32(x):
    """Exact value -> float32, round to nearest even (overflow to inf); the reference fma32 must match."""
    if x == 0:
        return 0.0
    neg, x = x < 0, abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    k = max(e, -126) - 23
    q = x / Fraction(2) ** k
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** k
    out = float("inf") if v >= Fraction(2) ** 128 else float(v)
    return -out if neg else out


def exact_fma(a, b, c):
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:   # an exact zero sum is -0 only when both addends are -0 (round to nearest)
        return -0.0 if (np.signbit(a) != np.signbit(b)) and np.signbit(c) and (a == 0 or b == 0) and c == 0 else 0.0
    return round_f32(x)


def same_f32(x, y):
    return np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32)


def test_fma32_equals_exact_rounding_on_random_inputs():
    rng = np.random.default_rng(1)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 2.0 ** rng.integers(-30, 0, n))).astype(np.float32)   # cancellation
    c[::3] = (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(np.float32)[::3]
    got = S.fma32(a, b, c)
    for i in range(n):
        want = exact_fma(a[i], b[i], c[i])
        assert np.float32(want).view(np.uint32) == got[i].view(np.uint32), (a[i], b[i], c[i], got[i], want)


def test_fma32_on_constructed_midpoints_overflow_and_subnormals():
    cases = []
    one = np.float32(1.0)
    # products with bits far below float32 precision, and addends that put the exact sum on, or a residue below float64 precision
    # beside, a float32 rounding boundary; the overflow threshold 2^128 - 2^103; subnormal results; signed zeros
    for a, b, c in [
            (1 + 2.0 ** -12, 1 + 2.0 ** -12, -2.0 ** -24 - 2.0 ** -11),
            (1 + 2.0 ** -12, 1 - 2.0 ** -12, 2.0 ** -24),
            (1 + 2.0 ** -23, 1 + 2.0 ** -23, -2.0 ** -22),
            (1 + 2.0 ** -23, 1 + 2.0 ** -23, 2.0 ** -24 - 2.0 ** -22),
            (1 - 2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -24 + 2.0 ** -23),
            (1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** -24),
            (1 + 3 * 2.0 ** -23, 1 + 2.0 ** -23, -2.0 ** -21 + 2.0 ** -24),
            (3.0e38, 1.5, -1.0e38), (3.0e38, 1.5, -1.1e38), (2.0 ** 127, 2.0 - 2.0 ** -23, 2.0 ** 103),
            (2.0 ** 127, 2.0 - 2.0 ** -23, 2.0 ** 103 - 2.0 ** 80), (-(2.0 ** 127), 2.0 - 2.0 ** -23, -(2.0 ** 103)),
            (2.0 ** -75, 2.0 ** -75, 2.0 ** -149), (2.0 ** -75, 1.5 * 2.0 ** -75, 0.0), (2.0 ** -100, 2.0 ** -50, -0.0),
            (1.5 * 2.0 ** -149, 0.5, 2.0 ** -170), (-0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, -0.0),
            (1e-45, 1e30, -1e-15)]:
        cases.append((np.float32(a), np.float32(b), np.float32(c)))
    # the midpoints above 1 + k ulp reached exactly, and off by a product's low bits
    for k in range(8):
        a = np.float32(1 + k * 2.0 ** -23)
        cases += [(a, one, np.float32(2.0 ** -24)), (a, np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24 - 2.0 ** -23 * float(a)))]
    a, b, c = (np.array(x, np.float32) for x in zip(*cases))
    got = S.fma32(a, b, c)
    for i in range(len(cases)):
        want = exact_fma(a[i], b[i], c[i])
        assert same_f32(got[i], want), (a[i], b[i], c[i], got[i], want)
    assert S.fma32(np.float32(2.0 ** 127), np.float32(2.0 - 2.0 ** -23), np.float32(2.0 ** 103)) == np.inf
    assert np.isnan(S.fma32(np.float32(np.inf), np.float32(0.0), np.float32(1.0)))
    assert S.fma32(np.float32(np.inf), np.float32(2.0), np.float32(np.nan)) != S.fma32(np.float32(np.inf), np.float32(2.0), np.float32(np.nan))


def brute_sched_order(cost, classes):
    classes = min(max(classes, 1), 64)
    mx = max(int(c) for c in cost)
    to_class = np.float32(classes) / (np.float32(mx) + np.float32(1.0))
    cls = [classes - 1 - min(int(np.float32(int(c)) * to_class), classes - 1) for c in cost]
    return [i for _, i in sorted((cls[i], i) for i in range(len(cost)))]


@pytest.mark.parametrize("classes", [0, 1, 2, 31, 32, 33, 64, 1000])
def test_sched_order_equals_a_brute_force_sort(classes):
    rng = np.random.default_rng(classes)
    for cost in (np.zeros(300, np.uint32), np.full(257, 9, np.uint32), np.arange(511, dtype=np.uint32),
                 rng.integers(0, 5000, 1000).astype(np.uint32), np.r_[rng.integers(0, 40, 600), [0xFFFFFFFF]].astype(np.uint32),
                 (2 ** 24 + rng.integers(-4, 5, 700)).astype(np.uint32)):
        got = S.sched_order(cost, classes)
        assert got.tolist() == brute_sched_order(cost, classes)
        assert np.array_equal(np.sort(got), np.arange(cost.size))


def recursive_boxes(nodes, depth):
    f = nodes.view(np.float32)
    i = nodes.view(np.int32)
    out = []

    def walk(ofs, d):
        if d >= depth or ofs + 64 > nodes.nbytes:
            return
        q = ofs // 4
        out.append((f[q + 0], f[q + 1], f[q + 2], f[q + 3], f[q + 8], f[q + 9]))
        out.append((f[q + 4], f[q + 5], f[q + 6], f[q + 7], f[q + 10], f[q + 11]))
        for ch in (int(i[q + 12]), int(i[q + 13])):
            if ch >= 0:
                walk(ch, d + 1)
    walk(0, 0)
    return np.array(out, np.float32).reshape(-1, 6)


def as_multiset(rows):
    return sorted(tuple(r.view(np.uint32).tolist()) for r in rows)


@pytest.mark.parametrize("depth", [0, 1, 2, 5, 9, 10, 11])
def test_top_table_equals_a_recursive_walk(depth):
    tri, pos = scenes.random_soup(3000, seed=2)[:2]
    bvh = nt.sah_build(tri, pos, 1, 1)
    got = S.top_table(bvh.nodes, bvh.nodes.nbytes, depth)
    want = recursive_boxes(bvh.nodes, min(max(depth, 1), 10))
    assert got.shape[0] == want.shape[0] and as_multiset(got) == as_multiset(want)
    assert np.array_equal(got[:2], want[:2])           # the root's two children come first (block_incoherence reads them)
    # a truncated node buffer: children past its end are skipped
    cut = 64 * 40
    assert as_multiset(S.top_table(bvh.nodes[:cut], cut, depth)) == as_multiset(recursive_boxes(bvh.nodes[:cut], min(max(depth, 1), 10)))


def test_top_table_of_a_root_with_two_leaves():
    nodes = two_leaf_bvh((0, 1, 0, 1, 0, 1), (2, 3, 2, 3, 2, 3), [(0, 0, 0, 0)] * 3, [(0, 0, 0, 0)] * 3, 0, 1)[0]
    for depth in (1, 9, 10):
        t = S.top_table(nodes, 64, depth)
        assert t.tolist() == [[0, 1, 0, 1, 0, 1], [2, 3, 2, 3, 2, 3]]


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 1000, 8193])
def test_pool_k_thresholds(nb):
    D = S.NTR_BATCH_DIVERGENT
    assert S.pool_k(0, 0, nb, 4) == 1
    for apart in {(nb - 1) // 2, nb // 2, (nb + 1) // 2, (nb + 1) // 2 + 1}:    # 2 * apart at nb - 1, nb, nb + 1 (whichever are reachable)
        if apart <= 0:
            continue
        k = S.pool_k(apart, 0, nb, 4) & 0xFFFF
        assert k == (4 if 2 * apart >= nb else 1), (apart, nb)
    for total in (nb - 1, nb, nb + 1):                                           # 4 * apart + score at nb - 1, nb, nb + 1
        for apart in range(0, total // 4 + 1, max(1, total // 8)):
            score = total - 4 * apart
            w = S.pool_k(apart, score, nb, 2)
            assert bool(w & D) == (total >= nb), (apart, score, nb)
            assert (w & 0xFFFF) == (2 if apart > 0 and 2 * apart >= nb else 1)
    assert S.pool_k(0, 5, 0, 2) == 1                  # no blocks: never divergent


def two_ray_block(o1, d1, o2, d2, tmin=0.0, tmax=100.0, tmin2=0.0, tmax2=100.0):
    rays = np.zeros(256, nt.RAY_DTYPE)
    for k, v in zip(("ox", "oy", "oz", "dx", "dy", "dz"), (0, 0, 0, 1, 0, 0)):
        rays[k] = v
    rays["tmax"] = 1.0
    for idx, o, d, t0, t1 in ((100, o1, d1, tmin, tmax), (227, o2, d2, tmin2, tmax2)):
        rays[idx] = (o[0], o[1], o[2], t0, d[0], d[1], d[2], t1)
    return rays


def test_block_incoherence_branches_on_hand_built_rays():
    table = np.array([[0, 8, 0, 4, 0, 2], [4, 16, 0, 8, 0, 1]], np.float32)   # extent max(16, 8, 2) = 16: 1/8 of it = 2
    z, x = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    inc = lambda r: int(S.block_incoherence(r, table)[0])
    assert inc(two_ray_block(z, x, z, x, tmin=1.0, tmax=1.0)) == 8                   # degenerate sample ray
    assert inc(two_ray_block(z, x, z, x, tmin=np.nan)) == 8
    assert inc(two_ray_block(z, x, (2.0001, 0, 0), x)) == 1                          # starts apart: > 1/8 of the extent
    assert inc(two_ray_block(z, x, (2.0, 0, 0), x)) == 0                             # exactly 1/8: together
    assert inc(two_ray_block(z, x, (0, 0, -2.5), x)) == 1
    assert inc(two_ray_block(z, x, (np.nan, 0, 0), (-1.0, 0, 0))) != 1               # NaN distance: not apart
    assert inc(two_ray_block(z, x, z, (1.0, 1.0, 0.0))) == 0                         # 45 degrees
    assert inc(two_ray_block(z, (2.0, 0, 0), z, (1.0, 2.0, 0.0))) == 6               # cos = 1/sqrt(5) < 1/2, long
    assert inc(two_ray_block(z, x, z, (-1.0, 0.0, 0.0))) == 6                        # opposite: dot < 0
    assert inc(two_ray_block(z, x, z, (0.0, 1.0, 0.0), tmax=2.0)) == 2               # reach^2 = 4 = (1/8 ext)^2: not further
    assert inc(two_ray_block(z, x, z, (0.0, 1.0, 0.0), tmax=2.001)) == 6
    assert inc(two_ray_block(z, (0.5, 0, 0), z, (0.0, 1.0, 0.0), tmax=4.0)) == 2     # reach counts the direction's length
    assert inc(two_ray_block(z, (0.0, 0, 0), z, (0.0, 1.0, 0.0))) == 0               # zero-length direction: dot 0, 0 < 0 false
    # cos exactly 1/2 (dot 1, lengths^2 1 and 4: 4 dot^2 == l1 l2) is together; a little wider is not
    assert inc(two_ray_block(z, (1.0, 0, 0), z, (1.0, 1.0, 1.0 * 2 ** 0.5))) == 0
    assert inc(two_ray_block(z, (1.0, 0, 0), z, (1.0, 1.0, 1.0 * 2 ** 0.5 + 1e-6))) == 6
    assert inc(two_ray_block(z, (2.0, 0, 0), z, (0.5, 0.0, 0.0))) == 0               # same direction, other length


def test_block_incoherence_samples_clamp_to_the_last_ray():
    table = np.array([[0, 8, 0, 4, 0, 2], [4, 16, 0, 8, 0, 1]], np.float32)
    rays = np.zeros(300, nt.RAY_DTYPE)
    rays["dx"], rays["tmax"] = 1.0, 100.0
    rays[299] = (9, 9, 9, 0, 0, 1, 0, 100)          # block 1's samples (356, 483) are both ray 299: together, same direction
    rays[227] = (9, 9, 9, 0, 1, 0, 0, 100)          # block 0: lane 227 starts apart
    assert S.block_incoherence(rays, table).tolist() == [1, 0]
    assert S.block_incoherence(rays[:228], table).tolist() == [1]
    assert S.block_incoherence(rays[:227], table).tolist() == [0]     # lane 227 clamps to ray 226, lane 100 is ray 100
    assert S.block_incoherence(rays[:50], table).tolist() == [0]       # both samples clamp to ray 49
    assert S.coherence_words(rays, table, 2, 4) == [1, 0, 4 | S.NTR_BATCH_DIVERGENT]
    assert S.coherence_words(rays, table[:1], 2, 4) == [0, 0, 1]       # fewer than two boxes: nothing looked at


def test_dispatch_class_and_flatten_checker():
    cost = np.array([0, 1, 2, 3, 127, 128, 500, 0xFFFFFFFF], np.uint32)
    assert S.dispatch_class(cost).tolist() == [0, 0, 1, 1, 63, 63, 63, 63]
    cls = np.array([1, 0, 1, 2] * 40)
    nb = cls.size
    good = []
    for k in (2, 1, 0):
        for g in (2, 0, 1):   # any order of the groups
            good += [b for b in range(g * 64, min(nb, g * 64 + 64)) if cls[b] == k]
    assert S.check_flatten_order(good, cls) is None
    bad = list(good)
    bad[0], bad[1] = bad[1], bad[0]
    assert "ascending" in S.check_flatten_order(bad, cls)
    assert "rises" in S.check_flatten_order(good[::-1], cls)
    assert "permutation" in S.check_flatten_order(good[:-1] + [good[0]], cls)
    split = [b for b in good if cls[b] == 2]
    split = split[1:] + split[:1] + [b for b in good if cls[b] != 2]
    assert "split" in S.check_flatten_order(split, cls)
