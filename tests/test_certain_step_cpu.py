"""The certain-step rule of the per-ray kernels' prologue against the exact slab test (no GPU): wherever the rule calls a lane certain,
the exact float32 test -- (plane - o) / d, select-form folds, the three accept compares with tmin = 0 -- accepts exactly the child the
rule takes and rejects its sibling.  np_certain_step.py restates both in float32; all inputs stay inside the FAST path's ranges
(2^-40 <= |d| <= 2^20, 2^-36 <= |o| < 2^55 or o == 0, |plane| < 2^55, boxes lo <= hi)."""
import itertools

import numpy as np

import np_certain_step as cs

F = np.float32
SIGNS = np.array(list(itertools.product((1.0, -1.0), repeat=3)), dtype=F)   # every sign combination of d


def check(box0, box1, o, d, tmax, what):
    """asserts certain => (i0, i1) of the exact test; returns the certain mask"""
    box0, box1 = [np.asarray(a, F) for a in box0], [np.asarray(a, F) for a in box1]
    o, d, tmax = [np.asarray(a, F) for a in o], [np.asarray(a, F) for a in d], np.asarray(tmax, F)
    for b in (box0, box1):
        assert all((b[2 * k] <= b[2 * k + 1]).all() for k in range(3)), what + ": a box with lo > hi"
    for k in range(3):
        ad, ao = np.abs(d[k]), np.abs(o[k])
        assert ((ad >= F(2.0 ** -40)) & (ad <= F(2.0 ** 20))).all(), what + ": direction outside the FAST range"
        assert (((ao >= F(2.0 ** -36)) & (ao < F(2.0 ** 55))) | (o[k] == 0)).all(), what + ": origin outside the FAST range"
    seg_lo, seg_hi = cs.segment(o, d, tmax)
    certain, take0 = cs.certain(box0, box1, o, seg_lo, seg_hi)
    tmin = np.zeros_like(tmax)
    i0, _ = cs.exact_accept(box0, o, d, tmin, tmax)
    i1, _ = cs.exact_accept(box1, o, d, tmin, tmax)
    bad = certain & ((i0 != take0) | (i1 != ~take0))
    assert not bad.any(), "%s: %d of %d certain lanes disagree with the exact test, first at %d" % (what, int(bad.sum()), int(certain.sum()),
                                                                                                    int(np.argmax(bad)))
    return certain


def step_ulps(x, n):
    """x moved by n float32 steps (n may be negative, an array); finite non-zero x whose neighbours stay on its side of zero"""
    x = np.asarray(x, F)
    i = x.view(np.int32).astype(np.int64)
    return (i + np.where(i < 0, -1, 1) * n).astype(np.int32).view(F)


def test_generated_pairs():
    """1.2 M sibling pairs and rays: scenes from 2^-5 to 2^12 units, origins mostly inside one child (some copied from a plane), every
    direction sign, lengths from far shorter to far longer than the boxes; at least a fifth certain and a fifth not."""
    rng = np.random.default_rng(20261017)
    n = 1200000
    S = (2.0 ** rng.uniform(-5, 12, n))
    c = rng.uniform(-4, 4, (n, 3)) * S[:, None]
    half = rng.uniform(0.05, 1.0, (n, 3)) * S[:, None]
    lo, hi = c - half, c + half
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    cut = lo[rows, ax] + rng.uniform(0.1, 0.9, n) * (hi[rows, ax] - lo[rows, ax])
    gap = rng.uniform(-0.05, 0.3, n) * S * (rng.random(n) < 0.7)       # siblings overlap, touch (30 %: the same plane) or stand apart
    lo0, hi0, lo1, hi1 = lo.copy(), hi.copy(), lo.copy(), hi.copy()
    hi0[rows, ax] = cut
    lo1[rows, ax] = np.minimum(cut + gap, hi[rows, ax])
    shrink = rng.uniform(0.0, 0.2, (n, 3)) * half                       # children need not share the parent's other planes
    lo1 += shrink
    lo1 = np.minimum(lo1, hi1)
    which = rng.random(n) < 0.5
    blo, bhi = np.where(which[:, None], lo0, lo1), np.where(which[:, None], hi0, hi1)
    o = blo + rng.random((n, 3)) * (bhi - blo)
    away = rng.random(n) < 0.15
    o[away] = (c + rng.uniform(-1.5, 1.5, (n, 3)) * S[:, None])[away]
    o = o.astype(F)
    lo0, hi0, lo1, hi1 = [a.astype(F) for a in (lo0, hi0, lo1, hi1)]
    hi0, hi1 = np.maximum(lo0, hi0), np.maximum(lo1, hi1)
    onp = rng.random((n, 3)) < 0.1                                       # origin components copied from a plane of either child
    pick = rng.integers(0, 4, (n, 3))
    planes = np.stack([lo0, hi0, lo1, hi1], 0)
    o = np.where(onp, np.take_along_axis(planes, pick[None], 0)[0], o)
    o = np.where(np.abs(o) < F(2.0 ** -36), F(0.0), o)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(np.abs(d) < 1e-6, 1e-6, d) * (2.0 ** rng.uniform(-3, 3, n))[:, None]
    length = S * 2.0 ** rng.uniform(-9, 3, n)
    tmax = (length / np.linalg.norm(d, axis=1)).astype(F)
    box = lambda l, h: (l[:, 0], h[:, 0], l[:, 1], h[:, 1], l[:, 2], h[:, 2])
    certain = check(box(lo0, hi0), box(lo1, hi1), [o[:, k] for k in range(3)], [d[:, k].astype(F) for k in range(3)], tmax, "generated")
    share = float(certain.mean())
    print("generated pairs: %d, certain share %.3f" % (n, share))
    assert n >= 1000000
    assert share >= 0.2, "the generator makes too few certain pairs (%.3f): the test would be vacuous" % share
    assert 1.0 - share >= 0.2, "the generator makes too few uncertain pairs (%.3f)" % (1.0 - share)


def test_origin_on_planes_and_flat_boxes():
    """Origins exactly on a lo or hi plane of their box (every axis, every corner combination), zero-thickness boxes on every axis, siblings
    that touch, overlap or stand apart on either side, every direction sign, short and long rays."""
    cases = []
    for base in (1.0, -3.0, 1000.0, 2.0 ** -8):
        w = abs(base) * 0.5
        for flat in (None, 0, 1, 2):                                    # the origin's box has zero thickness on this axis
            lo0 = np.array([base, base, base])
            hi0 = lo0 + w
            if flat is not None:
                hi0[flat] = lo0[flat]
            for ax in range(3):
                for side, gap in itertools.product((1, -1), (0.0, 0.25 * w, -0.25 * w, 1e-3 * w)):
                    lo1, hi1 = lo0.copy(), hi0.copy()
                    if side > 0:
                        lo1[ax] = hi0[ax] + gap; hi1[ax] = max(lo1[ax], hi0[ax] + w)
                    else:
                        hi1[ax] = lo0[ax] - gap; lo1[ax] = min(hi1[ax], lo0[ax] - w)
                    for flat1 in (False, True):
                        if flat1:
                            (hi1 if side > 0 else lo1)[ax] = (lo1 if side > 0 else hi1)[ax]
                        for corner in itertools.product((0.0, 0.5, 1.0), repeat=3):   # 0 / 1: on the lo / hi plane
                            o = lo0 + np.array(corner) * (hi0 - lo0)
                            for length in (1e-3 * w, 0.2 * w, 0.26 * w, 5.0 * w, 1e6 * w):
                                cases.append((lo0.copy(), hi0.copy(), lo1.copy(), hi1.copy(), o, length))
    a = [np.array([c[i] for c in cases], dtype=np.float64) for i in range(5)]
    length = np.array([c[5] for c in cases])
    m = len(cases)
    rng = np.random.default_rng(5)
    total = certain_n = 0
    for s in SIGNS:
        for dirs in (np.array([0.6, 0.48, 0.64]), np.array([1.0, 2.0 ** -20, 2.0 ** -30]), np.array([2.0 ** -12, 1.0, 0.5])):
            d = (s * dirs)[None, :] + np.zeros((m, 3))
            tmax = (length / np.linalg.norm(dirs)).astype(F)
            lo0, hi0, lo1, hi1, o = [x.astype(F) for x in a]
            box = lambda l, h: (l[:, 0], h[:, 0], l[:, 1], h[:, 1], l[:, 2], h[:, 2])
            for swap in (False, True):                                   # the origin's box as child 0 and as child 1
                b0, b1 = (box(lo1, hi1), box(lo0, hi0)) if swap else (box(lo0, hi0), box(lo1, hi1))
                c = check(b0, b1, [o[:, k] for k in range(3)], [d[:, k].astype(F) for k in range(3)], tmax, "planes")
                total += m
                certain_n += int(c.sum())
    assert certain_n > total // 10 and total - certain_n > total // 10, (certain_n, total)


def test_endpoint_within_4_ulp_of_the_sibling_plane():
    """The ray's far end on axis k lands within +-4 ulp of the sibling's near plane: |o| from 2^-10 to 2^20, reach from 2^-10 |o| to
    2^10 |o|, every direction sign, each axis.  Here the rule's margin decides: it may call the sibling out of reach only where the exact
    near quotient exceeds tmax."""
    rng = np.random.default_rng(11)
    e = np.arange(-10, 21)
    j = np.arange(-10, 11)
    ulps = np.arange(-4, 5)
    reps = 6
    E, J, U, R = [x.reshape(-1) for x in np.meshgrid(e, j, ulps, np.arange(reps), indexing="ij")]
    m = E.size
    total = certain_n = 0
    for s in SIGNS:
        for ax in range(3):
            omag = (2.0 ** E) * rng.uniform(1.0, 2.0, m)
            o = (rng.choice((-1.0, 1.0), (m, 3)) * omag[:, None] * rng.uniform(0.5, 1.0, (m, 3))).astype(F)
            o[:, ax] = (rng.choice((-1.0, 1.0), m) * omag).astype(F)
            d = (s[None, :] * rng.uniform(0.3, 1.0, (m, 3))).astype(F)
            reach = (2.0 ** J) * omag * rng.uniform(1.0, 2.0, m)
            tmax = (reach / np.abs(d[:, ax].astype(np.float64))).astype(F)
            end = (o[:, ax].astype(np.float64) + tmax.astype(np.float64) * d[:, ax].astype(np.float64)).astype(F)   # the far end, rounded once
            end = np.where(end == 0, F(2.0 ** -40) * s[ax], end)
            plane = step_ulps(end, U * np.where(end < 0, -1, 1) * int(s[ax]))     # U > 0: further along the ray
            w = np.maximum(np.abs(o), np.abs(plane)[:, None]).max(1).astype(F)
            lo0, hi0 = o - w[:, None] * F(0.25), o + w[:, None] * F(0.25)            # the origin's box: all the way round the origin
            lo1, hi1 = o - w[:, None] * F(0.5), o + w[:, None] * F(0.5)              # the sibling: wide on the other axes, starts at `plane`
            if s[ax] > 0:
                lo1[:, ax] = plane; hi1[:, ax] = np.maximum(plane, plane + np.abs(plane))
                hi0[:, ax] = np.maximum(o[:, ax], np.minimum(hi0[:, ax], plane))
            else:
                hi1[:, ax] = plane; lo1[:, ax] = np.minimum(plane, plane - np.abs(plane))
                lo0[:, ax] = np.minimum(o[:, ax], np.maximum(lo0[:, ax], plane))
            box = lambda l, h: (l[:, 0], h[:, 0], l[:, 1], h[:, 1], l[:, 2], h[:, 2])
            c = check(box(lo0, hi0), box(lo1, hi1), [o[:, k] for k in range(3)], [d[:, k] for k in range(3)], tmax, "endpoint axis %d" % ax)
            total += m
            certain_n += int(c.sum())
    print("endpoint cases: %d, certain %d" % (total, certain_n))
    assert total >= 24 * 31 * 21 * 9
    assert 0 < certain_n < total


def test_tmax_at_both_ends():
    """tmax so small that tmax |d| is below, at and above the 2^-100 at which the rule stops trusting its product (tiny origins, planes a few
    ulp away, |d| up to 2^20; origin 0 with planes at 2^-93), subnormal tmax, and tmax so large that the reach overflows: 2^100, FLT_MAX, inf
    with |d| down to 2^-40 and coordinates up to 2^54."""
    rng = np.random.default_rng(13)
    m = 20000
    total = certain_n = 0
    for s in SIGNS:
        # small end: the sibling's near plane n ulp beyond the origin's box on axis 0, tmax around the quotient ulp / |d|
        for omag, dmag in ((2.0 ** -36, 2.0 ** 20), (2.0 ** -36, 1.0), (2.0 ** -20, 2.0 ** 20), (0.0, 2.0 ** 20), (0.0, 2.0 ** -7)):
            o = np.full((m, 3), omag, dtype=np.float64) * rng.uniform(1.0, 1.99, (m, 3))
            o = o.astype(F)
            d = (s[None, :] * dmag * rng.uniform(0.5, 1.0, (m, 3))).astype(F)
            n_ulp = rng.integers(1, 5, m)
            if omag == 0.0:
                plane = (s[0] * 2.0 ** -93 * rng.uniform(1.0, 2.0, m)).astype(F)
                w = F(2.0 ** -90)
            else:
                plane = step_ulps(o[:, 0], n_ulp * int(s[0]))
                w = F(omag)
            q = np.abs((plane.astype(np.float64) - o[:, 0]) / d[:, 0].astype(np.float64))
            tmax = (q * 2.0 ** rng.uniform(-3, 3, m)).astype(F)
            tmax[::7] = F(1e-45)                                   # subnormal
            tmax[1::7] = (F(2.0 ** -100) / np.abs(d[1::7, 0])).astype(F)
            tmax[2::7] = step_ulps((F(2.0 ** -100) / np.abs(d[2::7, 0])).astype(F), -1)
            tmax = np.maximum(tmax, F(1e-45))
            lo0, hi0 = o - w, o + w
            lo1, hi1 = o - w, o + w
            if s[0] > 0:
                lo1[:, 0] = plane; hi1[:, 0] = plane + w; hi0[:, 0] = o[:, 0]
            else:
                hi1[:, 0] = plane; lo1[:, 0] = plane - w; lo0[:, 0] = o[:, 0]
            box = lambda l, h: (l[:, 0], h[:, 0], l[:, 1], h[:, 1], l[:, 2], h[:, 2])
            c = check(box(lo0, hi0), box(lo1, hi1), [o[:, k] for k in range(3)], [d[:, k] for k in range(3)], tmax, "small tmax")
            total += m
            certain_n += int(c.sum())
        # large end
        for tm in (2.0 ** 100, np.finfo(F).max, np.inf):
            for dmag in (2.0 ** -40, 1.0, 2.0 ** 20):
                scale = 2.0 ** rng.uniform(-10, 53, m)
                o = (rng.uniform(-1.0, 1.0, (m, 3)) * scale[:, None]).astype(F)
                o = np.where(np.abs(o) < F(2.0 ** -36), F(2.0 ** -36), o)
                d = (s[None, :] * dmag * rng.uniform(1.0, 1.0 + (dmag < 2.0 ** 20) * 0.9, (m, 3))).astype(F)
                w = scale.astype(F)[:, None] * F(0.5)
                lo0, hi0 = o - w, o + w
                off = (rng.choice((-1.0, 1.0), (m, 3)) * rng.uniform(0.0, 3.0, (m, 3)) * (rng.random((m, 3)) < 0.5)).astype(F) * w
                lo1, hi1 = lo0 + off, hi0 + off                      # the sibling: ahead, behind, beside or around the origin
                box = lambda l, h: (l[:, 0], h[:, 0], l[:, 1], h[:, 1], l[:, 2], h[:, 2])
                c = check(box(lo0, hi0), box(lo1, hi1), [o[:, k] for k in range(3)], [d[:, k] for k in range(3)], np.full(m, tm, dtype=F), "large tmax")
                total += m
                certain_n += int(c.sum())
    print("tmax ends: %d, certain %d" % (total, certain_n))
    assert 0 < certain_n < total
