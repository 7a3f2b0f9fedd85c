"""float32 numpy restatement of the certain-step rule of the per-ray kernels' wave-uniform prologue (trace_kernels.hip: certain_reach,
certain_end, uniform_prologue<.., CERTAIN>) and of the exact slab test it stands in for (Intersect::RayBox, Util.cpp:34-46, with
select-form folds).  Every value is the float32 the kernel holds: the two single-rounding products / fused multiply-adds of the
kernel are formed exactly in float64 (24-bit operands and power-of-two factors: at most 47 significant bits) and rounded once."""
import numpy as np

F = np.float32
D = np.float64
REACH_MIN = F(2.0 ** -100)


def reach(tmax, d):
    """certain_reach: RN(RN(tmax |d|) (1 + 2^-20)), or +inf when the product is below 2^-100 (or not a number)."""
    with np.errstate(all="ignore"):
        p = (np.asarray(tmax, F) * np.abs(np.asarray(d, F))).astype(F)
        grown = (p.astype(D) * D(1.0 + 2.0 ** -20)).astype(F)
        return np.where(p >= REACH_MIN, grown, F(np.inf)).astype(F)


def end(o, r, sign):
    """certain_end: s = RN(o +- reach), then fma(|s|, +-2^-22, s): outward by two to four ulp of s."""
    with np.errstate(all="ignore"):
        o = np.asarray(o, F)
        s = (o + r).astype(F) if sign > 0 else (o - r).astype(F)
        return (s.astype(D) + np.abs(s).astype(D) * D(sign * 2.0 ** -22)).astype(F)


def segment(o, d, tmax):
    """(segLo, segHi), three arrays each: the origin on the side the ray leaves, the inflated far end on the other"""
    lo, hi = [], []
    for k in range(3):
        r = reach(tmax, d[k])
        neg = np.asarray(d[k], F) < 0
        ok = np.asarray(o[k], F)
        lo.append(np.where(neg, end(ok, r, -1), ok).astype(F))
        hi.append(np.where(neg, ok, end(ok, r, +1)).astype(F))
    return lo, hi


def inside(box, o):
    lox, hix, loy, hiy, loz, hiz = box
    return (lox <= o[0]) & (o[0] <= hix) & (loy <= o[1]) & (o[1] <= hiy) & (loz <= o[2]) & (o[2] <= hiz)


def outside(box, seg_lo, seg_hi):
    lox, hix, loy, hiy, loz, hiz = box
    return (lox > seg_hi[0]) | (hix < seg_lo[0]) | (loy > seg_hi[1]) | (hiy < seg_lo[1]) | (loz > seg_hi[2]) | (hiz < seg_lo[2])


def certain(box0, box1, o, seg_lo, seg_hi):
    """(certain, take0): the lane's step is settled by comparisons; it takes child 0 (else child 1).  box = (lox, hix, loy, hiy, loz, hiz)."""
    take0 = inside(box0, o) & outside(box1, seg_lo, seg_hi)
    take1 = inside(box1, o) & outside(box0, seg_lo, seg_hi)
    return take0 | take1, take0


def _sel_min(a, b):
    return np.where(a < b, a, b)


def _sel_max(a, b):
    return np.where(a > b, a, b)


def exact_accept(box, o, d, tmin, tmax):
    """The exact test: (accept, mn) with t = (plane - o) / d in float32, select-form min / max folds, and the three accept compares."""
    lox, hix, loy, hiy, loz, hiz = box
    with np.errstate(all="ignore"):
        q = lambda p, k: ((np.asarray(p, F) - o[k]).astype(F) / d[k]).astype(F)
        t0x, t1x, t0y, t1y, t0z, t1z = q(lox, 0), q(hix, 0), q(loy, 1), q(hiy, 1), q(loz, 2), q(hiz, 2)
        mn = _sel_max(_sel_max(_sel_min(t0x, t1x), _sel_min(t0y, t1y)), _sel_min(t0z, t1z))
        mx = _sel_min(_sel_min(_sel_max(t0x, t1x), _sel_max(t0y, t1y)), _sel_max(t0z, t1z))
        return (mn <= mx) & (mx >= tmin) & (mn <= tmax), mn
