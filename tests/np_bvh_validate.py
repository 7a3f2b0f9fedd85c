"""ntr_bvh_validate's five flags, stated twice (test helper).

* expected_flags: the rules as include/ntrace_amd.h documents them (the ntr_bvh_validate comment), over a whole Compact node array.
* VALUE_BITS and ORDER_PAIRS: literal tables, written by hand from the same text and not computed from the function above.  VALUE_BITS
  names, for each threshold value, the range flags that one box coordinate of that value takes away from an otherwise ordinary tree;
  ORDER_PAIRS says which (lo, hi) pairs are ordered.  tests/test_bvh_validate_cpu.py holds the two statements against each other,
  tests/test_bvh_validate_gpu.py holds the kernel against both.

A Compact node is 16 words: words 0..11 are the two child boxes as (lo, hi) pairs -- c0.x, c0.y, c1.x, c1.y, c0.z, c1.z --, words 12 and
13 the two children (negative: ~(row of the leaf's first Woop row)), words 14 and 15 unused."""
import numpy as np

import ntrace_amd as nt

F = np.float32
U = np.uint32

FINITE, FASTDIV, NOTINY, ORDERED, WIDE_LEAVES = nt.BVH_FINITE, nt.BVH_FASTDIV, nt.BVH_NOTINY, nt.BVH_ORDERED, nt.BVH_WIDE_LEAVES
assert (FINITE, FASTDIV, NOTINY, ORDERED, WIDE_LEAVES) == (1, 2, 4, 8, 16)


def node_words(nodes):
    """any view of a Compact node buffer as int32[n, 16]"""
    a = np.ascontiguousarray(nodes)
    return a.reshape(-1).view(np.uint8).view(np.int32).reshape(-1, 16)


def expected_flags(nodes, woop_bytes=None):
    """ntr_bvh_validate's flags restated over a Compact node array (woop_bytes: unused, the leaf statistics come from the child words)."""
    w = node_words(nodes)
    box = w[:, :12].view(F).astype(np.float64)         # NaN stays NaN, every float32 is exact
    mag = np.abs(box)
    flags = 0
    with np.errstate(invalid="ignore"):
        if bool(np.all(np.isfinite(box) & (mag < 2.0 ** 100))):
            flags |= FINITE
        if bool(np.all(mag < 2.0 ** 55)):              # false for NaN
            flags |= FASTDIV
        if bool(np.all((box == 0.0) | (mag >= 2.0 ** -93))):   # a NaN is neither
            flags |= NOTINY
        if bool(np.all(box[:, 0::2] <= box[:, 1::2])):
            flags |= ORDERED
    child = w[:, 12:14].reshape(-1).astype(np.int64)
    leaf = child[child < 0]
    if leaf.size > 0:
        L, M = int(leaf.size), int((~leaf).max())
        if M / L >= 7.0:
            flags |= WIDE_LEAVES
    return flags


def bits_of(x):
    return int(np.asarray(x, dtype=F).view(U))


# ---- the hand-written table ------------------------------------------------------------------------------------------------------------
# float32 bit patterns of the magnitudes (sign bit clear); each holds for both signs
P55, P55_BELOW = 0x5B000000, 0x5AFFFFFF           # 2^55 = 2^(182 - 127): exponent field 182 = 0xB6 -> 0x5B000000
P100, P100_BELOW = 0x71800000, 0x717FFFFF         # 2^100: exponent field 227 = 0xE3 -> 0x71800000
INF, QNAN, FLT_MAX_BITS = 0x7F800000, 0x7FC00000, 0x7F7FFFFF
M93, M93_BELOW = 0x11000000, 0x10FFFFFF           # 2^-93: exponent field 34 = 0x22 -> 0x11000000
DENORM_MAX, DENORM_MIN, ZERO = 0x007FFFFF, 0x00000001, 0x00000000

_MAGNITUDE_BITS = {
    P55: FASTDIV,                       # |x| < 2^55 fails at 2^55 itself
    P55_BELOW: 0,
    P100: FINITE | FASTDIV,
    P100_BELOW: FASTDIV,
    INF: FINITE | FASTDIV,
    QNAN: FINITE | FASTDIV | NOTINY | ORDERED,   # no compare with NaN holds: it is not "0 or >= 2^-93", and its pair is not lo <= hi
    FLT_MAX_BITS: FINITE | FASTDIV,     # the empty sibling box of a one-leaf tree: lo = FLT_MAX, hi = -FLT_MAX
    M93: 0,
    M93_BELOW: NOTINY,
    DENORM_MAX: NOTINY,
    DENORM_MIN: NOTINY,
    ZERO: 0,
}
# word -> the flags a box coordinate of that value clears, whichever slot it stands in (ORDERED for non-NaN values depends on the slot's
# partner and is not part of this table: ORDER_PAIRS)
VALUE_BITS = {}
for _m, _b in _MAGNITUDE_BITS.items():
    VALUE_BITS[_m] = _b
    VALUE_BITS[_m | 0x80000000] = _b
assert len(VALUE_BITS) == 24

# (lo word, hi word) -> is the pair ordered (lo <= hi under float compare)
ORDER_PAIRS = {
    (0x3FC00000, 0x3FC00000): True,     # lo == hi = 1.5
    (0xBFC00000, 0xBFC00000): True,     # -1.5
    (0x3FC00001, 0x3FC00000): False,    # lo one ulp above hi
    (0xBFBFFFFF, 0xBFC00000): False,    # the same below zero: -1.5 + ulp > -1.5
    (0x00000001, 0x00000000): False,    # the smallest denormal above +0
    (0x00000000, 0x80000000): True,     # (+0, -0)
    (0x80000000, 0x00000000): True,     # (-0, +0)
    (0x7FC00000, 0x3FC00000): False,    # NaN as lo
    (0x3FC00000, 0x7FC00000): False,    # NaN as hi
    (0xFFC00000, 0x7FC00000): False,    # NaN as both
    (0x7F7FFFFF, 0xFF7FFFFF): False,    # the empty box
    (0xFF800000, 0x7F800000): True,     # (-inf, +inf)
}
