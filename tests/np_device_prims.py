"""Plain numpy references of the shared device toolkit (radix_sort.h, device_prims.h), in integer or exact arithmetic: what
ntr_selftest_onesweep / _scan / _scan_block_sums / _float_order / _box_words must return word for word (tests/test_device_prims_gpu.py).
tests/test_device_prims_cpu.py holds these references to something independent of them."""
import numpy as np

U = np.uint32
F = np.float32
FLT_MAX_BITS = 0x7F7FFFFF
BOX_OUT_WORDS = 26   # per merge path and group: words [0..5], members [6], corners [7..12], grown [13..18], of no members [19..24], area [25]


# ---- the one-sweep sort ---------------------------------------------------------------------------------------------------------------
def sort_order(words, passes):
    """the permutation of an LSD sort: one stable argsort of the 8-bit digit per pass, composed over the passes [(shift, pass number), ..]"""
    words = np.asarray(words, dtype=U)
    order = np.arange(words.shape[0])
    for shift, _ in passes:
        digit = (words[order] >> U(shift)) & U(255)
        order = order[np.argsort(digit, kind="stable")]
    return order


def sort_mode0(keys, vals, passes):
    """(keys, values) after the passes; vals None: element i carries i"""
    keys = np.asarray(keys, dtype=U)
    vals = np.arange(keys.shape[0], dtype=np.int32) if vals is None else np.asarray(vals, dtype=np.int32)
    order = sort_order(keys, passes)
    return keys[order], vals[order]


def sort_mode2(key_array, word, stride, vals, passes):
    """element i carries the value vals[i] and the key word key_array[vals[i] * stride + word]"""
    vals = np.asarray(vals, dtype=np.int32)
    words = np.asarray(key_array, dtype=U).reshape(-1)[vals.astype(np.int64) * stride + word]
    order = sort_order(words, passes)
    return words[order], vals[order]


# ---- scans ------------------------------------------------------------------------------------------------------------------------------
def exclusive_scan(items, bits):
    """(exclusive prefix, total) of unsigned items in Python integers, reduced mod 2^bits; a 2-D array scans its columns independently"""
    a = np.asarray(items)
    zero = np.zeros((1,) + a.shape[1:], dtype=object)
    incl = np.cumsum(np.concatenate([zero, a.astype(object)]), axis=0, dtype=object) % (1 << bits)   # incl[i] = items[0] + .. + items[i - 1]
    dt = np.uint32 if bits == 32 else np.uint64
    return incl[:-1].astype(dt), incl[-1:].astype(dt)[0]


# ---- the floats' total order -----------------------------------------------------------------------------------------------------------
def total_key(bits):
    """the place of a float word in the total order, from its IEEE fields: negative words below the positive ones (sign), a negative
    word the lower the larger its magnitude, -0 (-1) just below +0 (0); NaNs have the largest magnitudes and so lie beyond the
    infinities on their sign's side"""
    b = np.asarray(bits, dtype=U).astype(np.int64)
    sign, mag = b >> 31, b & 0x7FFFFFFF
    return np.where(sign == 1, -mag - 1, mag)


def key_bits(key):
    """the float word at a place of the total order"""
    k = np.asarray(key, dtype=np.int64)
    return np.where(k < 0, (-k - 1) | 0x80000000, k).astype(U)


def ord_enc(bits):
    return (total_key(bits) + (1 << 31)).astype(U)


def ord_dec(enc):
    return key_bits(np.asarray(enc, dtype=U).astype(np.int64) - (1 << 31))


def float_order_single(bits):
    """[n][6] as ntr_selftest_float_order writes it: ord_enc, ord_dec(ord_enc), ord_enc_int, ord_dec_int, ord_to_int, ord_from_int"""
    bits = np.asarray(bits, dtype=U)
    k = total_key(bits)
    signed = k.astype(np.int32).view(U)
    return np.stack([ord_enc(bits), bits, signed, bits, signed, ord_enc(bits)], axis=1)


def float_order_pairs(bits):
    """[n][n][2]: ord_min, ord_max of (word i, word j) -- the operand that comes first / last in the total order"""
    bits = np.asarray(bits, dtype=U)
    k = total_key(bits)
    a, b = bits[:, None], bits[None, :]
    first = k[:, None] <= k[None, :]
    last = k[:, None] >= k[None, :]
    return np.stack([np.where(first, a, b), np.where(last, a, b)], axis=2).astype(U)


def float_word_set(seed=7):
    """the zeros, the ends of the denormal and normal ranges, one, the infinities, quiet and signalling NaNs of both signs with low and
    high payloads, and 200 random words"""
    pos = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, FLT_MAX_BITS, 0x7F800000,
           0x7FC00000, 0x7FC00001, 0x7FFFFFFF, 0x7F800001, 0x7FBFFFFF]   # quiet: low, high payload; signalling: low, high payload
    fixed = pos + [w | 0x80000000 for w in pos]
    rnd = np.random.default_rng(seed).integers(0, 1 << 32, 200, dtype=np.uint64)
    return np.concatenate([np.array(fixed, dtype=np.uint64), rnd]).astype(U)


# ---- boxes as six words, wave folds ----------------------------------------------------------------------------------------------------
def _area(lo, hi):
    """box_area_valid in float32, product by product as the device code has it (no contraction)"""
    if not np.all(lo <= hi):
        return F(0)
    x, y, z = (hi - lo).astype(F)
    with np.errstate(over="ignore"):
        return F(F(F(F(x * y) + F(y * z)) + F(z * x)) * F(2))


def box_groups(boxes, group, groups, eps):
    """[groups][26] of one merge path (both paths must give it): the group's box is the min / max of its members' encoded corners"""
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 6)
    group = np.asarray(group)
    enc = ord_enc(boxes.view(U)).astype(np.int64)
    eps = F(eps)
    out = np.zeros((groups, BOX_OUT_WORDS), dtype=U)
    flt_max = np.array([FLT_MAX_BITS], dtype=U).view(F)[0]
    empty = np.concatenate([np.full(3, flt_max, F), np.full(3, -flt_max, F)]).view(U)
    for g in range(groups):
        mem = enc[group == g]
        n = mem.shape[0]
        if n:
            lo_enc, hi_enc = mem[:, :3].min(axis=0), mem[:, 3:].max(axis=0)
            words = np.concatenate([0xFFFFFFFF - lo_enc, hi_enc]).astype(U)
        else:
            words = np.zeros(6, dtype=U)
        lo, hi = ord_dec(~words[:3]).view(F), ord_dec(words[3:]).view(F)
        out[g, 0:6] = words
        out[g, 6] = n
        with np.errstate(over="ignore", invalid="ignore"):
            out[g, 7:13] = np.concatenate([lo, hi]).view(U) if n else empty
            out[g, 13:19] = np.concatenate([(lo - eps).astype(F), (hi + eps).astype(F)]).view(U) if n else empty
            out[g, 19:25] = empty
            out[g, 25] = np.array([_area(lo, hi)], dtype=F).view(U)[0]
    return out


def wave_folds(lane32, lane64):
    """[m][6]: min, max, sum (mod 2^32), or of the wave's 32-bit lane words and the min of its 64-bit ones (low, high), in every lane"""
    a = np.asarray(lane32, dtype=U).reshape(-1, 64)
    q = np.asarray(lane64, dtype=np.uint64).reshape(-1, 64).min(axis=1)
    per_wave = np.stack([a.min(axis=1), a.max(axis=1), (a.astype(np.uint64).sum(axis=1) & np.uint64(0xFFFFFFFF)).astype(U),
                         np.bitwise_or.reduce(a, axis=1), (q & np.uint64(0xFFFFFFFF)).astype(U), (q >> np.uint64(32)).astype(U)], axis=1)
    return np.repeat(per_wave, 64, axis=0)
