"""The two statements of ntr_bvh_validate's flags (tests/np_bvh_validate.py) against each other, without a GPU: the restatement over a
node array and the hand-written tables VALUE_BITS and ORDER_PAIRS, every value in every one of the 12 box slots of an ordinary tree."""
import numpy as np
import pytest

import np_bvh_validate as nv
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED, WIDE_LEAVES, VALUE_BITS, ORDER_PAIRS, expected_flags

F = np.float32
U = np.uint32
BOX = FINITE | FASTDIV | NOTINY | ORDERED


def f32(word):
    return np.array([word], dtype=U).view(F)[0]


def ordinary(n=5):
    """n nodes with boxes of a few units, lo < hi in every pair, and leaves at small offsets"""
    w = np.zeros((n, 16), dtype=np.int32)
    box = w[:, :12].view(F)
    box[:, 0::2] = np.arange(n, dtype=F)[:, None] - 2.5
    box[:, 1::2] = np.arange(n, dtype=F)[:, None] + 1.25
    w[:, 12] = 64
    w[:, 13] = ~(4 * np.arange(n, dtype=np.int32))
    return w


def test_the_table_names_the_values_it_should():
    want = [2.0 ** 55, np.nextafter(F(2.0 ** 55), F(0)), 2.0 ** 100, np.nextafter(F(2.0 ** 100), F(0)), np.inf, np.finfo(F).max, 2.0 ** -93,
            np.nextafter(F(2.0 ** -93), F(0)), 2.0 ** -126 - 2.0 ** -149, 2.0 ** -149, 0.0]
    for x in want:
        for s in (1.0, -1.0):
            assert nv.bits_of(s * x) in VALUE_BITS, x
    assert 0x7FC00000 in VALUE_BITS and 0xFFC00000 in VALUE_BITS and np.isnan(f32(0x7FC00000))
    assert len(VALUE_BITS) == 2 * (len(want) + 1)


def test_an_ordinary_tree_has_the_four_box_flags():
    assert expected_flags(ordinary()) & BOX == BOX


@pytest.mark.parametrize("slot", range(12))
def test_restatement_and_table_agree_on_every_value_in_every_slot(slot):
    clean = ordinary()
    base = expected_flags(clean)
    for word, cleared in sorted(VALUE_BITS.items()):
        for node in (0, 2, 4):
            w = clean.copy()
            w[node, slot] = np.array([word], dtype=U).view(np.int32)[0]
            lo, hi = w[node, slot & ~1:(slot & ~1) + 2].view(F)
            want = base & ~cleared
            if not (lo <= hi):
                want &= ~ORDERED
            assert expected_flags(w) == want, "word 0x%08x in slot %d of node %d" % (word, slot, node)


@pytest.mark.parametrize("pair", range(6))
def test_restatement_and_table_agree_on_the_ordered_pairs(pair):
    for (lo, hi), ordered in ORDER_PAIRS.items():
        w = ordinary()
        w[3, 2 * pair:2 * pair + 2] = np.array([lo, hi], dtype=U).view(np.int32)
        got = expected_flags(w)
        assert bool(got & ORDERED) == ordered, "(0x%08x, 0x%08x) in pair %d" % (lo, hi, pair)
        # and the range flags are what the two values alone call for
        assert got & (FINITE | FASTDIV | NOTINY) == (FINITE | FASTDIV | NOTINY) & ~VALUE_BITS.get(lo, 0) & ~VALUE_BITS.get(hi, 0)


def test_words_12_to_15_are_not_box_coordinates():
    w = ordinary()
    base = expected_flags(w)
    for word in (0x7F800000, 0x7FC00000, 0x00000001, 0x7F7FFFFF):      # positive words: no leaf statistics change either
        for col in (12, 14, 15):
            x = w.copy()
            x[:, col] = np.array([word], dtype=U).view(np.int32)[0]
            assert expected_flags(x) == base
    x = w.copy()
    x[1, 14] = x[1, 15] = np.array([0xFF800000], dtype=U).view(np.int32)[0]     # a negative word outside the child words is no leaf
    assert expected_flags(x) == base


@pytest.mark.parametrize("L", (1, 2, 3, 1000))
def test_wide_leaves_at_the_ratio_seven(L):
    for M, want in ((7 * L, True), (7 * L - 1, False), (7 * L + 1, True)):
        w = np.zeros((L, 16), dtype=np.int32)
        w[:, 12] = 64
        w[:, 13] = ~np.arange(L, dtype=np.int32)
        w[L // 2, 13] = ~M
        assert bool(expected_flags(w) & WIDE_LEAVES) == want, (L, M)
    w = np.zeros((3, 16), dtype=np.int32)
    w[:, 12:14] = 64
    assert not expected_flags(w) & WIDE_LEAVES, "no leaf, no ratio"
