"""The numpy references of the device toolkit's self tests (np_device_prims.py) held to something independent of them -- no GPU:
the composed per-digit sort against one stable argsort of the whole key, the total order of the float words against `<`, the scan
against a running sum, the box merge against numpy's own min / max where those are defined."""
import numpy as np

import np_device_prims as ref

U = np.uint32
F = np.float32
PASSES4 = [(0, 0), (8, 1), (16, 2), (24, 3)]


def test_composed_digit_sort_is_one_stable_sort_of_the_whole_key():
    rng = np.random.default_rng(1)
    for n in (1, 2, 257, 5000):
        for keys in (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U), rng.integers(0, 7, n).astype(U) * U(0x01010101),
                     np.full(n, 0xFFFFFFFF, dtype=U)):
            order = np.argsort(keys, kind="stable")
            assert np.array_equal(ref.sort_order(keys, PASSES4), order)
            k, v = ref.sort_mode0(keys, None, PASSES4)
            assert np.array_equal(k, keys[order]) and np.array_equal(v, order.astype(np.int32))
            vals = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
            assert np.array_equal(ref.sort_mode0(keys, vals, PASSES4)[1], vals[order])


def test_mode2_reference_sorts_the_values_by_the_word_they_point_at():
    rng = np.random.default_rng(2)
    n = 1000
    key_array = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(U)
    perm = rng.permutation(n).astype(np.int32)
    k1, v1 = ref.sort_mode2(key_array, 1, 6, perm, PASSES4)
    k0, v0 = ref.sort_mode2(key_array, 0, 6, v1, PASSES4)
    # two chained words == one stable sort by (word 0, word 1) of the elements in their first order
    wide = (key_array[perm, 0].astype(np.uint64) << np.uint64(32)) | key_array[perm, 1].astype(np.uint64)
    assert np.array_equal(v0, perm[np.argsort(wide, kind="stable")])
    assert np.array_equal(k0, key_array[v0, 0]) and np.array_equal(k1, key_array[v1, 1])
    assert np.array_equal(ref.sort_mode2(key_array[:, 0].copy(), 0, 1, perm, PASSES4)[1], ref.sort_mode2(key_array, 0, 6, perm, PASSES4)[1])


def test_total_order_agrees_with_less_than_and_places_zeros_and_nans():
    words = ref.float_word_set()
    key = ref.total_key(words)
    f = words.view(F)
    assert len(set(key.tolist())) == len(set(words.tolist())), "distinct words have distinct places"
    ok = np.isfinite(f) & (f != 0)
    assert ok.sum() > 150
    fi, ki = f[ok].astype(np.float64), key[ok]
    assert np.array_equal(fi[:, None] < fi[None, :], ki[:, None] < ki[None, :])
    place = lambda w: int(ref.total_key(np.array([w], dtype=U))[0])
    assert place(0x80000000) + 1 == place(0x00000000)                       # -0 just before +0
    assert place(0x80000001) < place(0x80000000) and place(0x00000000) < place(0x00000001)
    inf_p, inf_n = place(0x7F800000), place(0xFF800000)
    assert inf_n < place(0xFF7FFFFF) and place(0x7F7FFFFF) < inf_p
    for nan in (0x7FC00000, 0x7FC00001, 0x7FFFFFFF, 0x7F800001, 0x7FBFFFFF):
        assert np.isnan(np.array([nan], dtype=U).view(F)[0])
        assert place(nan) > inf_p and place(nan | 0x80000000) < inf_n      # beyond the infinities, by sign
    # the unsigned encoding keeps the order and is what device_prims.h states: sign set -> all bits flipped, else the sign bit set
    enc = ref.ord_enc(words)
    assert np.array_equal(enc[:, None] < enc[None, :], key[:, None] < key[None, :])
    assert np.array_equal(enc, np.where(words >> U(31), ~words, words | U(0x80000000)))


def test_decode_of_encode_is_the_identity_on_every_word_of_the_set():
    words = ref.float_word_set()
    assert np.array_equal(ref.ord_dec(ref.ord_enc(words)), words)
    assert np.array_equal(ref.key_bits(ref.total_key(words)), words)
    single = ref.float_order_single(words)
    assert np.array_equal(single[:, 1], words) and np.array_equal(single[:, 3], words) and np.array_equal(single[:, 5], single[:, 0])
    pairs = ref.float_order_pairs(words)
    assert np.array_equal(pairs[:, :, 0], pairs[:, :, 0].T) and np.array_equal(pairs[:, :, 1], pairs[:, :, 1].T)   # no result depends on the operands' order
    i = np.arange(words.shape[0])
    assert np.array_equal(pairs[i, i, 0], words) and np.array_equal(pairs[i, i, 1], words)
    f = words.view(F)
    ok = np.isfinite(f) & (f != 0)
    assert np.array_equal(pairs[np.ix_(ok, ok)][:, :, 0].view(F), np.minimum(f[ok][:, None], f[ok][None, :]))
    assert np.array_equal(pairs[np.ix_(ok, ok)][:, :, 1].view(F), np.maximum(f[ok][:, None], f[ok][None, :]))


def test_scan_reference_is_the_running_sum_reduced():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(U)
    ex, tot = ref.exclusive_scan(a, 32)
    run = 0
    for i in range(a.shape[0]):
        assert int(ex[i]) == run
        run = (run + int(a[i])) & 0xFFFFFFFF
    assert int(tot) == run and run != int(a.astype(np.uint64).sum()), "the sums must wrap"
    a4 = rng.integers(0, 1 << 32, (300, 4), dtype=np.uint64).astype(U)
    ex4, tot4 = ref.exclusive_scan(a4, 32)
    for c in range(4):
        exc, totc = ref.exclusive_scan(a4[:, c], 32)
        assert np.array_equal(ex4[:, c], exc) and tot4[c] == totc
    b = rng.integers(0, 1 << 64, 100, dtype=np.uint64)
    ex64, tot64 = ref.exclusive_scan(b, 64)
    assert int(ex64[-1]) == sum(int(x) for x in b[:-1]) % (1 << 64) and int(tot64) == sum(int(x) for x in b) % (1 << 64)
    ex0, tot0 = ref.exclusive_scan(np.zeros(0, dtype=U), 32)
    assert ex0.shape == (0,) and int(tot0) == 0


def test_box_reference_is_numpys_min_and_max_away_from_the_zeros():
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=(256, 3)).astype(F), rng.normal(size=(256, 3)).astype(F)
    boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)
    group = rng.integers(-1, 5, 256)
    group[group == 3] = -1                                    # group 3 receives nothing
    eps = F(1e-3)
    out = ref.box_groups(boxes, group, 5, eps)
    for g in range(5):
        mem = boxes[group == g]
        assert out[g, 6] == mem.shape[0]
        if g == 3:
            assert np.array_equal(out[g, 0:6], np.zeros(6, U)) and out[g, 25] == 0
            assert np.array_equal(out[g, 7:13].view(F), np.array([np.finfo(F).max] * 3 + [-np.finfo(F).max] * 3, dtype=F))
            continue
        lo, hi = mem[:, :3].min(axis=0), mem[:, 3:].max(axis=0)
        assert np.array_equal(out[g, 7:13].view(F), np.concatenate([lo, hi]))
        assert np.array_equal(out[g, 13:19].view(F), np.concatenate([lo - eps, hi + eps]).astype(F))
        d = (hi - lo).astype(np.float64)
        assert abs(float(out[g, 25:26].view(F)[0]) - 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])) < 1e-4
    assert np.array_equal(out[:, 19:25], np.tile(out[3, 7:13], (5, 1)))
    lane32 = ((np.arange(128) + 0xFFFFFFF0) & 0xFFFFFFFF).astype(U)        # wraps inside the first wave
    folds = ref.wave_folds(lane32, (np.arange(128, dtype=np.uint64) << np.uint64(33)) + np.uint64(5))
    wave0 = [(0xFFFFFFF0 + i) & 0xFFFFFFFF for i in range(64)]
    assert folds.shape == (128, 6) and np.array_equal(folds[:64], np.tile(folds[0], (64, 1)))
    assert folds[0].tolist() == [0, 0xFFFFFFFF, sum(wave0) & 0xFFFFFFFF, 0xFFFFFFFF, 5, 0]
    assert folds[64, 4] == 5 and folds[64, 5] == 128
