"""The shared device toolkit on the GPU, called directly with inputs chosen here (ntr_selftest_onesweep / _scan / _scan_block_sums /
_float_order / _box_words run the production templates of radix_sort.h and device_prims.h as they stand) against the plain numpy
references of np_device_prims.py.  Every comparison is exact, on integer views; every sort's error word is asserted zero.

* The one-sweep pass in each instantiation a builder or the ray sort launches, at the sizes around a 64-key round and a tile (ragged
  last tile, one tile more, 41 tiles), with the ticket forced on and off -- unforced, these grids are resident, so both paths must give
  the same bytes -- over key sets that choose the digit distribution: uniform, all equal (stability), digit 255 (a ragged tile's padding
  digit), one digit holding all but three keys (first, last, at a tile seam), sorted, reversed, two digits alternating per lane.
  MODE 1 has no caller any more and is not offered.
* The three-launch scan and scan_block_sums alone at the workgroup seams and across the carry loop (more than THREADS block sums), for
  every value type in use, with sums that wrap.
* ord_enc and its kin on the zeros, the denormal and normal ends, the infinities and NaNs of both signs, and all pairs through ord_min /
  ord_max in both operand orders.
* Boxes merged per lane and through wave_grouped_atomic for the wave shapes that take each of its branches, decoded by words_box and
  words_area; the wave folds."""
import numpy as np
import pytest

import ntrace_amd as nt
import np_device_prims as ref

U = np.uint32
I = np.int32
F = np.float32
gpu = pytest.mark.gpu
PASSES4 = [(0, 0), (8, 1), (16, 2), (24, 3)]
MODE0 = [c for c in nt.ONESWEEP_COMBOS if c[1] == 0]
MODE2 = [c for c in nt.ONESWEEP_COMBOS if c[1] == 2]


def tile_of(combo):
    return 256 * combo[0]


def sizes(combo):
    t = tile_of(combo)
    return (1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 1, 40 * t + 777)


def up(a):
    from gpu_util import up as _up
    return _up(a)


def blank(nbytes):
    import torch
    return torch.full((max(int(nbytes), 16),), 0xCD, dtype=torch.uint8, device="cuda:0")


def down(t, dtype, nbytes):
    return t.cpu().numpy()[:nbytes].view(dtype)


def rand_words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U)


def combo_id(c):
    return "items%d-mode%d-%s" % (c[0], c[1], "skip" if c[2] else "rank")


def combo_sizes(combos):
    return [pytest.param(c, n, id="%s-n%d" % (combo_id(c), n)) for c in combos for n in sizes(c)]


# ---- the one-sweep sort ---------------------------------------------------------------------------------------------------------------
def device_sort(combo, n, keys_ptr, stride, vals_ptr, passes, force):
    """(keys, values) of the last pass; the error word must be zero"""
    out_k, out_v = blank(n * 4), blank(n * 4)
    err = nt.selftest_onesweep(combo[0], combo[1], combo[2], n, keys_ptr, stride, vals_ptr, passes, force, out_k.data_ptr(), out_v.data_ptr())
    assert err == 0, "error word 0x%x" % err
    return down(out_k, U, n * 4), down(out_v, I, n * 4)


def assert_sorted(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: keys differ first at %d" % (what, int(np.nonzero(got[0] != want[0])[0][0]))
    assert np.array_equal(got[1], want[1]), "%s: values differ first at %d" % (what, int(np.nonzero(got[1] != want[1])[0][0]))


def key_sets(n, tile, rng):
    rnd = rand_words(rng, n)
    i = np.arange(n)
    skew = np.full(n, 0x55555555, dtype=U)           # one digit in every byte, but for three keys: first, at a tile seam, last
    skew[tile if n > tile else n // 2] = 0x80FE017F
    skew[0] = 0x01020304
    skew[n - 1] = 0xFEFDFCFB
    return {"uniform": rnd,
            "all equal": np.full(n, 0x9E3779B9, dtype=U),
            "digit 255 in the low byte": rnd | U(0xFF),
            "digit 255 in every byte": np.full(n, 0xFFFFFFFF, dtype=U),
            "one digit but three keys": skew,
            "sorted": np.sort(rnd),
            "reversed": np.sort(rnd)[::-1].copy(),
            "two digits alternating": np.where(i & 1, U(0xA1A1A1A1), U(0x3C3C3C3C)).astype(U)}


@gpu
@pytest.mark.parametrize("combo,n", combo_sizes(MODE0))
def test_onesweep_mode0_four_passes_every_key_set_both_paths(combo, n):
    """4 passes over shifts 0, 8, 16, 24 with consecutive pass numbers on one clearing of the tile state; the first pass with the values
    null (the value is the index) and given; every call after the first is a further sort on the same, freshly cleared state."""
    rng = np.random.default_rng(n * 31 + combo[0] + 2 * combo[2])
    vals = rng.integers(-(1 << 31), 1 << 31, n).astype(I)
    d_vals = up(vals)
    for name, keys in key_sets(n, tile_of(combo), rng).items():
        d_keys = up(keys)
        order = ref.sort_order(keys, PASSES4)
        assert np.array_equal(order, np.argsort(keys, kind="stable"))
        if name == "all equal":
            assert np.array_equal(order, np.arange(n))
        for given in (False, True):
            want = (keys[order], vals[order] if given else order.astype(I))
            got = {}
            for force in (0, 1):
                got[force] = device_sort(combo, n, d_keys.data_ptr(), 1, d_vals.data_ptr() if given else 0, PASSES4, force)
                assert_sorted(got[force], want, "%s, values %s, ticket %s" % (name, "given" if given else "null", "forced" if force else "as launched"))
            assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


class Mode2Input:
    """two key words per element behind a value: word w of element v at key_arrays[w][v * stride + offset[w]]"""

    def __init__(self, n, stride, words, vals):
        self.n, self.stride, self.vals = n, stride, vals
        if stride == 6:      # one 6-word key per element, as the ray sort's: the two words are words 1 and 0 of it
            flat = np.zeros((n, 6), dtype=U)
            flat[:, 1], flat[:, 0] = words[0], words[1]
            flat[:, 2:] = 0xDEADBEEF
            self.flat = [flat.reshape(-1)] * 2
            self.word = [1, 0]
            d = up(flat)
            self.dev = [d, d]
        else:                # dense words, as the batched PLOC build's mesh index
            self.flat = [np.ascontiguousarray(words[0]), np.ascontiguousarray(words[1])]
            self.word = [0, 0]
            self.dev = [up(self.flat[0]), up(self.flat[1])]
        self.d_vals = up(vals)

    def ptr(self, w):
        return self.dev[w].data_ptr() + 4 * self.word[w]


def chain_two_words(combo, inp, pass_lists, force):
    """MODE 2 then MODE 0 over the first word, then the same over the second word with the values the first sort left"""
    import torch
    n = inp.n
    k1, v1 = device_sort(combo, n, inp.ptr(0), inp.stride, inp.d_vals.data_ptr(), pass_lists[0], force)
    d_v1 = torch.from_numpy(v1.copy()).to("cuda:0")
    k2, v2 = device_sort(combo, n, inp.ptr(1), inp.stride, d_v1.data_ptr(), pass_lists[1], force)
    return (k1, v1), (k2, v2)


def chain_reference(inp, pass_lists):
    w1 = ref.sort_mode2(inp.flat[0], inp.word[0], inp.stride, inp.vals, pass_lists[0])
    w2 = ref.sort_mode2(inp.flat[1], inp.word[1], inp.stride, w1[1], pass_lists[1])
    return w1, w2


def mode2_words(n, rng):
    """uniform words; and words whose bytes 1 and 3 are the same in every key (passes the SKIP_TRIVIAL instantiations only copy)"""
    const = lambda w: (w & U(0x00FF00FF)) | U(0x5A00A500)
    return {"uniform": (rand_words(rng, n), rand_words(rng, n)),
            "constant bytes 1 and 3": (const(rand_words(rng, n)), const(rand_words(rng, n))),
            "first word constant": (np.full(n, 0x00FF00FF, dtype=U), rand_words(rng, n) & U(0xFF))}


@gpu
@pytest.mark.parametrize("combo,n", combo_sizes(MODE2))
def test_onesweep_mode2_then_mode0_over_two_words(combo, n):
    """As rayops_kernels.hip chains them (stride 6) and bvh_ploc_batch_kernels.hip (stride 1): the first pass over a word fetches it
    through the values, the other three run on the dense pairs; the second word's sort starts from the values of the first.  The result
    is one stable sort by (second word, first word), on both paths."""
    rng = np.random.default_rng(n * 17 + combo[2])
    lists = ([(0, 0), (8, 1), (16, 2), (24, 3)], [(0, 4), (8, 5), (16, 6), (24, 7)])
    for name, words in mode2_words(n, rng).items():
        vals = rng.permutation(n).astype(I)
        if n > 2:
            vals[n // 2] = vals[0]                      # a value may occur twice: the sort moves values, it does not need a permutation
        for stride in (1, 6):
            inp = Mode2Input(n, stride, words, vals)
            want = chain_reference(inp, lists)
            wide = (words[1][vals].astype(np.uint64) << np.uint64(32)) | words[0][vals].astype(np.uint64)
            assert np.array_equal(want[1][1], vals[np.argsort(wide, kind="stable")])
            got = {}
            for force in (0, 1):
                got[force] = chain_two_words(combo, inp, lists, force)
                for w in (0, 1):
                    assert_sorted(got[force][w], want[w], "%s, stride %d, word %d, ticket %s" % (name, stride, w, "forced" if force else "as launched"))
            assert all(got[0][w][j].tobytes() == got[1][w][j].tobytes() for w in (0, 1) for j in (0, 1))


@gpu
@pytest.mark.parametrize("n", sizes((8, 0, True)))
def test_onesweep_skip_trivial_passes_only_copy(n):
    """A pass whose digit is the same in every key is the identity: the SKIP_TRIVIAL instantiations take their copy path (MODE 2: fetch
    and copy).  Compared with the reference and with the same sort through the instantiations that rank every pass."""
    rng = np.random.default_rng(n + 5)
    keys = (rand_words(rng, n) & U(0x00FF00FF)) | U(0x5A00A500)       # bytes 1 and 3 constant
    vals = rng.integers(-(1 << 31), 1 << 31, n).astype(I)
    perm = rng.permutation(n).astype(I)
    d_keys, d_vals, d_perm = up(keys), up(vals), up(perm)
    mode0_lists = (PASSES4,                                   # trivial passes between ranked ones
                   [(8, 0), (0, 1)],                          # a trivial first pass (values null: the copy numbers the keys)
                   [(24, 5)], [(8, 9), (24, 10)],             # nothing but copies
                   [(16, 0), (24, 1), (8, 2), (0, 3)])        # another pass order
    for passes in mode0_lists:
        for given in (False, True):
            want = ref.sort_mode0(keys, vals if given else None, passes)
            for force in (0, 1):
                got = device_sort((8, 0, True), n, d_keys.data_ptr(), 1, d_vals.data_ptr() if given else 0, passes, force)
                ranked = device_sort((8, 0, False), n, d_keys.data_ptr(), 1, d_vals.data_ptr() if given else 0, passes, force)
                assert_sorted(got, want, "mode 0 %r values %s ticket %d" % (passes, given, force))
                assert_sorted(ranked, want, "mode 0 ranked %r values %s ticket %d" % (passes, given, force))
    mode2_lists = ([(8, 0)], [(24, 3)],                       # the fetch-and-copy path alone
                   [(24, 0), (0, 1), (8, 2), (16, 3)],        # ... followed by ranked and copied MODE 0 passes
                   PASSES4)
    for stride in (1, 6):
        flat = np.full((n, stride), 0xDEADBEEF, dtype=U)
        flat[:, stride - 1] = keys
        d_flat = up(flat)
        for passes in mode2_lists:
            want = ref.sort_mode2(flat.reshape(-1), stride - 1, stride, perm, passes)
            for force in (0, 1):
                got = device_sort((8, 2, True), n, d_flat.data_ptr() + 4 * (stride - 1), stride, d_perm.data_ptr(), passes, force)
                ranked = device_sort((8, 2, False), n, d_flat.data_ptr() + 4 * (stride - 1), stride, d_perm.data_ptr(), passes, force)
                assert_sorted(got, want, "mode 2 %r stride %d ticket %d" % (passes, stride, force))
                assert_sorted(ranked, want, "mode 2 ranked %r stride %d ticket %d" % (passes, stride, force))


@gpu
@pytest.mark.parametrize("combo", nt.ONESWEEP_COMBOS, ids=combo_id)
def test_onesweep_pass_numbers_and_a_second_sort_on_the_same_state(combo):
    """Pass numbers 0 and OS_MAX_PASSES - 1 (the status bits' ends), consecutive and scattered numbers on one clearing, and a second sort
    of other keys with the same pass numbers on the same state words after a fresh clear: no word of an earlier pass or sort is taken
    for one of this pass."""
    last = nt.ONESWEEP_MAX_PASS
    n = 3 * tile_of(combo) + 1
    rng = np.random.default_rng(combo[0] * 7 + combo[1] + combo[2])
    lists = ([(8, 0)], [(8, last)], [(0, last - 3), (8, last - 2), (16, last - 1), (24, last)], [(0, 7), (8, 3), (16, 99), (24, 0)],
             [(0, 5), (0, 6)], PASSES4, PASSES4)
    for passes in lists:
        keys = rand_words(rng, n) & U(0x3F0F3F0F)             # few digit values: long runs per digit in every tile
        if combo[1] == 0:
            d_keys = up(keys)
            want = ref.sort_mode0(keys, None, passes)
            run = lambda force: device_sort(combo, n, d_keys.data_ptr(), 1, 0, passes, force)
        else:
            perm = rng.permutation(n).astype(I)
            d_keys, d_perm = up(keys), up(perm)
            want = ref.sort_mode2(keys, 0, 1, perm, passes)
            run = lambda force: device_sort(combo, n, d_keys.data_ptr(), 1, d_perm.data_ptr(), passes, force)
        for force in (0, 1):
            assert_sorted(run(force), want, "%r ticket %d" % (passes, force))


@gpu
def test_onesweep_refuses_a_value_outside_the_keys():
    """MODE 2 follows its values into the key array: one outside [0, n) is refused before any pass runs"""
    n = 1000
    keys = np.arange(n, dtype=U)
    for bad in (-1, n, 1 << 30):
        vals = np.arange(n, dtype=I)
        vals[n // 2] = bad
        d_keys, d_vals = up(keys), up(vals)
        with pytest.raises(nt.NtrError) as e:
            device_sort((8, 2, False), n, d_keys.data_ptr(), 1, d_vals.data_ptr(), [(0, 0)], 0)
        assert e.value.code == -1


# ---- scans -----------------------------------------------------------------------------------------------------------------------------
SCAN_TYPES = {nt.SCAN_U32: ("u32", U, 32, 1), nt.SCAN_I32: ("i32", I, 32, 1), nt.SCAN_U64: ("u64", np.uint64, 64, 1), nt.SCAN_U4: ("U4", U, 32, 4)}


def scan_inputs(stype, n, threads, rng):
    """all ones, all zero, random values whose sums wrap (int: both signs, no overflow), one non-zero item at each seam"""
    _, dt, bits, width = SCAN_TYPES[stype]
    shape = (n, 4) if width == 4 else (n,)
    out = {"ones": np.ones(shape, dtype=dt), "zeros": np.zeros(shape, dtype=dt)}
    if stype == nt.SCAN_I32:
        out["random"] = rng.integers(-1000, 1001, shape).astype(dt)
    elif bits == 64:
        out["random"] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    else:
        out["random"] = rand_words(rng, shape)        # U4: four independent streams
    for seam in sorted({0, threads - 1, threads, threads + 1, threads * threads - 1, threads * threads, n - 1}):
        if 0 <= seam < n:
            a = np.zeros(shape, dtype=dt)
            a[seam] = (1, 2, 3, 0xFFFFFFFF) if width == 4 else 7
            out["one item at %d" % seam] = a
    return out


def scan_reference(stype, a):
    _, dt, bits, width = SCAN_TYPES[stype]
    unsigned = a.view(U) if dt is I else a
    ex, tot = ref.exclusive_scan(unsigned, bits)
    return ex, np.atleast_1d(tot)


def scan_cases():
    out = []
    for stype, (name, _, _, _) in SCAN_TYPES.items():
        for n in (1, 255, 256, 257, 256 * 256, 256 * 256 + 1):
            out.append(pytest.param(stype, 256, n, id="%s-256-n%d" % (name, n)))
        for n in (1, 1023, 1024, 1025):                       # (the seams above the block sums: the block-sum form below)
            out.append(pytest.param(stype, 1024, n, id="%s-1024-n%d" % (name, n)))
    return out


@gpu
@pytest.mark.parametrize("stype,threads,n", scan_cases())
def test_three_launch_scan(stype, threads, n):
    _, dt, bits, width = SCAN_TYPES[stype]
    item = np.dtype(dt).itemsize * width
    rng = np.random.default_rng(n + threads + stype)
    for name, a in scan_inputs(stype, n, threads, rng).items():
        want_ex, want_tot = scan_reference(stype, a)
        if name == "random" and n > 256 and stype != nt.SCAN_I32:
            assert int(np.asarray(want_tot).reshape(-1)[0]) != int(a.reshape(n, -1)[:, 0].astype(object).sum()), "the sums must wrap"
        d_in, d_out = up(a), blank(n * item)
        total = nt.selftest_scan(stype, threads, n, d_in.data_ptr(), d_out.data_ptr())
        got = down(d_out, want_ex.dtype, n * item).reshape(want_ex.shape)
        assert np.array_equal(got, want_ex), "%s: prefix differs first at item %d" % (name, int(np.nonzero(got != want_ex)[0][0]))
        assert np.array_equal(np.frombuffer(total, dtype=want_ex.dtype), want_tot.reshape(-1)), name
        assert np.array_equal(down(d_in, a.dtype, n * item).reshape(a.shape), a)


@gpu
@pytest.mark.parametrize("threads", (256, 1024))
@pytest.mark.parametrize("stype", list(SCAN_TYPES), ids=[v[0] for v in SCAN_TYPES.values()])
def test_scan_block_sums_alone_in_place_and_apart_with_and_without_total(stype, threads):
    """nb = THREADS + 1 and 3 * THREADS + 5 take the carry loop; nb = 0 writes nothing but a zero total"""
    _, dt, bits, width = SCAN_TYPES[stype]
    item = np.dtype(dt).itemsize * width
    for nb in (0, 1, threads, threads + 1, 3 * threads + 5):
        rng = np.random.default_rng(nb + threads + stype)
        inputs = scan_inputs(stype, nb, threads, rng) if nb else {"nothing": np.zeros((0, 4) if width == 4 else (0,), dtype=dt)}
        for name, a in inputs.items():
            want_ex, want_tot = scan_reference(stype, a)
            for in_place in (False, True):
                for want_total in (True, False):
                    d_in = up(a) if nb else blank(16)
                    d_out = d_in if in_place else blank(nb * item + 16)
                    total = nt.selftest_scan_block_sums(stype, threads, nb, d_in.data_ptr(), d_out.data_ptr(), want_total)
                    what = "%s nb %d in place %s total %s" % (name, nb, in_place, want_total)
                    got = down(d_out, want_ex.dtype, nb * item).reshape(want_ex.shape)
                    assert np.array_equal(got, want_ex), what
                    if want_total:
                        assert np.array_equal(np.frombuffer(total, dtype=want_ex.dtype), want_tot.reshape(-1)), what
                    else:
                        assert total is None
                    if not in_place:
                        assert np.array_equal(down(d_in, a.dtype, nb * item).reshape(a.shape), a), what
                        assert (d_out.cpu().numpy()[nb * item:] == 0xCD).all(), "%s: a write past the last sum" % what


# ---- the floats' total order -----------------------------------------------------------------------------------------------------------
@gpu
def test_float_order_encodings_and_min_max_of_all_pairs():
    words = ref.float_word_set()
    n = words.shape[0]
    assert n == 224
    d_words, d_single, d_pairs = up(words), blank(n * 6 * 4), blank(n * n * 2 * 4)
    nt.selftest_float_order(n, d_words.data_ptr(), d_single.data_ptr(), d_pairs.data_ptr())
    single = down(d_single, U, n * 6 * 4).reshape(n, 6)
    want = ref.float_order_single(words)
    for col, what in enumerate(("ord_enc", "ord_dec(ord_enc)", "ord_enc_int", "ord_dec_int(ord_enc_int)", "ord_to_int", "ord_from_int(ord_to_int)")):
        bad = np.nonzero(single[:, col] != want[:, col])[0]
        assert bad.size == 0, "%s of 0x%08x: 0x%08x, expected 0x%08x" % (what, words[bad[0]], single[bad[0], col], want[bad[0], col])
    pairs = down(d_pairs, U, n * n * 2 * 4).reshape(n, n, 2)
    want_pairs = ref.float_order_pairs(words)
    for k, what in enumerate(("ord_min", "ord_max")):
        bad = np.argwhere(pairs[:, :, k] != want_pairs[:, :, k])
        assert bad.shape[0] == 0, "%s(0x%08x, 0x%08x) = 0x%08x, expected 0x%08x" % (
            what, words[bad[0][0]], words[bad[0][1]], pairs[bad[0][0], bad[0][1], k], want_pairs[bad[0][0], bad[0][1], k])
        assert np.array_equal(pairs[:, :, k], pairs[:, :, k].T), "%s depends on the order of its operands" % what


# ---- boxes and wave folds ------------------------------------------------------------------------------------------------------------------
def box_case():
    """nine waves in three workgroups; groups 0 .. 72, of which 71 receives nothing"""
    rng = np.random.default_rng(11)
    waves = 9
    m = 64 * waves
    a, b = rng.normal(size=(m, 3)).astype(F), rng.normal(size=(m, 3)).astype(F)
    boxes = np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1)
    group = np.zeros(m, dtype=I)
    lane = np.arange(64)
    group[0:64] = 0                                           # all lanes in one group (the uniform branch)
    group[64:128] = -1                                        # all lanes none (uniform, nothing written)
    group[128:192] = np.where(lane == 17, 2, 1)               # one lane differing
    group[192:256] = np.where(lane < 32, 3, 4)                # a group change at lane 32
    group[256:320] = 5 + lane                                 # 64 distinct groups (5 .. 68)
    group[320:384] = np.where(lane == 0, -1, 69)              # lane 0 none, the rest one group: the uniform branch's writer is lane 0
    group[384:448] = np.where(lane == 0, 70, -1)              # ... and the other way round
    group[448:512] = 0                                        # a second wave (another workgroup) into group 0
    group[512:576] = np.where(lane == 63, -1, 72)             # the last lane none
    neg0, pos0 = F(-0.0), F(0.0)
    boxes[192:224, 0] = np.where(lane[:32] & 1, neg0, pos0)   # group 3: min x among -0 / +0 only -> -0; max x likewise -> +0
    boxes[192:224, 3] = np.where(lane[:32] & 2, neg0, pos0)
    boxes[145] = (3.0, 2.0, 1.0, -3.0, -2.0, -1.0)            # group 2 (lane 17 of wave 2): an inverted box, alone in its group
    boxes[230, 0], boxes[231, 5] = -np.inf, np.inf            # group 4: infinite corners (area +inf)
    lane32 = rand_words(rng, m)
    lane32[64:128] = 0x80000000                               # a wave of equal words whose sum wraps to 0
    lane32[128:192] |= U(0xFFFF0000)                          # sums that wrap
    lane64 = rng.integers(0, 1 << 64, m, dtype=np.uint64)
    lane64[64:128] = (lane64[64:128] & np.uint64(0xFFFFFFFF)) | np.uint64(0x7 << 32)     # equal high words: the low word decides
    lane64[128:192] = (lane64[128:192] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(9)   # equal low words
    lane64[200] = 0
    return m, boxes, group, 73, F(1e-3), lane32, lane64


@gpu
def test_boxes_merged_per_lane_and_by_wave_groups_and_the_wave_folds():
    m, boxes, group, groups, eps, lane32, lane64 = box_case()
    want = ref.box_groups(boxes, group, groups, eps)
    flt_max = np.finfo(F).max
    assert want[71, 6] == 0 and want[71, 25] == 0 and np.array_equal(want[71, 7:13].view(F), np.array([flt_max] * 3 + [-flt_max] * 3, dtype=F))
    assert want[3, 7] == 0x80000000 and want[3, 10] == 0 and want[2, 25] == 0 and want[4, 25:26].view(F)[0] == np.inf
    lo = boxes[group == 0][:, :3].min(axis=0)
    assert np.array_equal(want[0, 13:16].view(F), (lo - eps).astype(F))          # the grown corner is fl(min - eps)
    d_out, d_folds = blank(2 * groups * ref.BOX_OUT_WORDS * 4), blank(m * 6 * 4)
    d_boxes, d_group, d_l32, d_l64 = up(boxes), up(group), up(lane32), up(lane64)
    nt.selftest_box_words(m, d_boxes.data_ptr(), d_group.data_ptr(), groups, eps, d_l32.data_ptr(), d_l64.data_ptr(), d_out.data_ptr(), d_folds.data_ptr())
    got = down(d_out, U, 2 * groups * ref.BOX_OUT_WORDS * 4).reshape(2, groups, ref.BOX_OUT_WORDS)
    for path, what in enumerate(("atomic_max_box per lane", "wave_grouped_atomic")):
        bad = np.argwhere(got[path] != want)
        assert bad.shape[0] == 0, "%s: group %d word %d is 0x%08x, expected 0x%08x" % (
            what, bad[0][0], bad[0][1], got[path][bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]])
    folds = down(d_folds, U, m * 6 * 4).reshape(m, 6)
    want_folds = ref.wave_folds(lane32, lane64)
    assert want_folds[64, 2] == 0
    bad = np.argwhere(folds != want_folds)
    assert bad.shape[0] == 0, "lane %d fold %d is 0x%08x, expected 0x%08x" % (bad[0][0], bad[0][1], folds[bad[0][0], bad[0][1]], want_folds[bad[0][0], bad[0][1]])
    # a group outside [-1, groups) is refused, not followed
    group[5] = groups
    d_group = up(group)
    with pytest.raises(nt.NtrError) as e:
        nt.selftest_box_words(m, d_boxes.data_ptr(), d_group.data_ptr(), groups, eps, d_l32.data_ptr(), d_l64.data_ptr(), d_out.data_ptr(), d_folds.data_ptr())
    assert e.value.code == -1
