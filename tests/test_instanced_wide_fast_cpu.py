"""The spec of the FAST wide two-level trace (tests/np_instanced_wide_fast.py) without a device: withheld_wide() at each threshold, one
float on either side, as a lo and as a hi, in a slot of rows 0..2 and in a slot of rows 4..6, in either buffer, in a padding slot and in
the slack slot; the link and count words are never looked at; the flags of a widened pool against np_instanced_fast.withheld of the
binary pool; and the conditions on the inputs the GPU tier reuses (tests/instanced_wide_fast_cases.py), computed from the spec alone, so
that no GPU case passes by never running FAST."""
import numpy as np
import pytest

import instanced_scenes as isc
import instanced_wide_fast_cases as wc
import np_bvh_wide as bw
import np_instanced_fast as nfa
import np_instanced_wide as nw
import np_instanced_wide_fast as nwf
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED
from test_instanced_fast_cpu import THRESHOLDS

F = np.float32
ALL4 = FINITE | FASTDIV | NOTINY | ORDERED
PAIRS = [0, 3, 5, 6, 8, 11]      # of a slot's twelve (lo, hi) pairs: 0..5 are rows 0..2, 6..11 rows 4..6


def pair_word(pair):
    """The word of pair `pair`'s lo in a 128-byte slot."""
    return 2 * pair if pair < 6 else 16 + 2 * (pair - 6)


def _plain_wide():
    """A wide node whose boxes take nothing away: twelve ordered pairs of ordinary magnitude; links and count words nobody tests."""
    w = np.zeros(32, np.uint32)
    w[:12].view(F)[:] = [-1.5, 2.0, -3.0, 0.5, 0.25, 4.0, -2.0, -1.0, 1.0, 8.0, -0.5, 0.0]
    w[16:28].view(F)[:] = [-2.5, 1.0, -1.0, 1.5, 0.5, 2.0, -4.0, -3.0, 2.0, 16.0, -0.25, 0.0]
    w[12:16] = [0xFFFFFFFF, 0x7FC00000, 0xABABABAB, 0x00000001]
    w[28:32] = [0x7F800000, 0x7FC00000, 0xABABABAB, 0xFF800000]
    return w


def _planted(pair, lo, hi, slot=1, slots=3):
    """`slots` plain wide nodes, node `slot` with (lo, hi) as pair `pair` of its twelve."""
    nodes = np.stack([_plain_wide()] * slots)
    k = pair_word(pair)
    nodes[slot, k:k + 2].view(F)[:] = [lo, hi]
    return nodes


@pytest.mark.parametrize("lo,hi,bits", THRESHOLDS)
def test_withheld_wide_thresholds_in_either_buffer_and_either_half_of_a_slot(lo, hi, bits):
    plain = np.stack([_plain_wide()] * 2)
    assert nwf.validate(plain, plain) == (0, 0)
    for pair in PAIRS:
        planted = _planted(pair, lo, hi)
        assert nwf.withheld_wide(planted) == bits, (lo, hi, pair)
        assert nwf.validate(planted, plain) == (bits, 0)
        assert nwf.validate(plain, planted) == (0, bits)
        # the 128-byte slot as two 64-byte slots: rows 3 and 7 are the binary rule's child words
        assert nwf.withheld_wide(planted) == nfa.withheld(planted.reshape(-1, 16))


@pytest.mark.parametrize("lo,hi,bits", THRESHOLDS)
def test_withheld_wide_in_a_padding_slot_and_in_the_slack_slot(lo, hi, bits):
    """A widened pool; the float goes into the box of a padding slot (k >= count, link 0) of a node of count < 4, and into a slot of
    slack appended behind the last wide BLAS."""
    wp = nw.widen_pool(isc.pool_of(["soup64", "nested90"]))
    nodes = wp["nodes"].view(np.uint32).reshape(-1, 32).copy()
    assert nwf.withheld_wide(nodes) == 0
    short = np.flatnonzero(nodes[:, 28] < 4)
    assert short.size
    node = int(short[0])
    k = int(nodes[node, 28])                              # the first padding slot
    assert nodes[node, 12 + k] == 0
    planted = nodes.copy()
    for j, x in ((0, lo), (1, hi)):
        planted[node, bw.WBOX[k][j]] = np.array([x], F).view(np.uint32)[0]
    assert nwf.withheld_wide(planted) == bits, (lo, hi)
    slack = np.zeros(32, np.uint32)
    slack[16:18].view(F)[:] = [lo, hi]
    with_slack = np.concatenate([nodes.reshape(-1), slack])
    # a zero pair beside the planted one is ordered and of no magnitude: only the planted pair speaks
    assert nwf.withheld_wide(with_slack) == bits and nwf.validate(np.zeros(0, np.uint8), with_slack) == (0, bits)


def test_links_counts_empty_buffers_and_the_one_triangle_blas():
    plain = np.stack([_plain_wide()] * 3)
    assert nwf.validate(np.zeros((0, 32), np.uint32), plain) == (0, 0)       # one instance: no top-level node
    n = plain.copy()
    n[:, 12:16] = 0xABABABAB
    n[:, 28:32] = 0xABABABAB
    assert nwf.withheld_wide(n) == 0
    n[:, 12:16] = 0x7FC00000                                                  # NaN as a link or a count: not looked at
    n[:, 28:32] = 0x7F800000
    assert nwf.withheld_wide(n) == 0
    assert nwf.withheld_wide(np.zeros((2, 32), np.uint32)) == 0               # zeroed slack
    one = nw.widen_pool(isc.pool_of(["one"]))["nodes"]
    assert nwf.withheld_wide(one) == FINITE | FASTDIV | ORDERED               # the empty sibling box: lo = FLT_MAX, hi = -FLT_MAX
    assert nwf.validate(plain, nw.widen_pool(isc.pool_of(["soup64", "one"]))["nodes"]) == (0, FINITE | FASTDIV | ORDERED)


@pytest.mark.parametrize("names", [["soup64"], ["soup64", "soup1000", "nested90"], ["soup64", "one"], ["one", "soup1000", "nested90", "one"]])
def test_a_widened_pool_withholds_no_more_than_the_binary_pool(names):
    """Every wide box word is a binary box word: what the wide pool withholds is what the binary nodes withhold, or a subset of it."""
    pool = isc.pool_of(names)
    wide, binary = nwf.withheld_wide(nw.widen_pool(pool)["nodes"]), nfa.withheld(pool["nodes"])
    assert wide & ~binary == 0, (wide, binary)
    assert wide == ((FINITE | FASTDIV | ORDERED) if "one" in names else 0)


# ---- the GPU tier's inputs --------------------------------------------------------------------------------------------------------------
# fastWaveSteps / waveSteps of the wide loop, closest hit and any hit, as a throw-away walk gave them before this spec existed
SHARES = {"all_nice": ((175, 175), (169, 169)), "zero_direction": ((165, 175), None), "object_dir_small": ((170, 200), None),
          "object_dir_large": ((135, 198), None), "object_origin_zero": ((195, 195), None), "object_origin_zero_tiny": ((124, 195), None),
          "pool_withheld": ((9, 175), None), "tlas_withheld": ((109, 175), None), "range_ends": ((170, 175), None), "masks": ((142, 142), None),
          "seeded": ((175, 175), (149, 149)), "identity": ((130, 130), None)}


def _spec(c, any_hit, flags=None):
    tl = c["wide_tlas"]
    flags = nwf.validate(tl[0], c["wide_pool"]) if flags is None else flags
    seed = c["seed"](any_hit) if "seed" in c else None
    return nwf.trace(flags, tl[0], tl[1], tl[2], c["pool"], c["wide_pool"], c["rays"], any_hit, c.get("inst_masks"), c.get("ray_masks"),
                     seed=seed, seed_instance=c.get("seed_instance", -1)), flags


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_gpu_cases_run_the_form_they_are_about(name):
    c = wc.case(name)
    assert c["rays"].shape[0] == 64 * 3 + 17
    for any_hit in (False, True):
        out, flags = _spec(c, any_hit)
        f, cnt = out[6], out[5]
        print(name, any_hit, flags, f, cnt)
        assert f["fastWaveSteps"] <= f["waveSteps"] and f["niceStarts"] <= cnt["numRays"] and f["niceEntries"] <= cnt["numInstanceEntries"]
        if c["expect"] == "all":
            assert f["fastWaveSteps"] == f["waveSteps"] > 0
            assert f["niceEntries"] == cnt["numInstanceEntries"] > 0 or "seed" in c
        elif c["expect"] == "mixed":
            assert 0 < f["fastWaveSteps"] < f["waveSteps"]
        share = SHARES.get(name, (None, None))[any_hit]
        if share is not None:
            assert (f["fastWaveSteps"], f["waveSteps"]) == share
    # what each case is about, from the spec's own numbers (closest hit)
    out, flags = _spec(c, False)
    f, cnt = out[6], out[5]
    if name in ("all_nice", "masks", "seeded", "identity", "object_origin_zero"):
        assert flags == (0, 0) and f["niceStarts"] == 64 * 3 + 17
    if name == "zero_direction":
        assert f["niceStarts"] == 64 * 3 + 17 - 4
    if name in ("object_dir_small", "object_dir_large", "object_origin_zero_tiny"):
        assert flags[1] & FASTDIV == 0 and 0 < f["niceEntries"] < cnt["numInstanceEntries"]
    if name == "object_origin_zero_tiny":
        assert flags == (0, NOTINY)
        assert nwf.withheld_wide(c["wide_pool"][:-128]) == 0              # the slack slot alone withholds it
    if name == "pool_withheld":
        assert flags == (0, FINITE | FASTDIV | ORDERED) and f["niceEntries"] == 0 < cnt["numInstanceEntries"]
    if name == "tlas_withheld":
        assert flags == (FASTDIV, 0) and f["niceStarts"] == 0 < f["niceEntries"]
    if name == "range_ends":
        assert f["niceStarts"] == 64 * 3 + 17 - 4
    if name == "masks":
        assert cnt["numInstancesMasked"] > 0 and cnt["numInstanceEntries"] > 0
    if name == "seeded":
        ids = out[0]
        assert (out[4] == 3).sum() > 10 and ((out[4] >= 0) & (out[4] < 3)).sum() > 10 and (ids == -1).sum() > 10
        assert _spec(c, True)[0][5]["numInstanceEntries"] < cnt["numInstanceEntries"]      # the occluded any-hit rays never start
    if name == "identity":
        assert c["wide_tlas"][1] == -1 and cnt["numTopInnerVisits"] == 0 and cnt["numHits"] > 20


def test_fastdiv_withheld_on_both_levels_never_runs_fast():
    c = wc.case("all_nice")
    for any_hit in (False, True):
        out, _ = _spec(c, any_hit, flags=(FASTDIV, FASTDIV))
        base, _ = _spec(c, any_hit)
        assert out[6] == dict(waveSteps=base[6]["waveSteps"], fastWaveSteps=0, niceStarts=0, niceEntries=0)
        assert out[5] == base[5] and all(np.array_equal(a, b) for a, b in zip(out[:5], base[:5]))
