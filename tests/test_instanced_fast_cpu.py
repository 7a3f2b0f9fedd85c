"""The spec of the FAST two-level trace (tests/np_instanced_fast.py) without a device: validate() at each threshold, one float on either
side, in a top-level node and in a pool node; the spec's records equal np_instanced_masked / np_instanced_seeded; and the conditions on
the inputs the GPU tier reuses (tests/instanced_fast_cases.py), computed from the spec alone, so that no GPU case passes by never
running FAST."""
import numpy as np
import pytest

import instanced_fast_cases as fc
import instanced_scenes as isc
import np_bvh_validate as nv
import np_instanced as ni
import np_instanced_fast as nfa
import np_instanced_masked as nm
import np_instanced_seeded as nsd
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED

F = np.float32
ALL4 = FINITE | FASTDIV | NOTINY | ORDERED


def _plain_node():
    """A node whose boxes take nothing away: six ordered pairs of ordinary magnitude."""
    w = np.zeros(16, np.uint32)
    w[:12].view(F)[:] = [-1.5, 2.0, -3.0, 0.5, 0.25, 4.0, -2.0, -1.0, 1.0, 8.0, -0.5, 0.0]
    w[12:] = [0xFFFFFFFF, 0x7FC00000, 0xABABABAB, 0x00000001]           # words nobody tests
    return w


def _planted(pair, lo, hi):
    """Three plain nodes, the middle one with (lo, hi) as pair `pair` of its six."""
    nodes = np.stack([_plain_node()] * 3)
    nodes[1, :12].view(F)[2 * pair:2 * pair + 2] = [lo, hi]
    return nodes


# (lo, hi, the bits the pair withholds): each threshold with one float on either side, as a lo and as a hi
THRESHOLDS = [
    (-1.0, fc.below(2.0 ** 55), 0), (-1.0, 2.0 ** 55, FASTDIV), (-fc.below(2.0 ** 55), 1.0, 0), (-2.0 ** 55, 1.0, FASTDIV),
    (-1.0, fc.below(2.0 ** 100), FASTDIV), (-1.0, 2.0 ** 100, FASTDIV | FINITE), (-fc.below(2.0 ** 100), 1.0, FASTDIV),
    (-2.0 ** 100, 1.0, FASTDIV | FINITE), (-np.inf, np.inf, FASTDIV | FINITE),
    (2.0 ** -93, 1.0, 0), (fc.below(2.0 ** -93), 1.0, NOTINY), (-1.0, -2.0 ** -93, 0), (-1.0, -fc.below(2.0 ** -93), NOTINY),
    (0.0, 1.0, 0), (-0.0, 1.0, 0), (-1.0, 0.0, 0), (0.0, -0.0, 0), (-0.0, 0.0, 0),
    (np.nan, 1.0, ALL4), (-1.0, np.nan, ALL4),
    (4.0, 4.0, 0), (fc.above(4.0), 4.0, ORDERED), (-4.0, -fc.above(4.0), ORDERED), (2.0 ** -149, 0.0, ORDERED | NOTINY),
]


@pytest.mark.parametrize("lo,hi,bits", THRESHOLDS)
def test_validate_thresholds_in_either_buffer(lo, hi, bits):
    plain = np.stack([_plain_node()] * 2)
    assert nfa.validate(plain, plain) == (0, 0)
    for pair in (0, 3, 5):
        planted = _planted(pair, lo, hi)
        assert nfa.withheld(planted) == bits, (lo, hi, pair)
        assert nfa.validate(planted, plain) == (bits, 0)
        assert nfa.validate(plain, planted) == (0, bits)
        assert nfa.granted(bits) == ALL4 & ~bits
        assert nfa.withheld(planted) == ALL4 & ~nv.expected_flags(planted)      # ntr_bvh_validate's rule, word for word


def test_validate_order_slack_and_the_one_triangle_node():
    plain = np.stack([_plain_node()] * 2)
    assert nfa.validate(np.zeros((0, 16), np.uint32), plain) == (0, 0)          # one instance: no top-level node
    slack = np.concatenate([plain.view(np.uint8).reshape(-1), np.full(64, 0xAB, np.uint8)])
    # 0xABABABAB = -1.2e-12: ordinary magnitude, every pair lo == hi
    assert nfa.validate(plain, slack) == (0, 0)
    zeros = np.concatenate([plain.view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])
    assert nfa.validate(plain, zeros) == (0, 0)          # a zeroed gap
    one = isc.pool_of(["one"])["nodes"]
    assert nfa.withheld(one) == FINITE | FASTDIV | ORDERED                      # the empty sibling box: lo = FLT_MAX, hi = -FLT_MAX
    pool = isc.pool_of(["soup64", "one"], gap_nodes=1)
    assert nfa.validate(plain, pool["nodes"]) == (0, FINITE | FASTDIV | ORDERED)
    assert nfa.withheld(isc.pool_of(["soup64", "soup1000", "nested90"], gap_nodes=2)["nodes"]) == 0
    # the child words are not looked at
    n = plain.copy()
    n[:, 12:] = 0x7FC00000
    assert nfa.withheld(n) == 0


def test_level_nice_at_the_range_ends():
    def nice(w=0, **kw):
        v = dict(ox=1.0, oy=-2.0, oz=3.0, dx=0.5, dy=-0.25, dz=1.0)
        v.update(kw)
        return bool(nfa.level_nice([np.array([v[k]], F) for k in ("ox", "oy", "oz", "dx", "dy", "dz")], w)[0])
    assert nice() and not nice(FASTDIV) and nice(FINITE | ORDERED | NOTINY)
    assert nice(dx=2.0 ** -40) and not nice(dx=fc.below(2.0 ** -40)) and nice(dy=-2.0 ** 20) and not nice(dy=-fc.above(2.0 ** 20))
    assert nice(oz=2.0 ** -36) and not nice(oz=-fc.below(2.0 ** -36)) and nice(ox=fc.below(2.0 ** 55)) and not nice(ox=2.0 ** 55)
    assert nice(ox=0.0) and nice(oy=-0.0) and not nice(NOTINY, ox=0.0) and not nice(NOTINY, oy=-0.0)
    assert not nice(dz=0.0) and not nice(dz=np.nan) and not nice(ox=np.nan) and not nice(dx=np.inf) and not nice(oy=np.inf)


# ---- the records are the masked / seeded spec's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_records_equal_the_masked_and_the_seeded_spec(name):
    sc = isc.scene(name)
    pool = isc.pool_of(sc["names"])
    inst = ni.instances(sc["transforms"], sc["blas"])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    rays = np.concatenate([isc.scene_rays()[11::97], isc.odd_rays()[::9]])
    flags = nfa.validate(t["nodes"], pool["nodes"])
    assert flags == (0, 0)
    n = inst.shape[0]
    inst_masks = np.where(np.arange(n) % 2 == 0, 0x80000001, 0x2).astype(np.uint32)
    seed = nsd.seed_of(np.where(np.arange(rays.shape[0]) % 2 == 0, -1, 5), F(30.0), 1, 2)
    for any_hit in (False, True):
        for kw in (dict(), dict(inst_masks=inst_masks, ray_mask=0x3)):
            want = nm.trace(t["nodes"], t["root_link"], t["records"], pool, rays, any_hit, **kw)
            got = nfa.trace(flags, t["nodes"], t["root_link"], t["records"], pool, rays, any_hit, **kw)
            for g, w in zip(got[:5], want[:5]):
                assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
            assert got[5] == want[5] and 0 < got[6]["fastWaveSteps"] <= got[6]["waveSteps"]
            want = nsd.trace(seed, n, t["nodes"], t["root_link"], t["records"], pool, rays, any_hit, **kw)
            got = nfa.trace(flags, t["nodes"], t["root_link"], t["records"], pool, rays, any_hit, seed=seed, seed_instance=n, **kw)
            for g, w in zip(got[:5], want[:5]):
                assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
            assert got[5] == want[5]


# ---- the GPU tier's inputs --------------------------------------------------------------------------------------------------------------
def _spec(c, any_hit, flags=None):
    tl = c["tlas"]
    flags = nfa.validate(tl[0], c["pool"]["nodes"]) if flags is None else flags
    seed = c["seed"](any_hit) if "seed" in c else None
    return nfa.trace(flags, tl[0], tl[1], tl[2], c["pool"], c["rays"], any_hit, c.get("inst_masks"), c.get("ray_masks"), seed=seed,
                     seed_instance=c.get("seed_instance", -1)), flags


@pytest.mark.parametrize("name", fc.NAMES)
def test_the_gpu_cases_run_the_form_they_are_about(name):
    c = fc.case(name)
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
        assert c["tlas"][1] == -1 and cnt["numTopInnerVisits"] == 0 and cnt["numHits"] > 20


def test_fastdiv_withheld_on_both_levels_never_runs_fast():
    c = fc.case("all_nice")
    for any_hit in (False, True):
        out, _ = _spec(c, any_hit, flags=(FASTDIV, FASTDIV))
        base, _ = _spec(c, any_hit)
        assert out[6] == dict(waveSteps=base[6]["waveSteps"], fastWaveSteps=0, niceStarts=0, niceEntries=0)
        assert out[5] == base[5] and all(np.array_equal(a, b) for a, b in zip(out[:5], base[:5]))
