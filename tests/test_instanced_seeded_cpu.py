"""The seeded two-level trace without a device: the spec tests/np_instanced_seeded.py on a static world plus 32 small instances
(seeded_scenes.world_scene) against the unseeded spec over the same scene with the world as one more identity instance, against a
binary64 brute force with test_instanced_cpu.py's yardstick, with seeds that are all misses and all hits, with masks, in its counters,
and in its wide form."""
import numpy as np
import pytest

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_instanced as ni
import np_instanced_masked as nm
import np_instanced_seeded as nsd
import np_instanced_wide as nw
import np_tracer
import seeded_scenes as sds

F = np.float32
ALL = 0xFFFFFFFF
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _seeded(any_hit, seed=None, seed_instance=None, **kw):
    sc, r = sds.world_scene(), sds.rays()
    t = sc["tlas"]
    seed = sds.world_seed(sc, r, any_hit) if seed is None else seed
    return nsd.trace(seed, sc["inst"].shape[0] if seed_instance is None else seed_instance, t["nodes"], t["root_link"], t["records"], sc["pool"], r,
                     any_hit, **kw)


def _unseeded_all(any_hit, **kw):
    """np_instanced_masked.trace over the N + 1 instances, the world being identity instance N: computed once per mode and shared."""
    key = ("all", any_hit, tuple(sorted(kw)))
    if kw or key not in _cache:
        sc, r = sds.world_scene(), sds.rays()
        t = sc["tlas_all"]
        out = nm.trace(t["nodes"], t["root_link"], t["records"], sc["pool"], r, any_hit, **kw)
        if kw:
            return out
        _cache[key] = out
    return _cache[key]


def _fetches(c):
    return (c["numTopInnerVisits"] + c["numInstanceEntries"] + c["numInnerVisits"]) / c["numRays"]


def test_closest_hit_equals_the_unseeded_trace_with_the_world_as_an_instance():
    sc = sds.world_scene()
    n = sc["inst"].shape[0]
    assert n == 32 and sc["tlas"]["root_link"] == 0
    a, b = _seeded(False), _unseeded_all(False)
    differ = (a[0] != b[0]) | (_bits(a[1]) != _bits(b[1])) | (a[4] != b[4])
    print("closest hit: %d of %d rays differ in (id, t bits, instance)" % (int(differ.sum()), differ.size))
    assert not differ.any()
    real = (a[4] >= 0) & (a[4] < n)                  # the world's u, v are not compared: the single-level spec does not produce them
    assert real.sum() > 100 and (a[4] == n).sum() > 100 and (a[4] == -1).sum() > 100
    assert np.array_equal(_bits(a[2])[real], _bits(b[2])[real]) and np.array_equal(_bits(a[3])[real], _bits(b[3])[real])
    assert (_bits(a[2])[a[4] == n] == 0).all() and (_bits(a[3])[a[4] == n] == 0).all()      # the seed's w2 = w3 = 0, verbatim


def test_any_hit_equals_the_unseeded_trace_in_hit_or_miss():
    a, b = _seeded(True), _unseeded_all(True)
    differ = (a[0] != -1) != (b[0] != -1)
    print("any hit: %d of %d rays differ in hit or miss; %d hold another hit" % (int(differ.sum()), differ.size, int((a[0] != b[0]).sum())))
    assert not differ.any() and (a[0] != -1).sum() > 500
    n = sds.world_scene()["inst"].shape[0]
    seed = sds.world_seed(sds.world_scene(), sds.rays(), True)
    occluded = seed[:, 0].view(np.int32) != -1       # the world occludes: the seed stays, word for word
    assert np.array_equal(np.stack([_bits(x) for x in a[:4]], axis=1)[occluded], seed[occluded]) and (a[4][occluded] == n).all()


def test_closest_hit_against_binary64_brute_force():
    """test_instanced_cpu.py::test_spec_against_binary64_brute_force's yardstick: the single-level np_tracer on the flattened mesh of the
    N + 1 instances against the same brute force.  The seeded trace, binary and wide, may disagree on at most twice that count of bad
    rays plus four, at four times that largest relative t error."""
    sc, r = sds.world_scene(), sds.rays()
    verts, _ = isc.flatten(dict(names=sc["names"], transforms=sc["inst_all"]["objectToWorld"], blas=sc["inst_all"]["blas"]))
    hit_b, t_b = isc.brute_force(verts, r)
    pos32 = verts.reshape(-1, 3).astype(F)
    tri = np.arange(pos32.shape[0], dtype=np.int32).reshape(-1, 3)
    flat = pl.build(tri, pos32, *pl.scene_box(pos32), 8)
    fid, ft = np_tracer.trace(flat["nodes"], flat["woop"], flat["tri_index"], r)

    def against_brute(hit, tt, tol):
        both = hit & hit_b
        rel = np.abs(tt[both].astype(np.float64) - t_b[both]) / np.abs(t_b[both])
        status = int((hit != hit_b).sum())
        return status, (float(rel.max()) if rel.size else 0.0), status + (int((rel > tol).sum()) if tol is not None else 0)

    f_status, f_err, f_bad = against_brute(fid >= 0, ft, None)
    assert hit_b.sum() > r.shape[0] // 8
    for what, out in (("binary", _seeded(False)), ("wide", _wide_seeded(False))):
        s_status, s_err, s_bad = against_brute(out[0] != -1, out[1], 4.0 * f_err)
        print("%s seeded spec: %d status mismatches, largest relative t error %.3g, %d rays beyond %.3g; flat tracer: %d, %.3g"
              % (what, s_status, s_err, s_bad - s_status, 4.0 * f_err, f_status, f_err))
        assert s_bad <= 2 * f_bad + 4, (what, s_bad, f_bad)


@pytest.mark.parametrize("any_hit", [False, True])
def test_an_all_miss_seed_reproduces_the_unseeded_trace(any_hit):
    sc, r = sds.world_scene(), sds.rays()
    t = sc["tlas"]
    a = _seeded(any_hit, seed=sds.miss_seed(r), seed_instance=77)
    b = nm.trace(t["nodes"], t["root_link"], t["records"], sc["pool"], r, any_hit)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(_bits(x), _bits(y))
    assert a[5] == b[5] and a[5]["numHits"] > 100
    assert nsd.algorithmic_bytes(a[5]) == nm.algorithmic_bytes(b[5]) + 16 * r.shape[0]


@pytest.mark.parametrize("any_hit", [False, True])
def test_an_all_hit_seed_at_the_smallest_t_stays(any_hit):
    r = sds.rays()
    rng = np.random.default_rng(4)
    seed = nsd.seed_of(rng.integers(0, 1000, r.shape[0]), np.nextafter(r["tmin"].astype(F), F(np.inf)),
                       rng.integers(0, 2 ** 32, r.shape[0], dtype=np.uint64).astype(np.uint32),
                       rng.integers(0, 2 ** 32, r.shape[0], dtype=np.uint64).astype(np.uint32))
    a = _seeded(any_hit, seed=seed, seed_instance=-2)
    assert np.array_equal(np.stack([_bits(x) for x in a[:4]], axis=1), seed)          # no t lies between tmin and its successor
    assert (a[4] == -2).all() and a[5]["numHits"] == r.shape[0]
    if any_hit:
        assert all(a[5][k] == 0 for k in nm.COUNTERS if k not in ("numRays", "numHits"))
    else:
        # what that tmax admits: boxes that hold the ray's start; far less than the unseeded walk, and nothing is accepted
        base = _seeded(False, seed=sds.miss_seed(r))
        assert 0 < a[5]["numTopInnerVisits"] < base[5]["numTopInnerVisits"] and a[5]["numTriTests"] <= base[5]["numTriTests"]


def test_masks_compose_with_seeding():
    sc, r = sds.world_scene(), sds.rays()
    n = sc["inst"].shape[0]
    inst_masks = np.where(np.arange(n) % 2 == 0, 0x80000001, 0x2).astype(np.uint32)
    ray_masks = np.where(np.arange(r.shape[0]) % 3 == 0, 0x80000000, 0x3).astype(np.uint32)
    plain = _seeded(False)
    # per-ray and instance masks over the N instances, the world seen by every ray: the unseeded trace over N + 1 with the world's mask all ones
    a = _seeded(False, inst_masks=inst_masks, ray_masks=ray_masks)
    b = _unseeded_all(False, inst_masks=np.concatenate([inst_masks, [ALL]]).astype(np.uint32), ray_masks=ray_masks)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[4], b[4])
    assert a[5]["numInstancesMasked"] > 0 and a[5]["numInstanceEntries"] > 0 and not np.array_equal(a[4], plain[4])
    hit = (a[4] >= 0) & (a[4] < n)
    assert (inst_masks[a[4][hit]] & ray_masks[hit] != 0).all() and hit.sum() > 50
    # the launch's ray mask, and a mask that refuses every instance: the seed stays, the top level is still walked
    a = _seeded(False, inst_masks=inst_masks, ray_mask=0x2)
    hit = (a[4] >= 0) & (a[4] < n)
    assert (a[4][hit] % 2 == 1).all() and hit.sum() > 20
    seed = sds.world_seed(sc, r)
    for any_hit in (False, True):
        a = _seeded(any_hit, seed=seed, ray_mask=0)
        assert np.array_equal(np.stack([_bits(x) for x in a[:4]], axis=1), seed) and a[5]["numInstanceEntries"] == 0
        assert np.array_equal(a[4], np.where(seed[:, 0].view(np.int32) != -1, n, -1)) and a[5]["numInstancesMasked"] > 0


@pytest.mark.parametrize("any_hit", [False, True])
def test_the_two_level_counters_fall(any_hit):
    a, b = _seeded(any_hit)[5], _unseeded_all(any_hit)[5]
    print("anyHit=%d: %.2f 64-byte fetches per ray seeded, %.2f unseeded; %r; %r" % (any_hit, _fetches(a), _fetches(b), a, b))
    for k in ("numTopInnerVisits", "numInstanceEntries", "numInnerVisits", "numTriTests", "numLeafVisits"):
        assert a[k] < b[k], k
    assert _fetches(a) < _fetches(b) and a["numHits"] == b["numHits"]


# ---- the wide form -----------------------------------------------------------------------------------------------------------------------
def _wide(sc):
    if "wide" not in _cache:
        wp = nw.widen_pool(sc["pool"])
        t, ta = sc["tlas"], sc["tlas_all"]
        _cache["wide"] = (wp, nw.widen_tlas(t["nodes"], t["root_link"], sc["inst"], sc["pool"]["ranges"], wp["ranges"]),
                          nw.widen_tlas(ta["nodes"], ta["root_link"], sc["inst_all"], sc["pool"]["ranges"], wp["ranges"]))
    return _cache["wide"]


def _wide_seeded(any_hit, seed=None, seed_instance=None, **kw):
    sc, r = sds.world_scene(), sds.rays()
    wp, wt, _ = _wide(sc)
    seed = sds.world_seed(sc, r, any_hit) if seed is None else seed
    return nsd.trace_wide(seed, sc["inst"].shape[0] if seed_instance is None else seed_instance, wt["nodes"], wt["root_link"], wt["records"],
                          sc["pool"], wp, r, any_hit, **kw)


@pytest.mark.parametrize("any_hit", [False, True])
def test_wide_seeded_against_the_binary_seeded_spec(any_hit):
    """The rule between the two unseeded specs (np_instanced_wide's KNOWN LIMIT, test_instanced_wide_cpu.py): the wide spec is its own
    definition and is held to the brute-force yardstick (test_closest_hit_against_binary64_brute_force covers the wide form); between
    the two, hit or miss is compared -- an any-hit ray may end on another triangle -- and for closest hit the records, which no tie or
    rounded box separates on this scene.  The seeded state itself is exact: an all-miss seed gives np_instanced_wide.trace's every word
    and counter, and the wide counters fall as the binary ones do."""
    sc, r = sds.world_scene(), sds.rays()
    wp, wt, wta = _wide(sc)
    a, w = _seeded(any_hit), _wide_seeded(any_hit)
    assert np.array_equal(a[0] != -1, w[0] != -1)
    differ = (a[0] != w[0]) | (_bits(a[1]) != _bits(w[1])) | (a[4] != w[4])
    print("anyHit=%d: %d of %d records differ between the wide and the binary seeded spec" % (any_hit, int(differ.sum()), differ.size))
    if not any_hit:
        assert not differ.any()
    x = _wide_seeded(any_hit, seed=sds.miss_seed(r), seed_instance=5)
    y = nw.trace(wt["nodes"], wt["root_link"], wt["records"], sc["pool"], wp, r, any_hit)
    for p, q in zip(x[:5], y[:5]):
        assert np.array_equal(_bits(p), _bits(q))
    assert x[5] == y[5] and nsd.algorithmic_bytes_wide(x[5]) == nw.algorithmic_bytes(y[5]) + 16 * r.shape[0]
    u = nw.trace(wta["nodes"], wta["root_link"], wta["records"], sc["pool"], wp, r, any_hit)
    assert np.array_equal(u[0] != -1, w[0] != -1)
    for k in ("numTopInnerVisits", "numInstanceEntries", "numInnerVisits", "numTriTests", "numLeafVisits"):
        assert w[5][k] < u[5][k], k


def test_hostile_seed_words_are_taken_as_they_are():
    """NaN, infinities, negative t and id = INT_MIN: the ray is degenerate or not by !(tmin < tmax0) and nothing else; the words stay."""
    sc, r = sds.world_scene(), sds.rays()[:2048]
    t = sc["tlas"]
    n = r.shape[0]
    ts = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 1e30], F)[np.arange(n) % 6]
    ids = np.where(np.arange(n) % 4 == 0, -1, np.where(np.arange(n) % 4 == 1, np.iinfo(np.int32).min, 7)).astype(np.int32)
    seed = nsd.seed_of(ids, ts, 0xDEADBEEF, 0x7FC00001)
    for any_hit in (False, True):
        a = nsd.trace(seed, 32, t["nodes"], t["root_link"], t["records"], sc["pool"], r, any_hit)
        got = np.stack([_bits(x) for x in a[:4]], axis=1)
        kept = a[4] == np.where(ids != -1, 32, -1)
        dead = (ids != -1) & ~(r["tmin"] < ts)               # a seed that is a hit with a t that admits nothing
        assert kept[dead].all() and np.array_equal(got[dead], seed[dead]) and dead.sum() > 500
        assert np.array_equal(got[kept & (a[4] < 0)], seed[kept & (a[4] < 0)])      # a miss keeps its seed's t, whatever it is
        assert (~kept).sum() > 20                            # seeds that are misses or lie far still find the instances
