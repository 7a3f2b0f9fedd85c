"""The edge trees (tests/edge_trees.py) without a GPU: the construction, the flags each scene is built for, the conditions on the ray
sets, the two CPU restatements of the tracer against each other on every scene and set, and what a slightly worse divide would change
-- the reason the GPU tier compares counters and not only records."""
import numpy as np
import pytest

import np_tracer
from oracle import oracle

import edge_trees as et
from np_bvh_validate import FASTDIV, FINITE, NOTINY

F = np.float32
U = np.uint32
FLT_MAX = np.finfo(F).max
COUNTERS = ("numInnerVisits", "numTriTests", "numLeafVisits", "numHits")


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(et.SCENES))
def test_scene_has_the_flags_it_is_built_for(name):
    sc = et.scene(name)
    must, must_not = et.MUST[name]
    flags = sc.flags()
    assert flags & must == must and flags & must_not == 0, "%s: flags 0x%x" % (name, flags)
    nodes = et.node_words(sc.nodes)
    assert nodes.shape[0] == sc.in_tree.sum() - 1, "one triangle per leaf"
    assert sc.in_tree.all() or name.startswith("tinyz")
    c = sc.box_coordinates()
    pos = sc.pos.astype(np.float64).reshape(-1, 3, 3)[sc.in_tree]
    assert c.min() == pos.min() and c.max() == pos.max() and np.isin(c, pos).all(), "boxes are exact minima and maxima"


def test_far_boxes_lie_in_the_last_admitted_binade():
    a = np.abs(et.scene("far").box_coordinates())
    assert a.min() >= 2.0 ** 54 and a.max() < 2.0 ** 55


def test_far_top_and_far_out_differ_in_one_coordinate_value():
    top, out, far = et.scene("far_top"), et.scene("far_out"), et.scene("far")
    assert top.box_coordinates().max() == 2.0 ** 55 - 2.0 ** 31 == float(np.nextafter(F(2.0 ** 55), F(0)))
    assert out.box_coordinates().max() == 2.0 ** 55
    assert top.moved == out.moved and np.array_equal(top.rows[:, 1:], out.rows[:, 1:]) and np.array_equal(top.rows[:, 1:], far.rows[:, 1:])
    differ = np.flatnonzero((top.pos != out.pos).any(1))
    assert differ.tolist() == [3 * top.moved, 3 * top.moved + 1, 3 * top.moved + 2], "the three vertices of one x-plane triangle"
    assert top.rows[top.moved, 0].tolist() == [1.0, 0.0, 0.0, 2.0 ** 55 - 2.0 ** 31] and out.rows[out.moved, 0, 3] == 2.0 ** 55


def test_tinyz_reaches_the_smallest_admitted_coordinate():
    for name, smallest in (("tinyz", 2.0 ** -93), ("tinyz_out", 2.0 ** -94)):
        a = np.abs(et.scene(name).box_coordinates())
        assert a[a > 0].min() == smallest
    assert np.array_equal(et.node_words(et.scene("tinyz").nodes)[:, 12:], et.node_words(et.scene("tinyz_out").nodes)[:, 12:]), "the same tree"


def test_unit_analytic_rows_find_what_the_host_builders_rows_find():
    sc = et.scene("unit")
    rays = sc.rays("long")
    own, _ = oracle.trace(sc.nodes, sc.built.woop, sc.tri_index, rays)
    ref, _ = sc.reference("long", False)
    assert np.array_equal(own["id"], ref["id"])
    assert (ref["id"] >= 0).sum() > rays.shape[0] // 10


# ---- the ray sets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", et.CASES)
def test_ray_set_meets_its_conditions(name, which):
    sc = et.scene(name)
    rays = sc.rays(which)
    n = rays.shape[0]
    assert n % 64 == 1 and 0 < et.prefix(n) % 64 < 63
    nice = sc.nice(rays)
    if which == "zero" and name == "tinyz_out":
        assert not nice.any(), "without NOTINY no zero-origin ray is nice: every wave is GENERIC"
    elif name == "far_out":
        pass                                                       # FASTDIV is withheld: the tree keeps every wave off the FAST path
    elif which == "one_out":
        per_wave = nice[:n - 1].reshape(-1, 64).sum(1)
        assert (per_wave == 64).sum() >= 6 and (per_wave == 63).sum() >= 6, "FAST waves beside waves kept off it by one lane"
    else:
        assert nice.sum() >= 0.9 * n, "%d of %d nice" % (nice.sum(), n)
    if which in ("end_hi", "end_lo"):
        d = np.abs(np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)).astype(np.float64)
        if which == "end_hi":
            assert (d.max(1) >= 2.0 ** 19).all() and (d.max(1) <= 2.0 ** 20).all()
        else:
            assert (d.min(1) >= 2.0 ** -40).all() and (d.min(1) <= 2.0 ** -39).all()
        assert sc.nice(rays).sum() == sc.nice(sc.rays("long")[:n]).sum(), "scaling keeps every ray nice"
    if which == "zero":
        assert ((rays["oz"] == 0) & (np.abs(rays["dz"]) >= F(2.0 ** 19)) & (np.abs(rays["dz"]) <= F(2.0 ** 20))).all()
        assert np.signbit(rays["oz"]).sum() > n // 4 and (~np.signbit(rays["oz"])).sum() > n // 4
    ref, _ = sc.reference(which, False)
    real = (ref["id"] >= 0) & (ref["t"] < FLT_MAX)
    miss = ref["id"] < 0
    print("%s %s: %d rays, %d nice, %d real hits, %d misses, %d recorded misses" % (name, which, n, nice.sum(), real.sum(), miss.sum(),
                                                                                 n - real.sum() - miss.sum()))
    assert real.sum() >= 0.1 * n and (~real).sum() >= 0.1 * n, "hits and misses"
    finite = np.isfinite(rays["tmax"]) & real
    if which != "short":
        assert (ref["t"][finite].astype(np.float64) < 0.5 * rays["tmax"][finite]).all(), "a finite tmax lies above every hit"
    if sc.moved is not None:
        assert (ref["id"] == sc.moved).sum() >= 8, "rays that cross the moved triangle's box and hit it"


# ---- the two restatements --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", et.CASES)
def test_np_tracer_equals_oracle(name, which):
    sc = et.scene(name)
    rays = sc.rays(which)
    for any_hit in (False, True):
        ref, rst = sc.reference(which, any_hit)
        rid, rt, st = np_tracer.trace(sc.nodes, sc.woop, sc.tri_index, rays, any_hit=any_hit, return_stats=True)
        assert np.array_equal(rid, ref["id"]) and np.array_equal(rt.view(U), ref["t"].view(U)), (name, which, any_hit)
        assert st == {k: rst.as_dict()[k] for k in COUNTERS}, (name, which, any_hit)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------------
def _reciprocal(x, d):
    """x * RN(1 / d): one rounding short of the FAST path's corrected quotient"""
    return x * (F(1.0) / d)


def _flushing(x, d):
    """the divide, with quotients below 2^-112 flushed to zero"""
    q = x / d
    return np.where(np.abs(q) < F(2.0 ** -112), F(0.0) * q, q)


def _visits(sc, which, divide):
    rays = sc.rays(which)
    rid, rt, st = np_tracer.trace(sc.nodes, sc.woop, sc.tri_index, rays, return_stats=True, divide=divide)
    ref, _ = sc.reference(which, False)
    changed = int(((rid != ref["id"]) | (rt.view(U) != ref["t"].view(U))).sum())
    return st["numInnerVisits"], changed


@pytest.mark.parametrize("name", ("unit", "far"))
def test_a_divide_one_rounding_short_changes_the_counters(name):
    sc = et.scene(name)
    exact, _ = _visits(sc, "long", None)
    worse, changed = _visits(sc, "long", _reciprocal)
    print("%s long: numInnerVisits %d -> %d with x * RN(1/d), %d records change" % (name, exact, worse, changed))
    assert worse != exact, "the long rays must tell the divide from x * (1 / d)"


def test_a_divide_that_flushes_small_quotients_changes_tinyz():
    sc = et.scene("tinyz")
    exact, _ = _visits(sc, "zero", None)
    recip, changed_r = _visits(sc, "zero", _reciprocal)
    flush, changed_f = _visits(sc, "zero", _flushing)
    print("tinyz zero: numInnerVisits %d, %d with x * RN(1/d) (%d records), %d with quotients below 2^-112 flushed (%d records)" % (
        exact, recip, changed_r, flush, changed_f))
    assert flush != exact or changed_f > 0, "the zero-origin rays must tell the divide from one that loses quotients of 2^-113"
