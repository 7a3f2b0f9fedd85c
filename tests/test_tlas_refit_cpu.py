"""ntr_tlas_refit without a device: the numpy rule (tests/np_tlas_refit.py) returns a freshly built top-level tree unchanged; after
moved instances and switched BLASes every child box is the union of the instance boxes below it (by a plain recursive walk), the
topology words stay, and the two-level spec trace through the refitted tree agrees with a binary64 brute force over the flattened scene
and, bit for bit, with the trace through a rebuilt tree; the entry point refuses every argument error in both forms and, without a
device, says so."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_scenes as isc
import np_hlbvh
import np_instanced as ni
import np_tlas_refit as tr

F = np.float32
SIZES = (1, 2, 3, 65, 300)
# world sizes of about 3 units for the three BLASes of pool(): cornell spans 555, soup1000 22, the one triangle 1
BASE_SCALE = (0.006, 0.15, 3.0)
_cache = {}


def pool():
    if "pool" not in _cache:
        _cache["pool"] = isc.pool_of(["cornell", "soup1000", "one"], gap_nodes=1, gap_rows=3)
    return _cache["pool"]


def placed(n, seed, blas=None):
    """n instances of pool()'s BLASes inside the volume isc.scene_rays looks at: a rotation, a non-uniform scale of the BLAS's base scale
    times [1/2, 2] per axis (the first three mirrored), a translation within +-10; more than 65 instances shrink so that the volume
    stays as full.  blas: the indices, or None for seeded ones (few soups: the brute force pays per triangle)."""
    rng = np.random.default_rng(seed)
    blas = rng.choice(3, n, p=(0.49, 0.02, 0.49)) if blas is None else np.asarray(blas)
    shrink = min(1.0, (65.0 / n) ** (1.0 / 3.0))
    tf = []
    for i in range(n):
        s = BASE_SCALE[int(blas[i])] * shrink * 2.0 ** rng.uniform(-1, 1, 3)
        if i < 3:
            s[i % 3] = -s[i % 3]
        tf.append(isc.transform(isc.rotation(rng), s, rng.uniform(-10, 10, 3)))
    return ni.instances(np.stack(tf), blas.astype(np.int32))


def moved(inst, seed):
    """New seeded transforms for every instance (mirrored and non-uniformly scaled ones among them) and another BLAS for every third"""
    rng = np.random.default_rng(seed)
    blas = inst["blas"].copy()
    third = np.arange(blas.size) % 3 == 0
    # (to the soup rarely, as in placed(): a cornell becomes the triangle and back, a soup either, one in twenty a soup)
    to_soup, coin = rng.random(blas.size) < 0.05, rng.integers(0, 2, blas.size) * 2
    blas[third] = np.where(blas == 1, coin, np.where(to_soup, 1, 2 - blas))[third]
    return placed(inst.shape[0], seed + 1, blas)


def built(n, seed=None):
    key = ("built", n, seed)
    if key not in _cache:
        inst = placed(n, 500 + n if seed is None else seed)
        _cache[key] = (inst, ni.tlas_build(pool()["nodes"], pool()["ranges"], inst))
    return _cache[key]


def refitted(n):
    """(moved instances, the spec's refit of built(n)'s tree to them), computed once"""
    key = ("refit", n)
    if key not in _cache:
        inst, t = built(n)
        new = moved(inst, 900 + n)
        _cache[key] = (new, tr.refit(t["nodes"], t["root_link"], t["records"], pool()["nodes"], pool()["ranges"], new))
    return _cache[key]


# ---- the property that ties build and refit together ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_refit_of_a_fresh_build_changes_nothing(n):
    inst, t = built(n)
    out = tr.refit(t["nodes"], t["root_link"], t["records"], pool()["nodes"], pool()["ranges"], inst)
    assert out["err_bits"] == 0
    assert out["nodes"].tobytes() == t["nodes"].tobytes() and out["records"].tobytes() == t["records"].tobytes()
    assert out["scene_box"].tobytes() == np.concatenate([t["scene_min"], t["scene_max"]]).tobytes()
    assert out["stats"] == dict(numNodes=n - 1, numLeaves=n)


# ---- moved instances ----------------------------------------------------------------------------------------------------------------------
def _below(nodes, link, inst, boxes):
    """The union of the instance boxes below `link` by a plain recursive walk: (lo, hi) as f2i integers; boxes[(slot, k)] collects it."""
    if link < 0:
        lo, hi = ni.instance_box(pool()["nodes"], pool()["ranges"][int(inst["blas"][~link])], inst["objectToWorld"][~link])
        return np_hlbvh.f2i(lo), np_hlbvh.f2i(hi)
    s = link // 64
    lo0, hi0 = boxes[(s, 0)] = _below(nodes, int(nodes[s, 12]), inst, boxes)
    lo1, hi1 = boxes[(s, 1)] = _below(nodes, int(nodes[s, 13]), inst, boxes)
    return np.minimum(lo0, lo1), np.maximum(hi0, hi1)


@pytest.mark.parametrize("n", SIZES)
def test_boxes_are_the_unions_of_the_instance_boxes_below(n):
    inst, t = built(n)
    new, out = refitted(n)
    assert (new["blas"] != inst["blas"]).sum() == (n + 2) // 3 and not np.array_equal(new["objectToWorld"], inst["objectToWorld"])
    assert out["err_bits"] == 0 and out["stats"] == dict(numNodes=n - 1, numLeaves=n)
    assert out["nodes"].shape == t["nodes"].shape and np.array_equal(out["nodes"][:, 12:], t["nodes"][:, 12:])
    assert out["records"].tobytes() == ni.tlas_build(pool()["nodes"], pool()["ranges"], new)["records"].tobytes()
    if n == 1:
        lo, hi = ni.instance_box(pool()["nodes"], pool()["ranges"][int(new["blas"][0])], new["objectToWorld"][0])
        assert out["scene_box"].tobytes() == np.concatenate([lo, hi]).tobytes()
        return
    boxes = {}
    lo, hi = _below(out["nodes"], 0, new, boxes)
    assert len(boxes) == 2 * (n - 1)
    nf = out["nodes"].view(F)
    for (s, k), (blo, bhi) in boxes.items():
        w = nf[s, tr.BOX_WORDS[k]]
        assert np.array_equal(np_hlbvh.f2i(w[tr.LO]), blo) and np.array_equal(np_hlbvh.f2i(w[tr.HI]), bhi), (n, s, k)
    assert out["scene_box"].tobytes() == np.concatenate([np_hlbvh.i2f(lo), np_hlbvh.i2f(hi)]).astype(F).tobytes()


def _near_a_box_plane(rays, t_b, which, inst, rel=1e-4):
    """Per ray of `which`: does its brute-force t lie within `rel` (relative) of a plane of some instance's world box?"""
    o = np.stack([rays[k] for k in ("ox", "oy", "oz")], axis=1).astype(np.float64)[which]
    d = np.stack([rays[k] for k in ("dx", "dy", "dz")], axis=1).astype(np.float64)[which]
    near = np.zeros(which.size, bool)
    for i in range(inst.shape[0]):
        lo, hi = ni.instance_box(pool()["nodes"], pool()["ranges"][int(inst["blas"][i])], inst["objectToWorld"][i])
        with np.errstate(all="ignore"):
            for plane in (lo.astype(np.float64), hi.astype(np.float64)):
                tp = (plane[None, :] - o) / d
                near |= (np.abs(tp - t_b[which, None]) <= rel * np.abs(t_b[which, None])).any(axis=1)
    return near


@pytest.mark.parametrize("n", SIZES)
def test_trace_through_the_refitted_tree_against_brute_force_and_a_rebuilt_tree(n):
    """Hit / miss status against a binary64 brute force over the flattened world-space triangles.  A ray may differ only where its
    brute-force t lies within 1e-4 (relative) of a plane of an instance's world box -- boxes are not padded, so such a hit can be culled,
    as in every two-level tracer -- and at most 1 % of the rays may.  Measured with these seeds: no ray differs at any of the five sizes.
    The closest hit through the refitted tree also equals the one through a tree rebuilt over the moved instances in every word: both
    trees bound the same instance boxes exactly, so they differ in the order of the visits only."""
    new, out = refitted(n)
    rays = isc.scene_rays((32, 32), 1024)
    sc = dict(names=["cornell", "soup1000", "one"], transforms=new["objectToWorld"], blas=new["blas"])
    verts, _ = isc.flatten(sc)
    hit_b, t_b = isc.brute_force(verts, rays, chunk=128)
    rid, rt, ru, rv, rinst = ni.trace(out["nodes"], -1 if n == 1 else 0, out["records"], pool(), rays)
    differ = np.flatnonzero((rid >= 0) != hit_b)
    excused = _near_a_box_plane(rays, np.where(hit_b, t_b, rt.astype(np.float64)), differ, new) if differ.size else np.zeros(0, bool)
    print("N=%d: %d rays, %d hit, %d differ from the brute force in status, %d of them within 1e-4 of an instance-box plane"
          % (n, rays.shape[0], int(hit_b.sum()), differ.size, int(excused.sum())))
    assert excused.all(), ("a ray differs away from every box plane", n, differ[~excused])
    assert differ.size <= rays.shape[0] // 100
    assert hit_b.sum() > rays.shape[0] // 50 or n <= 3
    rebuilt = ni.tlas_build(pool()["nodes"], pool()["ranges"], new)
    eid, et, eu, ev, einst = ni.trace(rebuilt["nodes"], rebuilt["root_link"], rebuilt["records"], pool(), rays)
    assert np.array_equal(rid, eid) and np.array_equal(rinst, einst) and rt.tobytes() == et.tobytes()
    assert ru.tobytes() == eu.tobytes() and rv.tobytes() == ev.tobytes()


def test_a_bad_part_is_not_followed_in_the_rule():
    """Rule 7 on 5 instances: a box is rewritten exactly where everything below it is well formed."""
    inst, t = built(5, seed=77)
    new = moved(inst, 78)
    nodes = t["nodes"].copy()
    good = tr.refit(nodes, 0, t["records"], pool()["nodes"], pool()["ranges"], new)
    leaf = [(s, k) for s in range(4) for k in (0, 1) if nodes[s, 12 + k] < 0]
    for change, bit in (("blas", tr.ERR_BLAS), ("link", tr.ERR_LINK), ("leaf", tr.ERR_LEAF)):
        bad_nodes, bad_inst = nodes.copy(), new.copy()
        s, k = leaf[1]
        if change == "blas":
            bad_inst["blas"][~nodes[s, 12 + k]] = 3
        else:
            bad_nodes[s, 12 + k] = 64 * 9 if change == "link" else ~7
        out = tr.refit(bad_nodes, 0, t["records"], pool()["nodes"], pool()["ranges"], bad_inst)
        assert out["err_bits"] == bit and not out["scene_box"].any()
        assert np.array_equal(out["nodes"][:, 12:], bad_nodes[:, 12:])
        # the bad child and its ancestors keep their bytes; every other box is the good refit's
        stale = {(s, k)}
        node = s
        while node != 0:
            ps, pk = next((a, b) for a in range(4) for b in (0, 1) if nodes[a, 12 + b] == 64 * node)
            stale.add((ps, pk))
            node = ps
        for a in range(4):
            for b in (0, 1):
                want = bad_nodes if (a, b) in stale else good["nodes"]
                assert np.array_equal(out["nodes"][a, tr.BOX_WORDS[b]], want[a, tr.BOX_WORDS[b]]), (change, a, b)
        i = ~nodes[s, 12 + k]
        for j in range(5):
            want = t["records"][j] if (change == "blas" and j == i) else good["records"][j]
            assert np.array_equal(out["records"][j], want), (change, j)


# ---- symbols, sizes and the argument table ----------------------------------------------------------------------------------------------
def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols_and_sizes():
    assert C.sizeof(nt.TlasRefitResult) == 48
    assert nt.lib().ntr_tlas_refit_scratch_bytes(None) == -1 and b"ntr_tlas_refit_scratch_bytes" in nt.lib().ntr_last_error()
    assert isinstance(nt.tlas_refit_scratch_bytes(), int)


@pytest.mark.parametrize("blocking", [True, False])
def test_argument_errors_and_no_device(blocking):
    """Pointers are never dereferenced by a refused call (they are fake); the accepted call runs only where there is no device."""
    fake = 0x10000
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    good = dict(num_instances=5, d_instances=fake, ranges=ranges, d_pool_nodes=fake, pool_nodes_bytes=704, d_tlas_nodes=fake,
                tlas_nodes_bytes=256, root_link=0, d_records=fake, records_cap=320, d_scene_box=fake, blocking=blocking)
    one = dict(good, num_instances=1, d_tlas_nodes=0, tlas_nodes_bytes=0, root_link=-1, records_cap=64)
    bad_ranges = [[(32, 640, 0, 1600)], [(0, 96, 0, 1600)], [(0, 0, 0, 1600)], [(640, 128, 0, 1600)], [(0, 640, 8, 1600)], [(0, 640, 0, 1608)],
                  [(-64, 640, 0, 1600)], [(0, 640, -16, 1600)], [(0, 640, 0xFFFFFF00, 1600)], [(0, 640, 0, 0)]]
    cases = [dict(d_instances=0), dict(d_pool_nodes=0), dict(d_records=0), dict(d_tlas_nodes=0),
             dict(num_instances=0), dict(num_instances=-3), dict(num_instances=0x76543200 // 64 + 2, tlas_nodes_bytes=0x76543200 + 64),
             dict(ranges=[]),
             dict(tlas_nodes_bytes=192), dict(tlas_nodes_bytes=320), dict(tlas_nodes_bytes=0),
             dict(root_link=-1), dict(root_link=64), dict(records_cap=319),
             dict(d_instances=fake + 8), dict(d_pool_nodes=fake + 4), dict(d_tlas_nodes=fake + 8), dict(d_records=fake + 12),
             dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700), dict(pool_nodes_bytes=0xFFFFFF40)] + [dict(ranges=r) for r in bad_ranges]
    cases = [dict(good, **c) for c in cases]
    cases += [dict(one, root_link=0), dict(one, root_link=-2), dict(one, tlas_nodes_bytes=64), dict(one, records_cap=63)]
    cases.append(dict(good, pool_nodes_bytes=0xFFFFFF00, ranges=[(0, 0x76543240, 0, 1600)]))   # a BLAS above Compact's limit
    for kw in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.tlas_refit(**kw)
        assert e.value.code == -1 and "ntr_tlas_refit" in str(e.value), (kw, str(e.value))
        if blocking:
            assert bytes(e.value.result) == bytes(48), kw
    L = nt.lib()
    res = nt.TlasRefitResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert L.ntr_tlas_refit(5, fake, 2, None, fake, 704, fake, 256, 0, fake, 320, None, C.byref(res) if blocking else None, None) == -1
    assert not blocking or bytes(res) == bytes(48)
    if not _has_device():
        for kw in (good, dict(good, d_scene_box=0), one):
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_refit(**kw)
            assert e.value.code in (-2, -3), (kw, str(e.value))
        assert nt.tlas_refit_scratch_bytes() == 0
