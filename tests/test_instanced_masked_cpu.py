"""Instance visibility masks and counters without a device: the spec tests/np_instanced_masked.py equals np_instanced.trace when nothing
is masked; parity masks change a good share of the records and every remaining hit names a visible instance; against a binary64 brute
force over the visible instances' flattened triangles the masked spec is held to test_instanced_cpu.py's own cap; the counters obey
their identities; ntr_trace_instanced_masked and ntr_trace_instanced_stats refuse bad arguments and, without a device, say so; the
structs have the header's sizes and algorithmic_bytes is the header's formula."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_instanced as ni
import np_instanced_masked as nm
import np_tracer

F = np.float32
SCENES = ["three", "grid", "mirror"]
_cache = {}


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _scene(name):
    """-> (scene dict, pool, spec TLAS) of a named scene, built once."""
    if name not in _cache:
        sc = isc.scene(name)
        pool = isc.pool_of(sc["names"])
        _cache[name] = sc, pool, ni.tlas_build(pool["nodes"], pool["ranges"], ni.instances(sc["transforms"], sc["blas"]))
    return _cache[name]


def _rays():
    if "rays" not in _cache:
        _cache["rays"] = np.concatenate([scenes.primary_rays(isc.CAMERA, 64, 32)[0], scenes.random_rays(2048, 5, extent=12.0)])
    return _cache["rays"]


def _trace(name, any_hit=False, rays=None, **masks):
    sc, pool, t = _scene(name)
    return nm.trace(t["nodes"], t["root_link"], t["records"], pool, _rays() if rays is None else rays, any_hit, **masks)


def _unmasked(name, any_hit):
    key = ("unmasked", name, any_hit)
    if key not in _cache:
        _cache[key] = _trace(name, any_hit)
    return _cache[key]


def _parity(n):
    """Instance masks 1 for even instances and 2 for odd ones."""
    return np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


# ---- (1) no masks: np_instanced.trace --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_spec_without_masks_equals_the_unmasked_spec(name):
    sc, pool, t = _scene(name)
    n = sc["blas"].shape[0]
    for any_hit in (False, True):
        want = ni.trace(t["nodes"], t["root_link"], t["records"], pool, _rays(), any_hit)
        got = _unmasked(name, any_hit)
        assert _same(got[:5], want), (name, any_hit)
        assert got[5]["numInstancesMasked"] == 0
        # all-ones arrays and an all-ones ray mask are no masks either, counters included
        ones = _trace(name, any_hit, inst_masks=np.full(n, 0xFFFFFFFF, np.uint32), ray_masks=np.full(_rays().shape[0], 0xFFFFFFFF, np.uint32))
        assert _same(ones[:5], want) and ones[5] == got[5]


# ---- (2) parity masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_parity_masks_change_records_and_hits_name_visible_instances(name):
    n = _scene(name)[0]["blas"].shape[0]
    M = _parity(n)
    base = _unmasked(name, False)
    hits = int((base[0] != -1).sum())
    per_ray = np.where(np.arange(_rays().shape[0]) % 2 == 0, 1, 2).astype(np.uint32)
    for what, kw, m in (("ray mask 2", dict(ray_mask=2), np.full(_rays().shape[0], 2, np.uint32)), ("per-ray 1 / 2", dict(ray_masks=per_ray), per_ray)):
        got = _trace(name, False, inst_masks=M, **kw)
        changed = np.zeros(_rays().shape[0], bool)
        for g, b in zip(got[:5], base[:5]):
            changed |= g.view(np.uint32) != b.view(np.uint32)
        changed &= base[0] != -1
        print("%s, %s: %d of %d hit rays change their record" % (name, what, int(changed.sum()), hits))
        assert changed.sum() * 10 >= hits > 0, (name, what, int(changed.sum()), hits)
        hit = got[0] != -1
        assert (got[4][hit] >= 0).all() and ((M[got[4][hit]] & m[hit]) != 0).all()      # every remaining hit names a visible instance
        assert (got[4][~hit] == -1).all()
    # nothing visible: every ray misses and no ray pays a bottom-level step
    for kw in (dict(inst_masks=np.zeros(n, np.uint32)), dict(ray_mask=0), dict(inst_masks=M, ray_mask=0x80000000)):
        rid, rt, ru, rv, rinst, c = _trace(name, False, **kw)
        assert (rid == -1).all() and (rinst == -1).all() and (ru == 0).all() and (rv == 0).all()
        assert np.array_equal(rt.view(np.uint32), _rays()["tmax"].view(np.uint32))
        assert c["numInstanceEntries"] == c["numInnerVisits"] == c["numTriTests"] == c["numLeafVisits"] == c["numHits"] == 0
        assert c["numTopInnerVisits"] > 0 and c["numInstancesMasked"] > 0                                     # the top level is still walked


def test_bit_31_is_a_mask_bit():
    n = _scene("three")[0]["blas"].shape[0]
    M = np.array([0x80000000, 1, 0x80000001], np.uint32)[:n]
    got = _trace("three", False, inst_masks=M, ray_mask=0x80000000)
    hit = got[0] != -1
    assert hit.any() and set(np.unique(got[4][hit])) <= {0, 2} and (got[4][hit] == 0).any()


# ---- (3) the binary64 brute force over the visible instances ---------------------------------------------------------------------------
@pytest.mark.parametrize("ray_mask", [1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_masked_spec_against_binary64_brute_force(name, ray_mask):
    """test_instanced_cpu.py's yardstick, over the visible instances only: status mismatches plus rays beyond four times the flat
    single-level tracer's largest relative t error may number at most 2 f_bad + 4, f_bad the flat tracer's own status mismatches against
    the same brute force; at least 500 rays must hit."""
    sc, pool, t = _scene(name)
    M = _parity(sc["blas"].shape[0])
    rays = isc.scene_rays((96, 64), 2048)
    verts, who = isc.flatten(sc)
    keep = (M[who[:, 0]] & np.uint32(ray_mask)) != 0
    verts = verts[keep]
    hit_b, t_b = isc.brute_force(verts, rays)
    pos32 = verts.reshape(-1, 3).astype(F)
    tri = np.arange(pos32.shape[0], dtype=np.int32).reshape(-1, 3)
    flat = pl.build(tri, pos32, *pl.scene_box(pos32), 8)
    fid, ft = np_tracer.trace(flat["nodes"], flat["woop"], flat["tri_index"], rays)
    rid, rt, _, _, rinst, _ = nm.trace(t["nodes"], t["root_link"], t["records"], pool, rays, False, inst_masks=M, ray_mask=ray_mask)

    def against_brute(hit, tt, tol):
        both = hit & hit_b
        rel = np.abs(tt[both].astype(np.float64) - t_b[both]) / np.abs(t_b[both])
        status = int((hit != hit_b).sum())
        return status, (float(rel.max()) if rel.size else 0.0), status + (int((rel > tol).sum()) if tol is not None else 0)

    f_status, f_err, f_bad = against_brute(fid >= 0, ft, None)
    i_status, i_err, i_bad = against_brute(rid >= 0, rt, 4.0 * f_err)
    print("%s, ray mask %d: %d rays, %d hit; flat tracer: %d status mismatches, largest relative t error %.3g; masked spec: %d status "
          "mismatches, largest relative t error %.3g, %d rays beyond the tolerance %.3g"
          % (name, ray_mask, rays.shape[0], int(hit_b.sum()), f_status, f_err, i_status, i_err, i_bad - i_status, 4.0 * f_err))
    assert hit_b.sum() >= 500
    assert i_bad <= 2 * f_bad + 4, (i_bad, f_bad)
    hit = rid >= 0
    assert ((M[rinst[hit]] & np.uint32(ray_mask)) != 0).all() and (rinst[~hit] == -1).all()


# ---- counter identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid"])
def test_counter_identities(name, monkeypatch):
    """numHits is the records' hit count; numInstanceEntries + numInstancesMasked is the entering steps and numTriTests + numLeafVisits
    the rows read, both counted a second way: at the spec's two tests (visible, is_terminator), by the sizes of the batches they see."""
    n = _scene(name)[0]["blas"].shape[0]
    M = _parity(n)
    seen = dict(enter=0, rows=0)
    visible, is_terminator = nm.visible, nm.is_terminator

    def count_visible(Mi, m, i, k):
        seen["enter"] += int(i.size)
        return visible(Mi, m, i, k)

    def count_rows(rows_u32, row):
        seen["rows"] += int(row.size)
        return is_terminator(rows_u32, row)

    monkeypatch.setattr(nm, "visible", count_visible)
    monkeypatch.setattr(nm, "is_terminator", count_rows)
    per_ray = np.where(np.arange(_rays().shape[0]) % 2 == 0, 1, 2).astype(np.uint32)
    for any_hit in (False, True):
        for kw in (dict(), dict(inst_masks=M, ray_mask=2), dict(inst_masks=M, ray_masks=per_ray), dict(ray_mask=0)):
            seen.update(enter=0, rows=0)
            rid, _, _, _, rinst, c = _trace(name, any_hit, **kw)
            assert tuple(c) == nm.COUNTERS and c["numRays"] == _rays().shape[0]
            assert c["numHits"] == int((rid != -1).sum()) == int((rinst != -1).sum())
            assert c["numInstanceEntries"] + c["numInstancesMasked"] == seen["enter"] > 0
            assert c["numTriTests"] + c["numLeafVisits"] == seen["rows"]
            assert (c["numInstancesMasked"] > 0) == bool(kw) and (c["numInstanceEntries"] > 0) == (kw != dict(ray_mask=0))
            assert c["numInnerVisits"] >= c["numInstanceEntries"]      # every entry reads node 0 of its BLAS


# ---- argument errors and "no device" ----------------------------------------------------------------------------------------------------
def test_struct_sizes_and_algorithmic_bytes():
    assert C.sizeof(nt.InstanceVisibility) == 24 and C.sizeof(nt.InstancedTraceStats) == 64
    assert [f for f, _ in nt.InstancedTraceStats._fields_] == list(nm.COUNTERS)
    v = nt.InstanceVisibility(0x1000, 0x2000, 0x80000001)
    assert (v.d_instanceMasks, v.d_rayMasks, v.rayMask, v.pad) == (0x1000, 0x2000, 0x80000001, 0)
    d = nt.InstanceVisibility()
    assert (d.d_instanceMasks, d.d_rayMasks, d.rayMask) == (None, None, 0xFFFFFFFF)
    st = nt.InstancedTraceStats(1000, 7, 11, 13, 17, 19, 23, 29)
    hand = 52 * 1000 + 64 * (7 + 11 + 17) + 32 * 11 + 48 * 19 + 16 * 23 + 4 * 29
    assert hand == 55988
    assert st.algorithmic_bytes() == hand
    assert st.algorithmic_bytes(instance_masks=True) == hand + 4 * (11 + 13)
    assert st.algorithmic_bytes(ray_masks=True) == hand + 4 * 1000
    assert st.algorithmic_bytes(True, True) == hand + 4 * 24 + 4000 == nm.algorithmic_bytes(st.as_dict(), True, True)
    assert st.as_dict() == dict(zip(nm.COUNTERS, (1000, 7, 11, 13, 17, 19, 23, 29)))


def test_argument_errors_and_no_device():
    """Pointers are never dereferenced by a refused call; the accepted call runs only where there is no device to run it on."""
    fake = 0x10000
    tgood = dict(num_rays=64, any_hit=False, d_rays=fake, d_results=fake, d_instance_ids=fake, d_tlas_nodes=fake, tlas_nodes_bytes=256, root_link=0,
                 d_records=fake, num_instances=5, d_pool_nodes=fake, pool_nodes_bytes=704, d_pool_woop=fake, pool_woop_bytes=1680, d_pool_tri_index=fake)
    changes = [dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_instance_ids=0), dict(d_records=0), dict(num_instances=0),
               dict(root_link=64), dict(root_link=~5), dict(tlas_nodes_bytes=0), dict(tlas_nodes_bytes=100), dict(d_tlas_nodes=0),
               dict(pool_nodes_bytes=0), dict(pool_woop_bytes=8), dict(pool_woop_bytes=0xFFFFFF10), dict(d_pool_tri_index=0),
               dict(vis=nt.InstanceVisibility(fake + 2, 0)), dict(vis=nt.InstanceVisibility(0, fake + 1)), dict(vis=nt.InstanceVisibility(fake, fake + 3, 1))]
    for fn in (nt.trace_instanced_masked, nt.trace_instanced_stats):
        for vis in (None, nt.InstanceVisibility(fake, fake, 3)):
            for change in changes:
                with pytest.raises(nt.NtrError) as e:
                    fn(**dict(dict(tgood, vis=vis), **change))
                assert e.value.code == -1, (fn.__name__, change, str(e.value))
    assert nt.trace_instanced_masked(**dict(tgood, num_rays=0)) == 0.0
    st = nt.trace_instanced_stats(**dict(tgood, num_rays=0, vis=nt.InstanceVisibility(fake, 0, 1)))
    assert bytes(st) == bytes(64)
    # a null stats is refused, and a refused or empty call leaves the caller's stats zeroed
    L = nt.lib()
    args = (64, 0, fake, fake, fake, fake, 256, 0, fake, 5, fake, 704, fake, 1680, fake)
    assert L.ntr_trace_instanced_stats(*args, None, None, None) == -1 and b"null stats" in L.ntr_last_error()
    st = nt.InstancedTraceStats()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert L.ntr_trace_instanced_stats(*((-1,) + args[1:]), None, C.byref(st), None) == -1 and bytes(st) == bytes(64)
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert L.ntr_trace_instanced_stats(*((0,) + args[1:]), None, C.byref(st), None) == 0 and bytes(st) == bytes(64)
    if not _has_device():
        for vis in (None, nt.InstanceVisibility(fake, fake, 3)):
            with pytest.raises(nt.NtrError) as e:
                nt.trace_instanced_masked(**dict(tgood, vis=vis))
            assert e.value.code in (-2, -3)
            with pytest.raises(nt.NtrError) as e:
                nt.trace_instanced_stats(**dict(tgood, vis=vis))
            assert e.value.code in (-2, -3)
