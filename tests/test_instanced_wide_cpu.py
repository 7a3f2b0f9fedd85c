"""The two-level trace over 4-wide trees without a device: the spec tests/np_instanced_wide.py against a binary64 brute force with the
yardstick of test_instanced_cpu.py, against np_bvh_wide.trace through one identity instance, and with masks against the visible instances
alone; the structure widen_pool and widen_tlas promise; and the argument errors and no-device returns of the five new entry points."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_bvh_wide as bw
import np_instanced as ni
import np_instanced_wide as nw
import np_tracer

F = np.float32


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _scene(name):
    sc = isc.scene(name)
    pool = isc.pool_of(sc["names"])
    inst = ni.instances(sc["transforms"], sc["blas"])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    wpool = nw.widen_pool(pool)
    wt = nw.widen_tlas(t["nodes"], t["root_link"], inst, pool["ranges"], wpool["ranges"])
    return sc, pool, inst, t, wpool, wt


# ---- the spec against the world ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_spec_against_binary64_brute_force(name):
    """test_instanced_cpu.py::test_spec_against_binary64_brute_force's yardstick, unchanged: the single-level np_tracer on the flattened
    mesh against the same brute force.  The wide instanced spec may disagree on at most twice that count of bad rays plus four, at four
    times that largest relative t error."""
    sc, pool, inst, t, wpool, wt = _scene(name)
    rays = isc.scene_rays((96, 64), 2048)
    verts, who = isc.flatten(sc)
    hit_b, t_b = isc.brute_force(verts, rays)
    pos32 = verts.reshape(-1, 3).astype(F)
    tri = np.arange(pos32.shape[0], dtype=np.int32).reshape(-1, 3)
    flat = pl.build(tri, pos32, *pl.scene_box(pos32), 8)
    fid, ft = np_tracer.trace(flat["nodes"], flat["woop"], flat["tri_index"], rays)
    rid, rt, _, _, rinst, _ = nw.trace(wt["nodes"], wt["root_link"], wt["records"], pool, wpool, rays)

    def against_brute(hit, tt, tol):
        both = hit & hit_b
        rel = np.abs(tt[both].astype(np.float64) - t_b[both]) / np.abs(t_b[both])
        status = int((hit != hit_b).sum())
        return status, (float(rel.max()) if rel.size else 0.0), status + (int((rel > tol).sum()) if tol is not None else 0)

    f_status, f_err, f_bad = against_brute(fid >= 0, ft, None)
    i_status, i_err, i_bad = against_brute(rid >= 0, rt, 4.0 * f_err)
    print("%s: %d rays, %d hit; flat tracer: %d status mismatches, largest relative t error %.3g; wide instanced spec: %d status "
          "mismatches, largest relative t error %.3g, %d rays beyond the tolerance %.3g"
          % (name, rays.shape[0], int(hit_b.sum()), f_status, f_err, i_status, i_err, i_bad - i_status, 4.0 * f_err))
    assert hit_b.sum() > rays.shape[0] // 8
    assert i_bad <= 2 * f_bad + 4, (i_bad, f_bad)
    assert (rinst[rid >= 0] >= 0).all() and (rinst[rid < 0] == -1).all()


def test_spec_identity_instance_equals_the_wide_single_level_tracer():
    tri, pos, b = isc.blas("soup1000")
    pool = isc.pool_of(["soup1000"])
    inst = ni.instances([ni.IDENTITY], [0])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    wpool = nw.widen_pool(pool)
    wt = nw.widen_tlas(t["nodes"], t["root_link"], inst, pool["ranges"], wpool["ranges"])
    assert wt["root_link"] == -1 and wt["nodes"].shape == (0, 32)
    single = bw.widen(b["nodes"])
    assert wpool["nodes"].tobytes() == single["nodes"].tobytes()
    rays = np.concatenate([isc.finite_edge_rays(), isc.odd_rays()])
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst, cnt = nw.trace(wt["nodes"], wt["root_link"], wt["records"], pool, wpool, rays, any_hit)
        eid, et, eu, ev, est = bw.trace(single["nodes"], b["woop"], b["tri_index"], rays, any_hit=any_hit, return_stats=True)
        assert np.array_equal(rid, eid) and np.array_equal(rt.view(np.uint32), et.view(np.uint32))
        assert np.array_equal(ru.view(np.uint32), eu.view(np.uint32)) and np.array_equal(rv.view(np.uint32), ev.view(np.uint32))
        assert np.array_equal(rinst, np.where(eid >= 0, 0, -1))
        live = int((rays["tmin"] < rays["tmax"]).sum())
        assert cnt["numTopInnerVisits"] == 0 and cnt["numInstanceEntries"] == live and cnt["numInstancesMasked"] == 0
        assert (cnt["numInnerVisits"], cnt["numTriTests"], cnt["numLeafVisits"], cnt["numHits"]) == \
            (est["numInnerVisits"], est["numTriTests"], est["numLeafVisits"], est["numHits"])


def test_spec_masks_equal_the_visible_instances_alone():
    sc, pool, inst, t, wpool, wt = _scene("grid")
    rays = isc.scene_rays((48, 32), 1024)
    n = inst.shape[0]
    masks = np.where(np.arange(n) % 2 == 0, 0x80000000, 0x1).astype(np.uint32)      # parity: bit 31 is a mask bit like any other
    for ray_mask, keep in ((0x80000000, np.arange(n) % 2 == 0), (0x1, np.arange(n) % 2 == 1)):
        sub = inst[keep]
        ts = ni.tlas_build(pool["nodes"], pool["ranges"], sub)
        ws = nw.widen_tlas(ts["nodes"], ts["root_link"], sub, pool["ranges"], wpool["ranges"])
        for any_hit in (False, True):
            a = nw.trace(wt["nodes"], wt["root_link"], wt["records"], pool, wpool, rays, any_hit, inst_masks=masks, ray_mask=ray_mask)
            b = nw.trace(ws["nodes"], ws["root_link"], ws["records"], pool, wpool, rays, any_hit)
            hit = b[0] >= 0
            # (the visible instances' own top-level tree is another tree: an any-hit ray may end on another triangle, so hit or miss
            # is compared there; a closest hit is decided by t, and no two hits of these rays tie)
            assert np.array_equal(a[0] >= 0, hit) and hit.sum() > 50
            if not any_hit:
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
                assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
                assert np.array_equal(a[4][hit], np.flatnonzero(keep)[b[4][hit]])
            assert a[5]["numInstancesMasked"] > 0 and b[5]["numInstancesMasked"] == 0
    miss = nw.trace(wt["nodes"], wt["root_link"], wt["records"], pool, wpool, rays, False, inst_masks=masks, ray_mask=0)
    assert (miss[0] == -1).all() and (miss[4] == -1).all() and miss[5]["numInstanceEntries"] == 0 and miss[5]["numTopInnerVisits"] > 0


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def test_spec_wide_structure():
    pool = isc.pool_of(["one", "nested90", "soup64"], gap_nodes=2, gap_rows=1)
    wpool = nw.widen_pool(pool)
    off = 0
    for (o, ext, num, bound), (n_off, n_bytes, _, _) in zip(wpool["ranges"], pool["ranges"]):
        single = bw.widen(pool["nodes"][n_off:n_off + n_bytes])
        assert o == off and o % 128 == 0 and ext == 128 * single["stats"]["numNodes"] and num == single["stats"]["numNodes"]
        assert bound == single["stats"]["stackBound"]
        assert wpool["nodes"][o:o + ext].tobytes() == single["nodes"].tobytes()      # links relative to the BLAS's own start
        off += ext
    assert wpool["stats"]["nodesBytes"] == off == wpool["nodes"].size and wpool["ranges"][1][3] == 89
    # the top level: np_bvh_wide.widen takes the TLAS as it is, and instance links pass through
    for name in ("three", "grid", "mirror"):
        sc, p, inst, t, wp, wt = _scene(name)
        links = wt["nodes"][:, 12:16].reshape(-1)
        assert sorted(~links[links < 0]) == list(range(inst.shape[0])) and wt["root_link"] == 0
        for i, b in enumerate(inst["blas"]):
            assert tuple(wt["records"][i, 12:16]) == (wp["ranges"][int(b)][0], p["ranges"][int(b)][2] // 16, wp["ranges"][int(b)][1], 0)
            assert wt["records"][i, :12].tobytes() == inst["worldToObject"][i].tobytes()
    # one instance: no node; an instance of a BLAS that is not there: extent 0, and nothing of it is read
    inst = ni.instances([ni.IDENTITY, ni.IDENTITY], [1, 0])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    one = nw.widen_tlas(np.zeros((0, 16), np.int32), ~0, inst[:1], pool["ranges"], wpool["ranges"])
    assert one["root_link"] == -1 and one["nodes"].shape == (0, 32) and one["stats"]["stackBound"] == 0 + 1 + 89
    bad = inst.copy()
    bad["blas"][1] = 7
    wt = nw.widen_tlas(t["nodes"], t["root_link"], bad, pool["ranges"], wpool["ranges"])
    assert tuple(wt["records"][1, 12:16]) == (0, 0, 0, 0) and wt["records"][0, 14] == wpool["ranges"][1][1]
    rays = isc.scene_rays((16, 8), 64)
    rid, _, _, _, rinst, cnt = nw.trace(wt["nodes"], wt["root_link"], wt["records"], pool, wpool, rays)
    assert (rinst != 1).all()
    # stackBound: the top level's + the marker + the pool's largest.  Two instances of nested90: 1 + 1 + 89
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0)), isc.transform(isc.rotation(np.random.default_rng(3)), 1.0, (0.1, 0, 0))])
    inst = ni.instances(tf, [1, 1])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    wt = nw.widen_tlas(t["nodes"], t["root_link"], inst, pool["ranges"], wpool["ranges"])
    assert (wt["stats"]["tlasStackBound"], wt["stats"]["stackBound"]) == (1, 91) and wt["stats"]["stackBound"] <= nw.MAX_STACK


def test_algorithmic_bytes_of_the_binding_are_the_specs():
    st = nt.InstancedWideTraceStats(*range(10, 90, 10))
    d = st.as_dict()
    for im in (False, True):
        for rm in (False, True):
            assert st.algorithmic_bytes(im, rm) == nw.algorithmic_bytes(d, im, rm)
    assert nw.algorithmic_bytes(d) == 52 * 10 + 112 * (20 + 50) + 96 * 30 + 48 * 60 + 16 * 70 + 4 * 80


# ---- argument tables ------------------------------------------------------------------------------------------------------------------------
def test_widen_argument_errors_and_no_device():
    """Pointers are never dereferenced by a refused call; the accepted call runs only where there is no device to run it on."""
    fake, fake2 = 0x10000, 0x4000000
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    assert nt.pool_widen_capacity(ranges) == 128 * 11 and nt.pool_widen_capacity(ranges[1:]) == 128
    for bad in ([], [(0, 0, 0, 16)], [(0, 100, 0, 16)], [(0, 0x76543240, 0, 16)]):
        with pytest.raises(nt.NtrError) as e:
            nt.pool_widen_capacity(bad)
        assert e.value.code == -1
    assert nt.lib().ntr_pool_widen_capacity(2, None, None) == -1
    good = dict(ranges=ranges, d_pool_nodes=fake, pool_nodes_bytes=704, d_wide_pool_nodes=fake2, capacity=128 * 11)
    bad_ranges = [[(32, 640, 0, 1600)], [(0, 96, 0, 1600)], [(0, 0, 0, 1600)], [(640, 128, 0, 1600)], [(0, 640, 8, 1600)], [(0, 640, 0, 1608)],
                  [(-64, 640, 0, 1600)], [(0, 640, -16, 1600)], [(0, 640, 0xFFFFFF00, 1600)], [(0, 640, 0, 0)]]
    cases = [dict(ranges=[]), dict(d_pool_nodes=0), dict(d_wide_pool_nodes=0), dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700),
             dict(pool_nodes_bytes=0xFFFFFF40), dict(capacity=128 * 11 - 1), dict(d_wide_pool_nodes=fake + 64)] + [dict(ranges=r) for r in bad_ranges]
    for change in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.pool_widen(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in ranges])
    out = (nt.WideBlasRange * 2)()
    res = nt.BvhWideResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert L.ntr_pool_widen(2, C.cast(arr, C.c_void_p), fake, 704, fake2, 128 * 11, None, C.byref(res), None) == -1
    assert bytes(res) == bytes(C.sizeof(res))
    assert L.ntr_pool_widen(2, C.cast(arr, C.c_void_p), fake, 704, fake2, 128 * 11, C.cast(out, C.c_void_p), None, None) == -1

    wide = [(0, 1280, 10, 5), (1280, 128, 1, 1)]
    tgood = dict(num_instances=5, d_instances=fake, d_tlas_nodes=fake, tlas_nodes_bytes=256, root_link=0, ranges=ranges, wide_ranges=wide,
                 d_wide_tlas_nodes=fake2, capacity=512, d_wide_records=fake2 + 4096, records_cap=320)
    bad_wide = [[(64, 1280, 10, 5), wide[1]], [(0, 1000, 10, 5), wide[1]], [(0, 0, 0, 0), wide[1]], [(0xFFFFFF00, 128, 1, 1), wide[1]],
                [(0, 1280, 10, -1), wide[1]], [(-128, 1280, 10, 5), wide[1]]]
    tcases = [dict(num_instances=0), dict(d_instances=0), dict(d_instances=fake + 4), dict(d_tlas_nodes=0), dict(tlas_nodes_bytes=0),
              dict(tlas_nodes_bytes=100), dict(root_link=64), dict(root_link=~5), dict(ranges=[]), dict(d_wide_tlas_nodes=0),
              dict(capacity=511), dict(d_wide_records=0), dict(d_wide_records=fake2 + 8), dict(records_cap=319),
              dict(ranges=[(0, 640, 8, 1600), ranges[1]]), dict(ranges=[(0, 640, -16, 1600), ranges[1]])] + [dict(wide_ranges=w) for w in bad_wide]
    for change in tcases:
        with pytest.raises(nt.NtrError) as e:
            nt.tlas_widen(**dict(tgood, **change))
        assert e.value.code == -1, (change, str(e.value))
    warr = (nt.WideBlasRange * 2)(*[nt.WideBlasRange(*w) for w in wide])
    tres = nt.TlasWideResult()
    C.memset(C.byref(tres), 0xFF, C.sizeof(tres))
    assert L.ntr_tlas_widen(5, fake, fake, 256, 0, 2, C.cast(arr, C.c_void_p), None, fake2, 512, fake2 + 4096, 320, C.byref(tres), None) == -1
    assert bytes(tres) == bytes(C.sizeof(tres))
    assert L.ntr_tlas_widen(5, fake, fake, 256, 0, 2, C.cast(arr, C.c_void_p), C.cast(warr, C.c_void_p), fake2, 512, fake2 + 4096, 320, None, None) == -1
    if not _has_device():
        for call in (lambda: nt.pool_widen(**good), lambda: nt.tlas_widen(**tgood),
                     lambda: nt.tlas_widen(**dict(tgood, num_instances=1, root_link=~0, d_tlas_nodes=0, d_wide_tlas_nodes=0, records_cap=64))):
            with pytest.raises(nt.NtrError) as e:
                call()
            assert e.value.code in (-2, -3), str(e.value)
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        rc = L.ntr_pool_widen(2, C.cast(arr, C.c_void_p), fake, 704, fake2, 128 * 11, C.cast(out, C.c_void_p), C.byref(res), None)
        assert rc in (-2, -3) and bytes(res) == bytes(C.sizeof(res)) and bytes(out) == bytes(C.sizeof(out))
        C.memset(C.byref(tres), 0xFF, C.sizeof(tres))
        rc = L.ntr_tlas_widen(5, fake, fake, 256, 0, 2, C.cast(arr, C.c_void_p), C.cast(warr, C.c_void_p), fake2, 512, fake2 + 4096, 320,
                              C.byref(tres), None)
        assert rc in (-2, -3) and bytes(tres) == bytes(C.sizeof(tres))


@pytest.mark.parametrize("stats", [False, True])
def test_trace_instanced_wide_argument_errors_and_no_device(stats):
    fake = 0x10000
    call = nt.trace_instanced_wide_stats if stats else nt.trace_instanced_wide
    good = dict(num_rays=64, any_hit=False, d_rays=fake, d_results=fake, d_instance_ids=fake, d_wide_tlas_nodes=fake, wide_tlas_nodes_bytes=256,
                root_link=0, d_wide_records=fake, num_instances=5, d_wide_pool_nodes=fake, wide_pool_nodes_bytes=1408, d_pool_woop=fake,
                pool_woop_bytes=1680, d_pool_tri_index=fake)
    for change in (dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_instance_ids=0), dict(d_wide_records=0), dict(num_instances=0),
                   dict(root_link=128), dict(root_link=~5), dict(wide_tlas_nodes_bytes=0), dict(wide_tlas_nodes_bytes=192),
                   dict(wide_tlas_nodes_bytes=0x76543280), dict(d_wide_tlas_nodes=0), dict(d_wide_pool_nodes=0), dict(wide_pool_nodes_bytes=0),
                   dict(wide_pool_nodes_bytes=1344), dict(wide_pool_nodes_bytes=0xFFFFFF80), dict(pool_woop_bytes=8),
                   dict(pool_woop_bytes=0xFFFFFF10), dict(d_pool_tri_index=0), dict(vis=nt.InstanceVisibility(fake + 2, 0)),
                   dict(vis=nt.InstanceVisibility(0, fake + 1))):
        with pytest.raises(nt.NtrError) as e:
            call(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    zero = call(**dict(good, num_rays=0))
    assert (zero.as_dict() == dict.fromkeys(nt.InstancedWideTraceStats().as_dict(), 0)) if stats else zero == 0.0
    if stats:
        L = nt.lib()
        assert L.ntr_trace_instanced_wide_stats(64, 0, fake, fake, fake, fake, 256, 0, fake, 5, fake, 1408, fake, 1680, fake, None, None, None) == -1
    if not _has_device():
        for kw in (good, dict(good, root_link=~0, d_wide_tlas_nodes=0, wide_tlas_nodes_bytes=0), dict(good, vis=nt.InstanceVisibility(fake, fake, 3))):
            with pytest.raises(nt.NtrError) as e:
                call(**kw)
            assert e.value.code in (-2, -3), str(e.value)
