"""Instanced scenes without a device: ntr_instance_invert equals np_instanced.invert bit for bit; ntr_tlas_build refuses bad arguments
and, without a device, reports that with a zeroed result; the spec's two-level trace through one identity instance equals np_tracer on
the BLAS alone; and against a binary64 brute force over the flattened world-space triangles the instanced spec is no worse than twice
what binary32 and grazing rays cost the single-level tracer on the flattened mesh."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_hlbvh
import np_instanced as ni
import np_tracer

F = np.float32


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


# ---- ntr_instance_invert ------------------------------------------------------------------------------------------------------------
def test_instance_invert_equals_spec():
    ms = list(isc.seeded_transforms(200, 20261018, mirrored=0)) + [isc.transform(isc.rotation(np.random.default_rng(1)), (-2.0, 0.5, 3.0), (7, -8, 9))]
    for m in ms:
        got, want = nt.instance_invert(m), ni.invert(m)
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32)), m
        # and it is an inverse: worldToObject x objectToWorld is the identity to binary32's precision
        a, b = np.vstack([want.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]), np.vstack([m.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
        assert np.abs(a @ b - np.eye(4)).max() < 1e-4
    assert np.linalg.det(ms[-1].reshape(3, 4)[:, :3].astype(np.float64)) < 0


def test_instance_invert_refuses_a_singular_matrix():
    for m in (np.zeros(12, F), np.array([1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0], F), np.array([np.inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F),
              np.array([np.nan, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)):
        with pytest.raises(nt.NtrError) as e:
            nt.instance_invert(m)
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ni.invert(m)
    out = np.zeros(12, F)
    assert nt.lib().ntr_instance_invert(None, out.ctypes.data) == -1 and nt.lib().ntr_instance_invert(out.ctypes.data, None) == -1


# ---- ntr_tlas_build's argument table --------------------------------------------------------------------------------------------------
def test_tlas_build_argument_errors_and_no_device():
    """Pointers are never dereferenced by a refused call; the accepted call runs only where there is no device to run it on."""
    fake = 0x10000
    caps = nt.tlas_capacity(5)
    assert caps == (4 * 64, 5 * 64) and nt.tlas_capacity(1) == (64, 64)
    with pytest.raises(nt.NtrError):
        nt.tlas_capacity(0)
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    good = dict(num_instances=5, d_instances=fake, ranges=ranges, d_pool_nodes=fake, pool_nodes_bytes=704, d_tlas_nodes=fake,
                tlas_nodes_cap=caps[0], d_records=fake, records_cap=caps[1], radius=8)
    bad_ranges = [[(32, 640, 0, 1600)], [(0, 96, 0, 1600)], [(0, 0, 0, 1600)], [(640, 128, 0, 1600)], [(0, 640, 8, 1600)], [(0, 640, 0, 1608)],
                  [(-64, 640, 0, 1600)], [(0, 640, -16, 1600)], [(0, 640, 0xFFFFFF00, 1600)], [(0, 640, 0, 0)]]
    cases = [dict(num_instances=0), dict(num_instances=-3), dict(radius=0), dict(radius=65), dict(d_instances=0), dict(d_pool_nodes=0),
             dict(d_tlas_nodes=0), dict(d_records=0), dict(ranges=[]), dict(tlas_nodes_cap=caps[0] - 1), dict(records_cap=caps[1] - 1),
             dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700), dict(pool_nodes_bytes=0xFFFFFF40)] + [dict(ranges=r) for r in bad_ranges]
    for change in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.tlas_build(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    # a BLAS above Compact's limit, in a pool that could hold it
    with pytest.raises(nt.NtrError) as e:
        nt.tlas_build(**dict(good, pool_nodes_bytes=0xFFFFFF00, ranges=[(0, 0x76543240, 0, 1600)]))
    assert e.value.code == -1
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in ranges])
    res = nt.TlasResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert L.ntr_tlas_build(5, fake, 2, None, fake, 704, 8, fake, caps[0], fake, caps[1], C.byref(res), None) == -1
    assert bytes(res) == bytes(C.sizeof(res))
    assert L.ntr_tlas_build(5, fake, 2, C.cast(arr, C.c_void_p), fake, 704, 8, fake, caps[0], fake, caps[1], None, None) == -1
    assert L.ntr_tlas_scratch_bytes(None) == -1
    if not _has_device():
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        rc = L.ntr_tlas_build(5, fake, 2, C.cast(arr, C.c_void_p), fake, 704, 8, fake, caps[0], fake, caps[1], C.byref(res), None)
        assert rc == -2, (rc, L.ntr_last_error())
        assert bytes(res) == bytes(C.sizeof(res))
        with pytest.raises(nt.NtrError) as e:
            nt.trace_instanced(64, False, fake, fake, fake, fake, 256, 0, fake, 5, fake, 704, fake, 1680, fake)
        assert e.value.code in (-2, -3)
    # ntr_trace_instanced refuses what it can see
    tgood = dict(num_rays=64, any_hit=False, d_rays=fake, d_results=fake, d_instance_ids=fake, d_tlas_nodes=fake, tlas_nodes_bytes=256, root_link=0,
                 d_records=fake, num_instances=5, d_pool_nodes=fake, pool_nodes_bytes=704, d_pool_woop=fake, pool_woop_bytes=1680, d_pool_tri_index=fake)
    for change in (dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_instance_ids=0), dict(d_records=0), dict(num_instances=0),
                   dict(root_link=64), dict(root_link=~5), dict(tlas_nodes_bytes=0), dict(tlas_nodes_bytes=100), dict(d_tlas_nodes=0),
                   dict(pool_nodes_bytes=0), dict(pool_woop_bytes=8), dict(pool_woop_bytes=0xFFFFFF10), dict(d_pool_tri_index=0)):
        with pytest.raises(nt.NtrError) as e:
            nt.trace_instanced(**dict(tgood, **change))
        assert e.value.code == -1, (change, str(e.value))
    assert nt.trace_instanced(**dict(tgood, num_rays=0)) == 0.0


def test_blas_pool_hands_out_aligned_ranges():
    bp = nt.BlasPool()
    assert bp.add(100, 40) == (0, 0, 0) and bp.add(64, 16) == (1, 128, 48) and bp.add(640, 1600) == (2, 192, 64)
    assert bp.ranges == [(0, 128, 0, 48), (128, 64, 48, 16), (192, 640, 64, 1600)]
    assert (bp.nodes_bytes, bp.woop_bytes, bp.tri_index_bytes) == (832, 1664, 416)
    assert nt.INSTANCE_DTYPE.itemsize == 112 and nt.INSTANCE_DTYPE == ni.INSTANCE_DTYPE
    inst = nt.make_instances(isc.seeded_transforms(4, 2), [0, 1, 2, 1])
    assert inst.tobytes() == ni.instances(isc.seeded_transforms(4, 2), [0, 1, 2, 1]).tobytes()


# ---- the spec itself ------------------------------------------------------------------------------------------------------------------
def test_spec_tlas_structure():
    pool = isc.pool_of(["cornell", "soup64", "one"], gap_nodes=2, gap_rows=1)
    for n in (1, 2, 7, 300):
        inst = ni.instances(isc.seeded_transforms(n, n), np.arange(n) % 3)
        t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
        assert t["records"].shape == (n, 16) and (t["records"][:, 15] == 0).all()
        for i in range(n):
            r = pool["ranges"][int(inst["blas"][i])]
            assert tuple(t["records"][i, 12:15]) == (r[0], r[2] // 16, r[1])
        if n == 1:
            assert t["root_link"] == -1 and t["nodes"].shape == (0, 16) and t["stats"]["height"] == 0
            continue
        links = t["nodes"][:, 12:14].reshape(-1)
        assert t["root_link"] == 0 and sorted(~links[links < 0]) == list(range(n))            # every instance is a leaf exactly once
        assert sorted(links[links >= 0] // 64) == list(range(1, n - 1))                         # every node but the root is a child once
        lo, hi = np_hlbvh.f2i(t["scene_min"]), np_hlbvh.f2i(t["scene_max"])
        root = t["nodes"][0].view(F)
        assert np.array_equal(np.minimum(np_hlbvh.f2i(root[[0, 2, 8]]), np_hlbvh.f2i(root[[4, 6, 10]])), lo)
        assert np.array_equal(np.maximum(np_hlbvh.f2i(root[[1, 3, 9]]), np_hlbvh.f2i(root[[5, 7, 11]])), hi)
    # the one-triangle BLAS's empty child drops out of the union: the box is the triangle's
    lo, hi = ni.instance_box(pool["nodes"], pool["ranges"][2], ni.IDENTITY)
    pos = isc.blas("one")[1]
    assert np.array_equal(lo, pos.min(axis=0)) and np.array_equal(hi, pos.max(axis=0))


def test_spec_identity_instance_equals_the_single_level_tracer():
    tri, pos, b = isc.blas("soup1000")
    pool = isc.pool_of(["soup1000"])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], ni.instances([ni.IDENTITY], [0]))
    cam = scenes.random_soup(1000, seed=1100, walls=False)[2]
    rays = np.concatenate([scenes.random_rays(4096, 3), scenes.primary_rays(cam, 128, 64)[0]])
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst = ni.trace(t["nodes"], t["root_link"], t["records"], pool, rays, any_hit)
        eid, et = np_tracer.trace(b["nodes"], b["woop"], b["tri_index"], rays, any_hit=any_hit)
        assert np.array_equal(rid, eid)
        if not any_hit:
            assert np.array_equal(rt.view(np.uint32), et.view(np.uint32))
        assert np.array_equal(rinst, np.where(eid >= 0, 0, -1))
        assert (ru[rid < 0] == 0).all() and (rv[rid < 0] == 0).all() and (rid >= 0).sum() > 2000


def test_spec_stack_limit_is_the_devices():
    pool = isc.pool_of(["nested90"])
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0))] * 2)
    t = ni.tlas_build(pool["nodes"], pool["ranges"], ni.instances(tf, [0, 0]))
    rays = np.zeros(1, nt.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"], rays["dz"], rays["tmax"] = 0.3, 0.2, -2.0, 1.0, 1e30
    rays["dx"] = rays["dy"] = 0.01
    rid = ni.trace(t["nodes"], t["root_link"], t["records"], pool, rays)[0]
    assert rid[0] >= 0 and ni.MAX_STACK == 104 and ni.EXIT_MARKER > ni.SENTINEL


@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_spec_against_binary64_brute_force(name):
    """The yardstick is the single-level np_tracer on the flattened mesh (tree by np_bvh_ploc.build) against the same brute force: its
    share of rays with another hit / miss status and its largest relative t error are what binary32 and grazing rays cost without
    instancing.  The instanced spec may disagree on at most twice that share plus four rays, at four times that t tolerance: two
    roundings of the ray instead of none."""
    sc = isc.scene(name)
    pool = isc.pool_of(sc["names"])
    inst = ni.instances(sc["transforms"], sc["blas"])
    t = ni.tlas_build(pool["nodes"], pool["ranges"], inst)
    rays = isc.scene_rays((96, 64), 2048)
    verts, who = isc.flatten(sc)
    hit_b, t_b = isc.brute_force(verts, rays)
    pos32 = verts.reshape(-1, 3).astype(F)
    tri = np.arange(pos32.shape[0], dtype=np.int32).reshape(-1, 3)
    flat = pl.build(tri, pos32, *pl.scene_box(pos32), 8)
    fid, ft = np_tracer.trace(flat["nodes"], flat["woop"], flat["tri_index"], rays)
    rid, rt, _, _, rinst = ni.trace(t["nodes"], t["root_link"], t["records"], pool, rays)

    def against_brute(hit, tt, tol):
        both = hit & hit_b
        rel = np.abs(tt[both].astype(np.float64) - t_b[both]) / np.abs(t_b[both])
        status = int((hit != hit_b).sum())
        return status, (float(rel.max()) if rel.size else 0.0), status + (int((rel > tol).sum()) if tol is not None else 0)

    f_status, f_err, f_bad = against_brute(fid >= 0, ft, None)
    i_status, i_err, i_bad = against_brute(rid >= 0, rt, 4.0 * f_err)
    print("%s: %d rays, %d hit; flat tracer: %d status mismatches, largest relative t error %.3g; instanced spec: %d status mismatches, "
          "largest relative t error %.3g, %d rays beyond the tolerance %.3g"
          % (name, rays.shape[0], int(hit_b.sum()), f_status, f_err, i_status, i_err, i_bad - i_status, 4.0 * f_err))
    assert hit_b.sum() > rays.shape[0] // 8
    assert i_bad <= 2 * f_bad + 4, (i_bad, f_bad)
    # a hit names the instance and the triangle the brute force would name, wherever the two agree on t
    hit = (rid >= 0) & hit_b
    assert (rinst[hit] >= 0).all() and (rinst[rid < 0] == -1).all()
