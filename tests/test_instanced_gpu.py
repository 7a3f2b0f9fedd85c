"""Instanced scenes on the device: ntr_tlas_build equals the numpy spec (tests/np_instanced.py) in nodes, records, rootLink, scene box,
rounds and height at every size where the build takes another path; ntr_trace_instanced equals the spec in all four result words and the
instance id for closest hit and any hit; one identity instance gives ntr_trace_bvh's records; two runs give the same bytes, the scratch
pool is released, the status word stays clear; argument errors found on the device are reported.  Output buffers are prefilled with
0xAB and nothing beyond the result's extents may be written."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_instanced as ni
import sah_sweep_scenes as ss
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
TAIL, TILE = nt.PLOC_TAIL, nt.PLOC_TILE
_cache = {}


def _filled(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xAB, dtype=torch.uint8, device="cuda:0")


class _Scene:
    """A pool and instances on the device; build() makes the top-level tree into 0xAB-filled buffers of tlas_capacity bytes."""

    def __init__(self, pool, inst, radius=8, build=True):
        self.pool, self.inst, self.n = pool, inst, inst.shape[0]
        self.d_nodes, self.d_woop, self.d_idx = up(pool["nodes"]), up(pool["woop"]), up(pool["tri_index"])
        self.d_inst = up(inst)
        self.caps = nt.tlas_capacity(self.n)
        if build:
            self.build(radius)

    def build(self, radius=8):
        self.d_tlas, self.d_rec = _filled(self.caps[0] + 64), _filled(self.caps[1] + 64)
        self.res = nt.tlas_build(self.n, self.d_inst.data_ptr(), self.pool["ranges"], self.d_nodes.data_ptr(), self.pool["nodes"].size,
                                 self.d_tlas.data_ptr(), self.caps[0], self.d_rec.data_ptr(), self.caps[1], radius)
        torch.cuda.synchronize()
        r = self.res
        raw = self.d_tlas.cpu().numpy(), self.d_rec.cpu().numpy()
        for x, e in zip(raw, (r.nodesBytes, r.recordsBytes)):
            assert 0 <= e <= x.size and (x[e:] == 0xAB).all(), "bytes beyond the result's extents were written"
        self.tlas = raw[0][:r.nodesBytes].view(np.int32).reshape(-1, 16).copy()
        self.records = raw[1][:r.recordsBytes].view(np.uint32).reshape(-1, 16).copy()
        return self

    def trace(self, rays, any_hit, tlas=None):
        """-> (results as nt.RESULT_DTYPE, instance ids); tlas: (nodes, root_link, records) arrays to trace instead of the device build's."""
        n = rays.shape[0]
        d_rays = up(rays)
        d_res, d_ids = _filled(16 * n + 64), _filled(4 * n + 64)
        if tlas is None:
            args = (self.d_tlas.data_ptr(), self.res.nodesBytes, self.res.rootLink, self.d_rec.data_ptr())
        else:
            self._keep = up(tlas[0]) if tlas[0].size else _filled(64), up(tlas[2])
            args = (self._keep[0].data_ptr(), tlas[0].nbytes, tlas[1], self._keep[1].data_ptr())
        sec = nt.trace_instanced(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), *args, self.n, self.d_nodes.data_ptr(),
                                 self.pool["nodes"].size, self.d_woop.data_ptr(), self.pool["woop"].size, self.d_idx.data_ptr())
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all(), "bytes beyond the rays' results were written"
        self.seconds = sec
        return res[:16 * n].view(nt.RESULT_DTYPE).copy(), ids[:4 * n].view(np.int32).copy()


def _assert_tlas_equals_spec(s, radius=8, what=""):
    ref = ni.tlas_build(s.pool["nodes"], s.pool["ranges"], s.inst, radius)
    r = s.res
    assert r.rootLink == ref["root_link"], (r.rootLink, what)
    assert np.array_equal(s.records, ref["records"]), ("records differ", what)
    assert np.array_equal(s.tlas, ref["nodes"]), ("nodes differ", what, int(np.flatnonzero((s.tlas != ref["nodes"]).any(axis=1))[0]))
    assert np.array_equal(np.array(list(r.sceneMin), F).view(np.uint32), ref["scene_min"].view(np.uint32)), what
    assert np.array_equal(np.array(list(r.sceneMax), F).view(np.uint32), ref["scene_max"].view(np.uint32)), what
    got = dict(numNodes=r.numNodes, numRounds=r.numRounds, height=r.height, tailClusters=r.tailClusters)
    assert got == ref["stats"], (got, ref["stats"], what)
    assert r.nodesBytes == ref["nodes"].nbytes and r.recordsBytes == ref["records"].nbytes
    return ref


def _assert_trace_equals_spec(s, rays, what="", tlas=None):
    t = tlas or (s.tlas, s.res.rootLink, s.records)
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst = ni.trace(t[0], t[1], t[2], s.pool, rays, any_hit)
        got, ids = s.trace(rays, any_hit, tlas)
        gid, gt, gu, gv = isc.result_words(got)
        for name, g, e in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                           ("instance", ids, rinst)):
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, "%s anyHit=%d: %d %s mismatches of %d rays, first at ray %d: %r != %r" % (
                what, any_hit, bad.size, name, rays.shape[0], bad[0], g[bad[0]], e[bad[0]])
    return rid


def _three_blas_pool():
    return isc.pool_of(["cornell", "soup1000", "one"], gap_nodes=1, gap_rows=3)


def _seeded(n, seed, radius=8):
    pool = _three_blas_pool()
    rng = np.random.default_rng(seed)
    inst = ni.instances(isc.seeded_transforms(n, seed, mirrored=min(n, 3)), rng.integers(0, 3, n))
    return _Scene(pool, inst, radius)


def _named(name):
    if name not in _cache:
        sc = isc.scene(name)
        _cache[name] = _Scene(isc.pool_of(sc["names"]), ni.instances(sc["transforms"], sc["blas"]))
    return _cache[name]


# ---- the top-level build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, TAIL - 1, TAIL, TAIL + 1, 2 * TILE + 1])
def test_tlas_equals_spec(n):
    s = _seeded(n, 100 + n)
    _assert_tlas_equals_spec(s, 8, n)
    assert (s.res.tailClusters == n) == (1 < n <= TAIL)
    r = s.res
    print("N=%d: %d rounds, height %d, %.3f ms (boxes %.3f, sort %.3f, clusters %.3f, rounds %.3f, tail %.3f)"
          % (n, r.numRounds, r.height, r.seconds * 1e3, r.boxesMs, r.sortMs, r.clustersMs, r.roundsMs, r.tailMs))


@pytest.mark.parametrize("radius", [1, 64])
@pytest.mark.parametrize("n", [65, TAIL + 1])
def test_tlas_equals_spec_at_other_radii(n, radius):
    _assert_tlas_equals_spec(_seeded(n, 100 + n, radius), radius, (n, radius))


@pytest.mark.parametrize("n", [40, 1100])
def test_identical_instances_pair_up(n):
    """Equal boxes, equal codes, equal distances: the b term pairs them (0,1) (2,3) ..., at 1100 across a tile edge."""
    pool = _three_blas_pool()
    inst = ni.instances(np.tile(isc.transform(np.eye(3), 1.5, (1.0, 2.0, 3.0)), (n, 1)), np.ones(n, np.int32))
    s = _Scene(pool, inst)
    ref = _assert_tlas_equals_spec(s, 8, n)
    assert ref["stats"]["numRounds"] == int(np.ceil(np.log2(n)))


# ---- the two-level trace ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_trace_equals_spec_on_the_scenes(name):
    s = _named(name)
    _assert_tlas_equals_spec(s, 8, name)
    prim, _ = scenes.primary_rays(isc.CAMERA, 128, 64)
    rays = np.concatenate([prim, scenes.random_rays(4096, 5, extent=12.0), isc.finite_edge_rays(), isc.odd_rays()])
    rid = _assert_trace_equals_spec(s, rays, name)
    assert (rid >= 0).sum() > rays.shape[0] // 8
    print("%s: %d rays, %d hits, %.3f ms" % (name, rays.shape[0], int((rid >= 0).sum()), s.seconds * 1e3))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ray_counts(n):
    _assert_trace_equals_spec(_named("three"), isc.scene_rays((8, 8), 1000)[:n], n)


def test_1025_instances_of_a_small_soup():
    pool = isc.pool_of(["soup100"])
    inst = ni.instances(isc.seeded_transforms(TAIL + 1, 31, spread=12.0, mirrored=5, size=0.1), np.zeros(TAIL + 1, np.int32))
    s = _Scene(pool, inst)
    _assert_tlas_equals_spec(s, 8, "1025")
    rays = isc.scene_rays((64, 32), 2048)
    rid = _assert_trace_equals_spec(s, rays, "1025")
    assert (rid >= 0).sum() > 1000 and np.unique(s.trace(rays, False)[1]).size > 300


def test_a_pool_of_device_ploc_trees_and_an_uploaded_sah_tree():
    """Two BLASes built by ntr_ploc_build straight into pool + offset, one host SAH tree (leaves of several triangles) copied in."""
    meshes = [ss.scene("soup1000"), ss.scene("cornell")]
    sah = nt.sah_build(*ss.scene("soup64"))
    bp = nt.BlasPool()
    slots = [bp.add(*nt.lbvh_capacity(t.shape[0])[:2]) for t, _ in meshes] + [bp.add(sah.nodes.nbytes, sah.woop.nbytes)]
    d_nodes, d_woop, d_idx = (torch.zeros(b, dtype=torch.uint8, device="cuda:0") for b in (bp.nodes_bytes, bp.woop_bytes, bp.tri_index_bytes))
    ranges = []
    for (tri, pos), (k, no, wo) in zip(meshes, slots):
        d_tri, d_pos = up(tri), up(pos)
        caps = nt.lbvh_capacity(tri.shape[0])
        mn, mx = pos.min(axis=0), pos.max(axis=0)
        r = nt.ploc_build(tri.shape[0], d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, d_nodes.data_ptr() + no, caps[0],
                          d_woop.data_ptr() + wo, caps[1], d_idx.data_ptr() + wo // 4, caps[2])
        ranges.append((no, r.nodesBytes, wo, r.triWoopBytes))
    k, no, wo = slots[2]
    d_nodes[no:no + sah.nodes.nbytes] = up(sah.nodes)
    d_woop[wo:wo + sah.woop.nbytes] = up(sah.woop)
    d_idx[wo // 4:wo // 4 + sah.tri_index.nbytes] = up(sah.tri_index)
    ranges.append((no, sah.nodes.nbytes, wo, sah.woop.nbytes))
    torch.cuda.synchronize()
    pool = dict(nodes=d_nodes.cpu().numpy(), woop=d_woop.cpu().numpy(), tri_index=d_idx.cpu().numpy().view(np.int32), ranges=ranges)
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0)), isc.transform(isc.rotation(np.random.default_rng(3)), 0.02, (-5, -5, 4)),
                   isc.transform(isc.rotation(np.random.default_rng(4)), (1.5, -1.0, 0.8), (3, 2, -2))])
    s = _Scene(pool, ni.instances(tf, [0, 1, 2]))
    _assert_tlas_equals_spec(s, 8, "mixed")
    rid = _assert_trace_equals_spec(s, isc.scene_rays((64, 64), 2048), "mixed")
    hit_inst = s.trace(isc.scene_rays((64, 64), 2048), False)[1]
    assert set(np.unique(hit_inst)) == {-1, 0, 1, 2} and (rid >= 0).any()


def test_two_identical_instances_at_one_place_tie_by_visiting_order():
    pool = isc.pool_of(["soup1000"])
    s = _Scene(pool, ni.instances(np.tile(isc.transform(np.eye(3), 1.0, (0.5, 0, 0)), (2, 1)), [0, 0]))
    rays = isc.scene_rays((64, 32), 1024)
    _assert_trace_equals_spec(s, rays, "twins")
    ids = s.trace(rays, False)[1]
    assert (ids >= 0).any() and (ids[ids >= 0] == 0).all()   # child 0 first, and an equal t does not replace a hit


def test_a_deep_blas_instanced_twice_runs_past_the_lds_stack():
    pool = isc.pool_of(["nested90"])
    assert isc.blas("nested90")[2]["stats"]["height"] == 89
    tf = np.stack([isc.transform(np.eye(3), 1.0, (0, 0, 0)), isc.transform(isc.rotation(np.random.default_rng(8)), 1.0, (0.25, 0.25, 0))])
    s = _Scene(pool, ni.instances(tf, [0, 0]))
    rng = np.random.default_rng(2)
    rays = scenes.random_rays(1000, 6, extent=1.0)
    for k in ("ox", "oy", "oz"):
        rays[k] = (rng.uniform(0, 1, 1000) ** 8 * 4.0).astype(F)   # most origins near the small end of the chain
    rays["oz"] -= F(2.0)
    rays["dx"], rays["dy"], rays["dz"] = rng.normal(0, 0.1, 1000).astype(F), rng.normal(0, 0.1, 1000).astype(F), F(1.0)
    rid = _assert_trace_equals_spec(s, rays, "nested")
    assert (rid >= 0).any()


# ---- identity -----------------------------------------------------------------------------------------------------------------------
def test_one_identity_instance_gives_the_single_level_records():
    tri, pos, b = isc.blas("soup1000")
    pool = isc.pool_of(["soup1000"])
    s = _Scene(pool, ni.instances([ni.IDENTITY], [0]))
    assert s.res.rootLink == -1 and s.res.numNodes == 0 and s.res.nodesBytes == 0
    cam = scenes.random_soup(1000, seed=1100, walls=False)[2]
    rays = np.concatenate([scenes.primary_rays(cam, 128, 64)[0], scenes.random_rays(4096, 3)])
    view = nt.BvhView(s.d_nodes.data_ptr(), pool["nodes"].size, s.d_woop.data_ptr(), pool["woop"].size, s.d_idx.data_ptr())
    d_rays = up(rays)
    for any_hit in (False, True):
        d_res = _filled(16 * rays.shape[0])
        view.trace("fermi_speculative_while_while", rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr())
        torch.cuda.synchronize()
        want = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
        got, ids = s.trace(rays, any_hit)
        assert got.tobytes() == want.tobytes(), any_hit
        assert np.array_equal(ids, np.where(want["id"] >= 0, 0, -1))


# ---- determinism and scratch --------------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.tlas_scratch_bytes() == 0
    a = _seeded(2 * TILE + 1, 7)
    held = nt.tlas_scratch_bytes()
    assert held > 0
    tl, rec = a.tlas.copy(), a.records.copy()
    a.build()
    assert nt.tlas_scratch_bytes() == held
    assert a.tlas.tobytes() == tl.tobytes() and a.records.tobytes() == rec.tobytes()
    rays = isc.scene_rays((32, 32), 1024)
    r1, r2 = a.trace(rays, False), a.trace(rays, False)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()
    nt.lbvh_release_workspace()
    assert nt.tlas_scratch_bytes() == 0
    a.build()
    assert a.tlas.tobytes() == tl.tobytes()
    nt.lbvh_release_workspace()


# ---- argument errors found with a device ----------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device():
    pool = _three_blas_pool()
    inst = ni.instances(isc.seeded_transforms(5, 3), [0, 1, 2, 1, 0])
    s = _Scene(pool, inst, build=False)
    d_tlas, d_rec = _filled(s.caps[0]), _filled(s.caps[1])
    good = dict(num_instances=5, d_instances=s.d_inst.data_ptr(), ranges=pool["ranges"], d_pool_nodes=s.d_nodes.data_ptr(),
                pool_nodes_bytes=pool["nodes"].size, d_tlas_nodes=d_tlas.data_ptr(), tlas_nodes_cap=s.caps[0], d_records=d_rec.data_ptr(),
                records_cap=s.caps[1])
    r0 = pool["ranges"][1]
    misaligned = [pool["ranges"][0], (r0[0] + 32, r0[1], r0[2], r0[3]), pool["ranges"][2]]
    outside = [pool["ranges"][0], (pool["nodes"].size, 64, r0[2], r0[3]), pool["ranges"][2]]
    odd_rows = [pool["ranges"][0], (r0[0], r0[1], r0[2] + 8, r0[3]), pool["ranges"][2]]
    for change in (dict(tlas_nodes_cap=s.caps[0] - 1), dict(records_cap=s.caps[1] - 1), dict(ranges=misaligned), dict(ranges=outside),
                   dict(ranges=odd_rows), dict(radius=0), dict(radius=65), dict(num_instances=0), dict(d_records=0)):
        with pytest.raises(nt.NtrError) as e:
            nt.tlas_build(**dict(good, **change))
        assert e.value.code == -1, (change, str(e.value))
    torch.cuda.synchronize()
    assert (d_tlas.cpu().numpy() == 0xAB).all() and (d_rec.cpu().numpy() == 0xAB).all()   # refused before any device work
    for bad_index in (3, -1):
        bad = inst.copy()
        bad["blas"][2] = bad_index
        d_bad = up(bad)
        res = nt.TlasResult()
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        arr = (nt.BlasRange * 3)(*[nt.BlasRange(*r) for r in pool["ranges"]])
        rc = nt.lib().ntr_tlas_build(5, d_bad.data_ptr(), 3, C.cast(arr, C.c_void_p), s.d_nodes.data_ptr(), pool["nodes"].size, 8, d_tlas.data_ptr(),
                                     s.caps[0], d_rec.data_ptr(), s.caps[1], C.byref(res), None)
        assert rc == -1 and b"blas index" in nt.lib().ntr_last_error() and bytes(res) == bytes(C.sizeof(res))
    r = nt.tlas_build(**good)
    assert (r.numNodes, r.rootLink, r.tailClusters) == (4, 0, 5) and r.seconds > 0
