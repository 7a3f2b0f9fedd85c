"""ntr_ploc_build_batch on the device: the pool, the ranges and the per-mesh counts equal the numpy spec (tests/np_ploc_batch.py:
np_bvh_ploc.build per mesh, np_instanced.make_pool over the results) byte for byte at every shape where the segmented kernels can go
wrong -- one mesh against ntr_ploc_build itself, segment edges inside a tile, inside a halo and on a tile edge, meshes shorter than the
radius, one-triangle meshes first, last and adjacent, meshes that finish in different rounds, more meshes than one workgroup of the
per-mesh kernel, ties, overlapping triangle ranges.  The ranges feed ntr_tlas_build and ntr_trace_instanced; two calls give the same
bytes and the scratch pool is released; errors found on the device are reported.  Pool buffers are prefilled with 0xAB and nothing beyond
the extents may be written."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_instanced as ni
import np_ploc_batch as pb
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
TILE = nt.PLOC_TILE
SLACK = 256


def _woop_equal(got, exp):
    """Words that are NaN on both sides compare equal (a NaN that arithmetic produces carries the processor's sign and payload), every
    other word by bits: test_bvh_ploc_gpu.py's rule."""
    got, exp = got.view(np.uint32), exp.view(np.uint32)
    return got.shape == exp.shape and bool(((got == exp) | (np.isnan(got.view(F)) & np.isnan(exp.view(F)))).all())


class _Batch:
    """A device batch build into pool buffers of ntr_ploc_batch_capacity bytes plus slack, all filled with 0xAB."""

    def __init__(self, meshes, tri, pos, radius=8, expect=None):
        self.meshes, self.tri, self.pos, self.radius = meshes, np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F), radius
        self.d_tri, self.d_pos = up(self.tri), up(self.pos)
        self.caps = nt.ploc_batch_capacity(meshes)
        self.bufs = [torch.full((c + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in self.caps[:3]]
        args = (meshes, self.tri.shape[0], self.d_tri.data_ptr(), self.pos.shape[0], self.d_pos.data_ptr(), self.bufs[0].data_ptr(), self.caps[0],
                self.bufs[1].data_ptr(), self.caps[1], self.bufs[2].data_ptr(), self.caps[2], radius)
        self.error = None
        if expect is None:
            self.res, self.ranges, self.mesh_results = nt.ploc_build_batch(*args)
        else:
            with pytest.raises(nt.NtrError) as e:
                nt.ploc_build_batch(*args)
            assert e.value.code == expect, str(e.value)
            self.error, self.res, self.ranges, self.mesh_results = e.value, None, e.value.ranges, e.value.mesh_results
        torch.cuda.synchronize()
        raw = [b.cpu().numpy() for b in self.bufs]
        for x, c in zip(raw, self.caps[:3]):
            assert (x[c:] == 0xAB).all(), "bytes beyond the pool's extents were written"
        self.nodes, self.woop, self.idx = raw[0][:self.caps[0]], raw[1][:self.caps[1]], raw[2][:self.caps[2]].view(np.int32)

    def assert_equals_spec(self, what=""):
        ref = pb.build(self.meshes, self.tri, self.pos, self.radius)
        assert self.ranges == ref["ranges"] == self.caps[3], what
        assert (self.caps[0], self.caps[1], self.caps[2]) == (ref["nodes"].size, ref["woop"].size, 4 * ref["tri_index"].size), what
        for k, (no, nb, wo, wb) in enumerate(ref["ranges"]):   # mesh by mesh, so that a failure names the mesh
            assert np.array_equal(self.nodes[no:no + nb], ref["nodes"][no:no + nb]), ("nodes differ", what, k, self.meshes[k][:2])
            assert np.array_equal(self.idx[wo // 16:(wo + wb) // 16], ref["tri_index"][wo // 16:(wo + wb) // 16]), ("triIndex differs", what, k)
            assert _woop_equal(self.woop[wo:wo + wb], ref["woop"][wo:wo + wb]), ("triWoop differs", what, k)
        got = [m.as_dict() for m in self.mesh_results]
        assert got == ref["stats"], (what, [(k, g, s) for k, (g, s) in enumerate(zip(got, ref["stats"])) if g != s][:3])
        if self.res is not None:
            r = self.res
            assert (r.numMeshes, r.numTris) == (len(self.meshes), sum(m[1] for m in self.meshes))
            assert (r.nodesBytes, r.triWoopBytes, r.triIndexBytes) == self.caps[:3]
            assert r.numRounds == max(s["numRounds"] for s in ref["stats"]) and r.maxHeight == max(s["height"] for s in ref["stats"])
        return ref


def _soup(n, seed):
    return scenes.random_soup(n, seed=seed, walls=False)[:2]


def _soups(sizes, seed=0):
    return pb.concat([_soup(n, 1000 * seed + 7 * k + n) for k, n in enumerate(sizes)])


def _identical(n):
    return np.arange(3 * n, dtype=np.int32).reshape(-1, 3), np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0.5)] * n, F)


# ---- one mesh: ntr_ploc_build's own bytes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, TILE - 1, TILE + 1, 2 * TILE + 1])
def test_one_mesh_equals_ploc_build(n):
    tri, pos = _soup(n, 7)
    box = pl.scene_box(pos)
    d_tri, d_pos = up(tri), up(pos)
    caps = nt.lbvh_capacity(n)
    for radius in (1, 8, 64):
        b = _Batch([(0, n, box[0], box[1])], tri, pos, radius)
        single = [torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in caps]
        r = nt.ploc_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), box[0], box[1], single[0].data_ptr(), caps[0], single[1].data_ptr(),
                          caps[1], single[2].data_ptr(), caps[2], radius)
        torch.cuda.synchronize()
        assert (r.nodesBytes, r.triWoopBytes, r.triIndexBytes) == b.caps[:3]
        for got, want, e in zip((b.nodes, b.woop, b.idx.view(np.uint8)), single, b.caps[:3]):
            assert np.array_equal(got, want.cpu().numpy()[:e]), (n, radius)
        m = b.mesh_results[0]
        assert (m.numNodes, m.numLeaves, m.numRounds, m.height) == (r.numNodes, r.numLeaves, r.numRounds, r.height)
        b.assert_equals_spec((n, radius))


# ---- segment edges against tile edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 8, 64])
def test_segment_edges_inside_tiles_halos_and_on_a_tile_edge(radius):
    """Boundaries at 1000 (inside tile 0 and inside tile 1's halo), 1048 and 1049 (inside tile 1, within tile 0's halo at radius 64),
    3049 .. 3054 (inside tile 2); then sizes that put a boundary at exactly 1024 and another at exactly 2048."""
    assert TILE == 1024
    for sizes in ((1000, 48, 1, 2000, 3, 1, 1, 70), (1000, 24, 1024, 1, 1, 70)):
        tri, pos, meshes = _soups(sizes, radius)
        _Batch(meshes, tri, pos, radius).assert_equals_spec((sizes, radius))


def test_one_triangle_meshes_first_last_and_adjacent_and_meshes_shorter_than_the_radius():
    for radius in (8, 64):
        for sizes in ((1, 1, 5, 1), (1, 40, 1, 1, 1, 7, 1), (2, 1, 3), (5, 7, 2, 6, 63, 64, 65), (1,) * 9):
            tri, pos, meshes = _soups(sizes, 3)
            _Batch(meshes, tri, pos, radius).assert_equals_spec((sizes, radius))


def test_meshes_that_finish_in_different_rounds():
    parts = [_soup(2, 5), pl.nested_scene(90), _soup(3000, 6)]
    tri, pos, meshes = pb.concat(parts)
    b = _Batch(meshes, tri, pos)
    ref = b.assert_equals_spec("chain beside soups")
    assert [s["numRounds"] for s in ref["stats"]][:2] == [1, 89] and b.res.numRounds == 89 and b.res.maxHeight == 89


def test_more_meshes_than_one_workgroup_of_the_per_mesh_kernel():
    rng = np.random.default_rng(20261018)
    sizes = [int(x) for x in rng.integers(1, 13, 1100)]
    n = sum(sizes)
    pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
    tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
    meshes, first = [], 0
    for s in sizes:
        box = pl.scene_box(pos[tri[first:first + s]])
        meshes.append((first, s, box[0], box[1]))
        first += s
    b = _Batch(meshes, tri, pos)
    b.assert_equals_spec("1100 meshes")
    r = b.res
    print("1100 meshes, %d triangles: %d rounds, %.3f ms (check %.3f, sort %.3f, emit %.3f, rounds %.3f)"
          % (n, r.numRounds, r.seconds * 1e3, r.checkMs, r.sortMs, r.emitMs, r.roundsMs))


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def test_identical_triangles_between_two_soups():
    tri, pos, meshes = pb.concat([_soup(700, 1), _identical(3000), _soup(900, 2)])
    for radius in (1, 8):
        b = _Batch(meshes, tri, pos, radius)
        b.assert_equals_spec(("identical3000", radius))
        assert b.mesh_results[1].numRounds == 12


def test_the_same_triangles_named_by_two_meshes_give_two_equal_blases():
    tri, pos = _soup(1500, 9)
    box = pl.scene_box(pos)
    inner = pl.scene_box(pos[tri[200:700]])
    meshes = [(0, 1500, box[0], box[1]), (200, 500, inner[0], inner[1]), (0, 1500, box[0], box[1]), (1499, 1, box[0], box[1])]
    b = _Batch(meshes, tri, pos)
    b.assert_equals_spec("overlapping ranges")
    (n0, nb0, w0, wb0), (n2, nb2, w2, wb2) = b.ranges[0], b.ranges[2]
    assert np.array_equal(b.nodes[n0:n0 + nb0], b.nodes[n2:n2 + nb2]) and np.array_equal(b.woop[w0:w0 + wb0], b.woop[w2:w2 + wb2])
    assert np.array_equal(b.idx[w0 // 16:(w0 + wb0) // 16], b.idx[w2 // 16:(w2 + wb2) // 16])


# ---- seeded --------------------------------------------------------------------------------------------------------------------------
def _seeded_mesh(rng, kind, n):
    if kind == 0:
        return _soup(n, int(rng.integers(1 << 30)))
    if kind == 1:     # a grid of coordinates: equal codes, equal distances, flat and degenerate triangles
        return np.arange(3 * n, dtype=np.int32).reshape(-1, 3), rng.integers(-4, 5, (3 * n, 3)).astype(F)
    if kind == 2:     # shared vertices, some degenerate triangles
        return rng.integers(0, n + 2, (n, 3)).astype(np.int32), rng.normal(0, 3, (n + 2, 3)).astype(F)
    pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)   # tiny extents and -0 / +0 coordinates
    pos[rng.random(pos.shape) < 0.2] = F(-0.0)
    return np.arange(3 * n, dtype=np.int32).reshape(-1, 3), pos


@pytest.mark.parametrize("group", range(4))
def test_seeded_batches_equal_spec(group):
    """20 batches (five per case) of 2 to 12 meshes drawn from the four kinds of test_bvh_ploc_gpu.test_seeded_soups_equal_spec, each of 1
    to 4000 triangles (log-uniform: most meshes are small, some span several tiles)."""
    rng = np.random.default_rng(20261018 + group)
    for i in range(5 * group, 5 * group + 5):
        parts = [_seeded_mesh(rng, int(rng.integers(4)), max(1, int(round(4000.0 ** rng.random())))) for _ in range(int(rng.integers(2, 13)))]
        tri, pos, meshes = pb.concat(parts)
        assert all(1 <= m[1] <= 4000 for m in meshes)
        radius = (1, 8, 3, 64, 17)[i % 5]
        _Batch(meshes, tri, pos, radius).assert_equals_spec((i, [m[1] for m in meshes], radius))


# ---- overflow ------------------------------------------------------------------------------------------------------------------------
def test_a_mesh_higher_than_the_tracer_stack_is_an_overflow_that_names_it():
    tri, pos, meshes = pb.concat([_soup(300, 4), _soup(1, 5), pl.nested_scene(120), _soup(50, 6)])
    b = _Batch(meshes, tri, pos, expect=-6)
    assert "mesh 2" in str(b.error) and "height 119" in str(b.error)
    b.assert_equals_spec("overflow")


# ---- the instanced trace over a batch-built pool ---------------------------------------------------------------------------------------
def test_ranges_feed_tlas_build_and_trace_instanced():
    sc = isc.scene("three")
    tri, pos, meshes = pb.concat([isc.blas(name)[:2] for name in sc["names"]])
    b = _Batch(meshes, tri, pos)
    ref = b.assert_equals_spec("three")
    pool = dict(nodes=ref["nodes"], woop=ref["woop"], tri_index=ref["tri_index"], ranges=ref["ranges"])
    inst = ni.instances(sc["transforms"], sc["blas"])
    n = inst.shape[0]
    d_inst = up(inst)
    caps = nt.tlas_capacity(n)
    d_tlas, d_rec = (torch.full((c + 64,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in caps)
    res = nt.tlas_build(n, d_inst.data_ptr(), b.ranges, b.bufs[0].data_ptr(), b.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(), caps[1])
    torch.cuda.synchronize()
    want = ni.tlas_build(pool["nodes"], pool["ranges"], inst, 8)
    tlas = d_tlas.cpu().numpy()[:res.nodesBytes].view(np.int32).reshape(-1, 16)
    records = d_rec.cpu().numpy()[:res.recordsBytes].view(np.uint32).reshape(-1, 16)
    assert res.rootLink == want["root_link"] and np.array_equal(tlas, want["nodes"]) and np.array_equal(records, want["records"])
    rays = isc.scene_rays(primary=(64, 32), random=1024)
    d_rays = up(rays)
    for any_hit in (False, True):
        d_res = torch.full((16 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_ids = torch.full((4 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        nt.trace_instanced(rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d_tlas.data_ptr(), res.nodesBytes,
                           res.rootLink, d_rec.data_ptr(), n, b.bufs[0].data_ptr(), b.caps[0], b.bufs[1].data_ptr(), b.caps[1],
                           b.bufs[2].data_ptr())
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        rid, rt, ru, rv, rinst = ni.trace(want["nodes"], want["root_link"], want["records"], pool, rays, any_hit)
        gid, gt, gu, gv = isc.result_words(d_res.cpu().numpy().view(nt.RESULT_DTYPE))
        ids = d_ids.cpu().numpy().view(np.int32)
        for name, g, e in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                           ("instance", ids, rinst)):
            assert np.array_equal(g, e), (name, any_hit)
        assert (rid >= 0).any() and len(set(rinst[rinst >= 0])) == 3


# ---- determinism and scratch -----------------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.ploc_batch_scratch_bytes() == 0
    tri, pos, meshes = _soups((1500, 1, 700, 2100, 30), 11)
    a = _Batch(meshes, tri, pos)
    held = nt.ploc_batch_scratch_bytes()
    assert held > 0
    c = _Batch(meshes, tri, pos)
    assert nt.ploc_batch_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.ploc_batch_scratch_bytes() == 0
    d = _Batch(meshes, tri, pos)
    for other in (c, d):
        for x, y in ((a.nodes, other.nodes), (a.woop, other.woop), (a.idx, other.idx)):
            assert x.tobytes() == y.tobytes()
    print("scratch: %.1f B per triangle" % (held / tri.shape[0]))
    nt.lbvh_release_workspace()
    assert nt.ploc_batch_scratch_bytes() == 0


# ---- errors found on the device, and the capture ---------------------------------------------------------------------------------------
def test_a_bad_vertex_index_in_the_third_of_five_meshes():
    tri, pos, meshes = _soups((40, 300, 1200, 1, 25), 12)
    L = nt.lib()
    for bad_index in (pos.shape[0], -1):
        bad = tri.copy()
        bad[meshes[2][0] + 1100, 2] = bad_index
        b = _Batch(meshes, bad, pos, expect=-1)
        assert "vertex index" in str(b.error)
        assert (b.nodes == 0xAB).all() and (b.woop == 0xAB).all() and (b.idx.view(np.uint8) == 0xAB).all()   # the pool is untouched
    # a failed call zeroes *result
    d_bad, d_pos = up(bad), up(pos)
    caps = nt.ploc_batch_capacity(meshes)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps[:3]]
    arr = (nt.PlocBatchMesh * len(meshes))(*[nt.PlocBatchMesh(*m) for m in meshes])
    ranges = (nt.BlasRange * len(meshes))()
    res = nt.PlocBatchResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert L.ntr_ploc_build_batch(len(meshes), C.cast(arr, C.c_void_p), tri.shape[0], d_bad.data_ptr(), pos.shape[0], d_pos.data_ptr(), 8,
                                  bufs[0].data_ptr(), caps[0], bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(), caps[2],
                                  C.cast(ranges, C.c_void_p), None, C.byref(res), None) == -1
    assert bytes(res) == bytes(C.sizeof(res))
    torch.cuda.synchronize()
    assert not any(x.any().item() for x in bufs)


def test_a_capturing_stream_is_refused():
    tri, pos, meshes = _soups((30, 1, 50), 13)
    d_tri, d_pos = up(tri), up(pos)
    caps = nt.ploc_batch_capacity(meshes)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps[:3]]
    args = (meshes, tri.shape[0], d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), caps[0], bufs[1].data_ptr(), caps[1],
            bufs[2].data_ptr(), caps[2])
    nt.ploc_build_batch(*args)                                   # the scratch pool exists before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        bufs[0].fill_(0)   # so that the graph is not empty
        try:
            nt.ploc_build_batch(*args, stream=cs)
        except nt.NtrError as e:
            errs.append((e.code, str(e)))
    assert len(errs) == 1 and errs[0][0] == -1 and "captured" in errs[0][1]
    torch.cuda.synchronize()
    res, _, _ = nt.ploc_build_batch(*args)                       # the library is as usable as before
    assert res.numMeshes == 3
