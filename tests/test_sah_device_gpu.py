"""ntr_sah_device_build on the device: the Compact buffers and counts equal the numpy spec (tests/np_sah_sweep.py) byte for byte;
on the bench scenes the tree equals the host SAH builder's by the lockstep walk; trace records over the device tree equal
oracle.trace bit for bit; validate, SAH cost, refit and the scratch pool work with it; errors that need a device are reported."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_sah_sweep as sw
import sah_sweep_scenes as ss
from gpu_util import DeviceBvh, assert_parity, up

pytestmark = pytest.mark.gpu

F = np.float32
THREADS = 16


class _Built:
    """A device build into buffers of lbvh_capacity(n) bytes, or of `room` times as many (trees with splits without a winner)."""

    def __init__(self, tri, pos, prefs=(1, 1), room=1, stream=0):
        tri = np.ascontiguousarray(tri, np.int32)
        pos = np.ascontiguousarray(pos, F)
        n = tri.shape[0]
        self.n, self.nv = n, pos.shape[0]
        self.d_tri, self.d_pos = up(tri), up(pos)
        self.caps = tuple(room * c for c in nt.lbvh_capacity(n))
        self.d_nodes, self.d_woop, self.d_idx = (torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in self.caps)
        self.res = nt.sah_device_build(n, self.d_tri.data_ptr(), self.nv, self.d_pos.data_ptr(), self.d_nodes.data_ptr(), self.caps[0],
                                       self.d_woop.data_ptr(), self.caps[1], self.d_idx.data_ptr(), self.caps[2], prefs[0], prefs[1], stream)
        torch.cuda.synchronize()
        r = self.res
        self.nodes = self.d_nodes.cpu().numpy()[:r.nodesBytes].view(np.int32).reshape(-1, 16).copy()
        self.woop = self.d_woop.cpu().numpy()[:r.triWoopBytes].copy()
        self.idx = self.d_idx.cpu().numpy()[:r.triIndexBytes].view(np.int32).copy()

    def view(self):
        v = nt.BvhView(self.d_nodes.data_ptr(), self.res.nodesBytes, self.d_woop.data_ptr(), self.res.triWoopBytes, self.d_idx.data_ptr())
        v.validate()
        return v


def _assert_equal_to_spec(b, ref, what="", nan_rows=False):
    """nan_rows: the scene's Woop rows overflow (coordinates near 1e19), and the sign and payload of a NaN that arithmetic produces
    are the processor's (x86 gives 0xFFC00000, gfx950 0x7FC00000): such words are compared as NaN == NaN, every other word by bits."""
    assert np.array_equal(b.nodes, ref["nodes"]), ("nodes differ", what)
    assert np.array_equal(b.idx, ref["tri_index"]), ("triIndex differs", what)
    if nan_rows:
        got, exp = b.woop.view(np.uint32), ref["woop"].view(np.uint32)
        assert got.shape == exp.shape and ((got == exp) | (np.isnan(got.view(F)) & np.isnan(exp.view(F)))).all(), ("triWoop differs", what)
    else:
        assert np.array_equal(b.woop, ref["woop"]), ("triWoop differs", what)
    st, r = ref["stats"], b.res
    got = dict(numInnerNodes=r.numNodes, numLeaves=r.numLeaves, numLevels=r.numLevels, maxDepth=r.maxDepth, numDropped=r.numDropped)
    assert got == st, (got, st, what)
    assert r.nodesBytes == ref["nodes"].nbytes and r.triWoopBytes == ref["woop"].nbytes and r.triIndexBytes == ref["tri_index"].nbytes


# ---- 4. device == spec, byte for byte ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefs", ss.LEAF_PREFS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_device_build_equals_spec(name, prefs):
    tri, pos = ss.scene(name)
    b = _Built(tri, pos, prefs, room=4 if name == "huge" else 1)
    _assert_equal_to_spec(b, sw.build(tri, pos, *prefs), (name, prefs), nan_rows=name == "huge")
    r = b.res
    print("%s %s: %d tris, %d dropped, %d inner, %d leaves, depth %d, %d levels, %.3f ms (prep %.3f, sort %.3f, levels %.3f, emit %.3f)"
          % (name, prefs, tri.shape[0], r.numDropped, r.numNodes, r.numLeaves, r.maxDepth, r.numLevels, r.seconds * 1e3, r.prepMs, r.sortMs,
             r.levelsMs, r.emitMs))


def test_soup_20000_equals_spec():
    tri, pos, _ = scenes.random_soup(20000, seed=77, walls=False)
    _assert_equal_to_spec(_Built(tri, pos), sw.build(tri, pos))


def test_randomised_soups_equal_spec():
    rng = np.random.default_rng(20261016)
    for i in range(200):
        big = i % 50 == 49
        n = int(rng.integers(20000, 50001)) if big else int(rng.integers(1, 600))
        kind = i % 4
        if kind == 0:
            tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        elif kind == 1:   # a grid of coordinates: equal keys, equal costs, flat and degenerate triangles
            pos = rng.integers(-4, 5, (3 * n, 3)).astype(F)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        elif kind == 2:   # shared vertices, some degenerate triangles
            pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
            tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
        else:             # tiny extents and -0 / +0 coordinates
            pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)
            pos[rng.random(pos.shape) < 0.2] = F(-0.0)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        prefs = ss.LEAF_PREFS[i % 3] if not big else (1, 1)
        _assert_equal_to_spec(_Built(tri, pos, prefs), sw.build(tri, pos, *prefs), (i, n, kind, prefs))


# ---- 5. device == host tree on the bench scenes ----------------------------------------------------------------------------
_bench = {}


def _bench_scene(name):
    if name not in _bench:
        _bench.clear()
        _bench[name] = {"atrium": scenes.atrium, "conference": scenes.conference_room, "hairball500k": lambda: scenes.hairball(500000)}[name]()
    return _bench[name]


@pytest.mark.parametrize("prefs", [(1, 1), (1, 8)])
@pytest.mark.parametrize("name", ["atrium", "conference", "hairball500k"])
def test_device_tree_equals_host_tree(name, prefs):
    tri, pos, _ = _bench_scene(name)
    b = _Built(tri, pos, prefs)
    h = nt.sah_build(tri, pos, *prefs)
    inner, leaves = sw.walk_equal((b.nodes, b.woop, b.idx), ss.buffers(h))
    r = b.res
    assert inner == r.numNodes == h.nodes.nbytes // 64 and leaves == r.numLeaves
    assert r.triWoopBytes == h.woop.nbytes and r.triIndexBytes == h.tri_index.nbytes
    print("%s %s: %d tris, %d inner, depth %d, %d levels, device %.2f ms wall (prep %.3f, sort %.3f, levels %.3f, emit %.3f), host %.1f ms"
          % (name, prefs, tri.shape[0], r.numNodes, r.maxDepth, r.numLevels, r.seconds * 1e3, r.prepMs, r.sortMs, r.levelsMs, r.emitMs,
             h.info["buildSeconds"] * 1e3))


# ---- 6. trace parity on the device tree's own buffers ----------------------------------------------------------------------
def _trace(view, kernel, d_rays, n, any_hit):
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    view.trace(kernel, n, any_hit, d_rays.data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    return d_res


def test_trace_records_equal_oracle_on_atrium():
    tri, pos, cam = _bench_scene("atrium")
    b = _Built(tri, pos)
    view = b.view()
    rays, _ = scenes.primary_rays(cam, 512, 512)
    d_rays = up(rays)
    d_prim = None
    for kernel in ("fermi_speculative_while_while", "kepler_dynamic_fetch"):
        for any_hit in (False, True):
            ref, _ = oracle.trace(b.nodes, b.woop, b.idx, rays, any_hit=any_hit, threads=THREADS)
            d_res = _trace(view, kernel, d_rays, rays.shape[0], any_hit)
            assert_parity(d_res.cpu().numpy().view(nt.RESULT_DTYPE), ref, "primary %s anyHit=%d" % (kernel, any_hit))
            if not any_hit:
                d_prim = d_res
    ns, cnt = 8, 65536
    d_nrm = up(scenes.tri_normals(tri, pos))
    d_ao = torch.zeros(cnt * ns * 32, dtype=torch.uint8, device="cuda:0")
    d_a = torch.zeros(cnt * ns, dtype=torch.int32, device="cuda:0")
    nt.raygen_ao(d_ao.data_ptr(), d_a.data_ptr(), d_a.data_ptr(), d_rays.data_ptr(), d_prim.data_ptr(), d_nrm.data_ptr(), 100000, cnt, ns, 5.0,
                 0xFFF2D5E4)
    torch.cuda.synchronize()
    ao = d_ao.cpu().numpy().view(nt.RAY_DTYPE)
    for kernel in ("fermi_speculative_while_while", "kepler_dynamic_fetch"):
        for any_hit in (False, True):
            ref, _ = oracle.trace(b.nodes, b.woop, b.idx, ao, any_hit=any_hit, threads=THREADS)
            got = _trace(view, kernel, d_ao, cnt * ns, any_hit).cpu().numpy().view(nt.RESULT_DTYPE)
            assert_parity(got, ref, "AO %s anyHit=%d" % (kernel, any_hit))


# ---- 7. works with its neighbours --------------------------------------------------------------------------------------------
def test_validate_and_sah_cost_equal_the_host_tree():
    tri, pos, _ = _bench_scene("atrium")
    b = _Built(tri, pos)
    hb = DeviceBvh(nt.sah_build(tri, pos))
    flags = nt.bvh_validate(b.d_nodes.data_ptr(), b.res.nodesBytes)
    assert flags & nt.BVH_FINITE and flags & nt.BVH_ORDERED
    mine = nt.bvh_sah_cost(b.d_nodes.data_ptr(), b.res.nodesBytes, b.d_woop.data_ptr(), b.res.triWoopBytes)
    host = nt.bvh_sah_cost(hb.nodes.data_ptr(), hb.host.nodes.nbytes, hb.woop.data_ptr(), hb.host.woop.nbytes)
    print("sahCost device tree %r host tree %r" % (mine.sahCost, host.sahCost))
    assert np.float32(mine.sahCost).view(np.uint32) == np.float32(host.sahCost).view(np.uint32)


def test_refit_with_unmoved_vertices_changes_nothing():
    tri, pos = ss.scene("soup1000")
    for prefs in ((1, 1), (4, 8)):
        b = _Built(tri, pos, prefs)
        r = b.res
        nt.bvh_refit(b.d_nodes.data_ptr(), r.nodesBytes, b.d_woop.data_ptr(), r.triWoopBytes, b.d_idx.data_ptr(), r.triIndexBytes, b.n,
                     b.d_tri.data_ptr(), b.nv, b.d_pos.data_ptr(), 0.0)
        torch.cuda.synchronize()
        nodes = b.d_nodes.cpu().numpy()[:r.nodesBytes].view(np.int32).reshape(-1, 16)
        assert np.array_equal(nodes[:, :12], b.nodes[:, :12])
        assert np.array_equal(b.d_woop.cpu().numpy()[:r.triWoopBytes], b.woop)


def test_scratch_determinism_and_release():
    nt.lbvh_release_workspace()
    assert nt.sah_device_scratch_bytes() == 0
    tri, pos, _ = scenes.random_soup(60000, seed=3)
    a = _Built(tri, pos)
    held = nt.sah_device_scratch_bytes()
    assert held > 0
    c = _Built(tri, pos)
    for x, y in ((a.nodes, c.nodes), (a.woop, c.woop), (a.idx, c.idx)):
        assert x.tobytes() == y.tobytes()
    small = ss.scene("soup1000")
    _assert_equal_to_spec(_Built(*small), sw.build(*small))
    assert nt.sah_device_scratch_bytes() == held          # a smaller mesh allocates nothing
    print("scratch: %.1f B per triangle" % (held / tri.shape[0]))
    nt.lbvh_release_workspace()
    assert nt.sah_device_scratch_bytes() == 0
    _assert_equal_to_spec(_Built(*small), sw.build(*small))
    assert 0 < nt.sah_device_scratch_bytes() < held


# ---- 8. error paths that need a device ---------------------------------------------------------------------------------------
def test_device_errors():
    tri, pos = ss.scene("cornell")
    d_tri, d_pos = up(tri), up(pos)
    n = tri.shape[0]
    caps = nt.lbvh_capacity(n)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in caps]

    def call(tri_ptr=None, caps=caps, prefs=(1, 1)):
        return nt.sah_device_build(n, tri_ptr or d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), bufs[0].data_ptr(), caps[0],
                                   bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(), caps[2], *prefs)

    for short in ((caps[0] - 1, caps[1], caps[2]), (caps[0], caps[1] - 1, caps[2]), (caps[0], caps[1], caps[2] - 1)):
        with pytest.raises(nt.NtrError) as e:
            call(caps=short)
        assert e.value.code == -1
    bad = tri.copy()
    bad[3, 1] = pos.shape[0]   # vertex index out of range: found on the device, no fault
    d_bad = up(bad)
    with pytest.raises(nt.NtrError) as e:
        call(tri_ptr=d_bad.data_ptr())
    assert e.value.code == -1
    bad[3, 1] = -1
    d_bad = up(bad)
    with pytest.raises(nt.NtrError) as e:
        call(tri_ptr=d_bad.data_ptr())
    assert e.value.code == -1
    assert call().numNodes == 33
    # a chain of splits without a winner outgrows buffers of lbvh_capacity() bytes: reported, nothing written beyond them
    htri, hpos = ss.scene("huge")
    with pytest.raises(nt.NtrError) as e:
        _Built(htri[:8], hpos)
    assert e.value.code == -6
