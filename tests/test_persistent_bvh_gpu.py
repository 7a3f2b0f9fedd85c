"""ntr_persistent_bvh_build on the device: the Compact buffers and counts equal the numpy spec (tests/np_bvh_binned.py) byte for
byte; builds are deterministic across runs and streams; ntr_bvh_validate gives the flags the buffers call for; trace records over
the device tree equal oracle.trace bit for bit for every kernel name, closest and any hit; the hairball builds and traces; the
scratch grows and is released; bad parameters are rejected."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_bvh_binned as bb
import ray_sets
from gpu_util import up
from np_bvh_validate import expected_flags

pytestmark = pytest.mark.gpu

F = np.float32
_specs = {}


def _tri_scene(corners, s=0.25):
    pos = np.array([v for (x, y, z) in corners for v in [(x, y, z), (x + s, y, z), (x, y + s, z)]], F)
    return np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3), pos


def _scene(name):
    if name == "cornell":
        return scenes.cornell_box()[:2]
    if name == "soup1500":
        return scenes.random_soup(1500, seed=11)[:2]
    if name == "atrium":
        return scenes.atrium()[:2]
    if name == "t16":
        return _tri_scene([(float(i % 5) * 2, float(i // 5) * 2, 0.0) for i in range(16)])
    if name == "t17":
        return _tri_scene([(float(i % 5) * 2, float(i // 5) * 2, 0.0) for i in range(17)])
    if name == "stacked":     # identical triangles: no plane separates them, the median does
        return _tri_scene([(0.0, 0.0, 0.0)] * 40)
    if name == "one":
        return _tri_scene([(1.0, 2.0, 3.0)])
    if name == "flat":
        rng = np.random.default_rng(3)
        pos = rng.uniform(-5, 5, (600, 3)).astype(F)
        pos[:, 2] = 0
        return np.arange(600, dtype=np.int32).reshape(-1, 3), pos
    if name == "zero_area":   # points and segments
        rng = np.random.default_rng(4)
        pos = rng.uniform(-5, 5, (300, 3)).astype(F)
        tri = np.stack([np.arange(300), np.arange(300), (np.arange(300) + 1) % 300], 1).astype(np.int32)
        tri[::3, 2] = tri[::3, 0]
        return tri, pos
    raise KeyError(name)


def _bbox(pos):
    mn, mx = oracle.scene_bbox(np.ascontiguousarray(pos, F))
    return np.asarray(mn, F), np.asarray(mx, F)


def _spec(name, tri, pos, params=None):
    key = (name, tuple(sorted((params or {}).items())))
    if key not in _specs:
        mn, mx = _bbox(pos)
        _specs[key] = bb.build(tri, pos, mn, mx, params)
    return _specs[key]


class _Built:
    def __init__(self, tri, pos, params=None, stream=0):
        tri = np.ascontiguousarray(tri, np.int32)
        pos = np.ascontiguousarray(pos, F)
        n = tri.shape[0]
        self.d_tri, self.d_pos = up(tri), up(pos)
        capn, capw, capi = nt.lbvh_capacity(n)
        self.d_nodes = torch.full((capn,), 0xAB, dtype=torch.uint8, device="cuda:0")
        self.d_woop = torch.full((capw,), 0xAB, dtype=torch.uint8, device="cuda:0")
        self.d_idx = torch.full((capi,), 0xAB, dtype=torch.uint8, device="cuda:0")
        mn, mx = _bbox(pos)
        self.res = nt.persistent_bvh_build(n, self.d_tri.data_ptr(), pos.shape[0], self.d_pos.data_ptr(), mn, mx, self.d_nodes.data_ptr(),
                                           capn, self.d_woop.data_ptr(), capw, self.d_idx.data_ptr(), capi, params, stream)
        torch.cuda.synchronize()
        r = self.res
        self.nodes = self.d_nodes.cpu().numpy()[:r.nodesBytes].view(np.int32).reshape(-1, 16)
        self.woop = self.d_woop.cpu().numpy()[:r.triWoopBytes].copy()
        self.idx = self.d_idx.cpu().numpy()[:r.triIndexBytes].view(np.int32).copy()


def _assert_equal_to_spec(b, ref):
    assert np.array_equal(b.nodes, ref["nodes"]), "nodes differ"
    assert np.array_equal(b.idx, ref["tri_index"]), "triIndex differs"
    assert np.array_equal(b.woop, ref["woop"]), "triWoop differs"
    st, r = ref["stats"], b.res
    got = dict(numInnerNodes=r.numNodes, numLeaves=r.numLeaves, numLevels=r.numLevels, maxDepth=r.maxDepth,
               medianFallbacks=r.medianFallbacks, costLeaves=r.costLeaves, depthLeaves=r.depthLeaves)
    assert got == st, (got, st)
    assert r.nodesBytes == ref["nodes"].nbytes and r.triWoopBytes == ref["woop"].nbytes and r.triIndexBytes == ref["tri_index"].nbytes


@pytest.mark.parametrize("name", ["cornell", "soup1500", "atrium", "t16", "t17", "stacked", "one", "flat", "zero_area"])
def test_device_build_equals_spec(name):
    tri, pos = _scene(name)
    b = _Built(tri, pos)
    ref = _spec(name, tri, pos)
    _assert_equal_to_spec(b, ref)
    bb.check_invariants(ref, tri, pos)
    flags = nt.bvh_validate(b.d_nodes.data_ptr(), b.res.nodesBytes)
    assert flags == expected_flags(b.nodes, b.res.triWoopBytes), (name, flags)
    r = b.res
    print("%s: %d tris, %d inner, %d leaves, depth %d, %d levels, %d median, %.3f ms (prep %.3f, levels %.3f, emit %.3f)"
          % (name, tri.shape[0], r.numNodes, r.numLeaves, r.maxDepth, r.numLevels, r.medianFallbacks, r.seconds * 1e3, r.prepMs,
             r.levelsMs, r.emitMs))


def test_device_build_params_equal_spec():
    tri, pos = _scene("soup1500")
    for params in (dict(triLimit=1, triMaxLimit=0), dict(triLimit=4), dict(triMaxLimit=64, ct=0.1), dict(maxDepth=4),
                   dict(ci=2.0, ct=0.5, epsilon=0.01), dict(triLimit=2000)):
        b = _Built(tri, pos, params)
        mn, mx = _bbox(pos)
        _assert_equal_to_spec(b, bb.build(tri, pos, mn, mx, params))


def test_randomised_soups_equal_spec():
    rng = np.random.default_rng(20261016)
    for i in range(200):
        big = i % 50 == 49
        n = int(rng.integers(20000, 50001)) if big else int(rng.integers(1, 600))
        kind = i % 4
        if kind == 0:
            tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        elif kind == 1:   # a grid of coordinates: centroids on planes, equal boxes
            pos = rng.integers(-4, 5, (3 * n, 3)).astype(F)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        elif kind == 2:   # shared vertices, some degenerate triangles
            pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
            tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
        else:             # tiny extents and -0 / +0 coordinates
            pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)
            pos[rng.random(pos.shape) < 0.2] = F(-0.0)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        params = dict(triLimit=int(rng.integers(1, 20)), triMaxLimit=int(rng.integers(0, 40))) if i % 3 == 0 else None
        b = _Built(tri, pos, params)
        mn, mx = _bbox(pos)
        _assert_equal_to_spec(b, bb.build(tri, pos, mn, mx, params))


def test_determinism_and_streams():
    tri, pos = _scene("atrium")
    a = _Built(tri, pos)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = _Built(tri, pos, stream=s.cuda_stream)
    c = _Built(tri, pos)
    for x, y, z in ((a.nodes, b.nodes, c.nodes), (a.woop, b.woop, c.woop), (a.idx, b.idx, c.idx)):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def _rays(kind, pos, cam):
    if kind == "primary":
        return scenes.primary_rays(cam, 64, 64)[0]
    if kind == "random":
        return scenes.random_rays(4096, 5, extent=float(np.abs(pos).max()))
    if kind == "box":
        return scenes.box_rays(pos, 4096, 13)
    if kind == "edge":
        return ray_sets.edge_rays(float(np.abs(pos).max()))
    raise KeyError(kind)


def _trace(b, d_rays, n, kernel, any_hit):
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    nt.trace_bvh(kernel, n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), b.d_nodes.data_ptr(), b.res.nodesBytes, b.d_woop.data_ptr(),
                 b.res.triWoopBytes, b.d_idx.data_ptr())
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(nt.RESULT_DTYPE)


def _assert_records(got, ref, any_hit, what):
    assert np.array_equal(got["id"], ref["id"]), what
    if not any_hit:
        assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), what


@pytest.mark.parametrize("name", ["cornell", "soup1500", "atrium", "one", "stacked"])
def test_trace_records_equal_oracle(name):
    tri, pos = _scene(name)
    cam = {"cornell": scenes.cornell_box, "soup1500": lambda: scenes.random_soup(1500, seed=11),
           "atrium": scenes.atrium}.get(name, scenes.cornell_box)()[2]
    b = _Built(tri, pos)
    for kind in ("primary", "random", "box", "edge"):
        rays = _rays(kind, pos, cam)
        d_rays = up(rays)
        for any_hit in (False, True):
            ref, _ = oracle.trace(b.nodes, b.woop, b.idx, rays, any_hit=any_hit, threads=8)
            for kernel in nt.KERNELS:
                _assert_records(_trace(b, d_rays, rays.shape[0], kernel, any_hit), ref, any_hit, (name, kind, kernel, any_hit))


def test_large_batch_equals_oracle():
    """A batch of 2^20 rays, so that the routed persistent body runs."""
    tri, pos, cam = scenes.atrium()
    b = _Built(tri, pos)
    rays = scenes.primary_rays(cam, 1024, 1024)[0]
    assert rays.shape[0] >= 1 << 20
    d_rays = up(rays)
    ref, _ = oracle.trace(b.nodes, b.woop, b.idx, rays, threads=16)
    for kernel in nt.KERNELS:
        _assert_records(_trace(b, d_rays, rays.shape[0], kernel, False), ref, False, kernel)


def test_hairball_builds_and_traces():
    tri, pos, cam = scenes.hairball()
    b = _Built(tri, pos)
    r = b.res
    assert r.numNodes == r.numLeaves - 1 and r.triWoopBytes == 16 * (3 * tri.shape[0] + r.numLeaves)
    flags = nt.bvh_validate(b.d_nodes.data_ptr(), r.nodesBytes)
    assert flags & nt.BVH_FINITE and flags & nt.BVH_ORDERED
    rays = scenes.primary_rays(cam, 256, 256)[0]
    nt.trace_status()
    got = _trace(b, up(rays), rays.shape[0], "fermi_speculative_while_while", False)
    assert nt.trace_status() == 0
    ref, _ = oracle.trace(b.nodes, b.woop, b.idx, rays, threads=16)
    _assert_records(got, ref, False, "hairball")
    assert (got["id"] >= 0).mean() > 0.1
    print("hairball %d: %d inner, depth %d, %d levels, build %.2f ms (prep %.3f, levels %.3f, emit %.3f)"
          % (tri.shape[0], r.numNodes, r.maxDepth, r.numLevels, r.seconds * 1e3, r.prepMs, r.levelsMs, r.emitMs))


def test_compact_link_limit_is_overflow():
    """A tree of more inner nodes than Compact's signed 32-bit child byte offsets address (0x76543200 / 64 = 31 019 208) is
    NTR_ERR_OVERFLOW, not a tree with wrapped links: a 4124 x 4124 vertex grid has 33 998 258 triangles, and with one-triangle leaves
    (triLimit 1, no SAH termination) the tree needs one inner node fewer."""
    k = 4124
    i, j = np.meshgrid(np.arange(k - 1, dtype=np.int64), np.arange(k - 1, dtype=np.int64), indexing="ij")
    a = (i * k + j).ravel()
    tri = np.concatenate([np.stack([a, a + k, a + k + 1], 1), np.stack([a, a + k + 1, a + 1], 1)]).astype(np.int32)
    del i, j, a
    v = np.arange(k * k, dtype=np.int64)
    pos = np.stack([v // k, v % k, np.zeros_like(v)], 1).astype(F)
    n = tri.shape[0]
    assert n - 1 > 0x76543200 // 64
    try:
        with pytest.raises(nt.NtrError) as e:
            _Built(tri, pos, dict(triLimit=1, triMaxLimit=0))
        assert e.value.code == -6, e.value
    finally:
        nt.lbvh_release_workspace()
        torch.cuda.empty_cache()


def test_scratch_grows_and_is_released():
    nt.lbvh_release_workspace()
    assert nt.persistent_bvh_scratch_bytes() == 0
    held = []
    for n in (100, 5000, 60000):
        tri, pos, _ = scenes.random_soup(n, seed=n)
        b = _Built(tri, pos)
        if n <= 5000:
            mn, mx = _bbox(pos)
            _assert_equal_to_spec(b, bb.build(tri, pos, mn, mx))
        held.append(nt.persistent_bvh_scratch_bytes())
    assert 0 < held[0] <= held[1] < held[2], held
    tri, pos, _ = scenes.random_soup(3000, seed=1)
    mn, mx = _bbox(pos)
    _assert_equal_to_spec(_Built(tri, pos), bb.build(tri, pos, mn, mx))
    assert nt.persistent_bvh_scratch_bytes() == held[2]
    nt.lbvh_release_workspace()
    assert nt.persistent_bvh_scratch_bytes() == 0
    _assert_equal_to_spec(_Built(tri, pos), bb.build(tri, pos, mn, mx))
    assert nt.persistent_bvh_scratch_bytes() > 0


def test_bad_parameters_invalid():
    tri, pos = _scene("cornell")
    d_tri, d_pos = up(tri), up(pos)
    n = tri.shape[0]
    capn, capw, capi = nt.lbvh_capacity(n)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
    mn, mx = _bbox(pos)

    def call(params=None, tri_ptr=None, caps=(capn, capw, capi), num=n, box=(mn, mx)):
        return nt.persistent_bvh_build(num, tri_ptr or d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), box[0], box[1], bufs[0].data_ptr(),
                                       caps[0], bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(), caps[2], params)

    for kw in (dict(triLimit=0), dict(triMaxLimit=-1), dict(maxDepth=0), dict(maxDepth=101), dict(ci=float("nan")),
               dict(ct=float("inf")), dict(epsilon=float("nan")), dict(epsilon=-1e-3)):
        with pytest.raises(nt.NtrError) as e:
            call(kw)
        assert e.value.code == -1, kw
    # the planes must not decrease along an axis: an inverted or non-finite scene box is a parameter error
    for k, lo, hi in ((0, 1.0, 0.0), (1, float("nan"), 1.0), (2, 0.0, float("inf")), (0, -float("inf"), 0.0)):
        bmn, bmx = mn.copy(), mx.copy()
        bmn[k], bmx[k] = lo, hi
        with pytest.raises(nt.NtrError) as e:
            call(box=(bmn, bmx))
        assert e.value.code == -1, (k, lo, hi)
    call(box=(mx, mx))   # a flat box (min == max on every axis) is accepted
    for caps in ((capn - 64, capw, capi), (capn, capw - 16, capi), (capn, capw, capi - 4)):
        with pytest.raises(nt.NtrError) as e:
            call(caps=caps)
        assert e.value.code == -1
    with pytest.raises(nt.NtrError) as e:
        call(num=0)
    assert e.value.code == -1
    bad = tri.copy()
    bad[3, 1] = pos.shape[0]   # vertex index out of range: found on the device, no fault
    d_bad = up(bad)
    with pytest.raises(nt.NtrError) as e:
        call(tri_ptr=d_bad.data_ptr())
    assert e.value.code == -1
    call(dict(maxDepth=100))   # the deepest accepted
