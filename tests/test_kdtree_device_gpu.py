"""ntr_kdtree_device_build on the device: the three buffers, scene box, delta and counts equal the numpy spec
(tests/np_kdtree_binned.py) byte for byte; builds are deterministic across runs and streams; ntr_trace_kdtree records over the device
tree equal np_kdtree.trace bit for bit and agree with the BVH tracer under the SAH kd-tree's allowances; a 1 M-triangle hairball
builds and traces; the scratch grows and is released; bad parameters are rejected."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import np_kdtree
import np_kdtree_binned as kb
import ray_sets
from gpu_util import up
from test_kdtree_gpu import classify_disagreements

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
    if name == "stacked":
        return _tri_scene([(0.0, 0.0, 0.0)] * 40)
    if name == "one":
        return _tri_scene([(1.0, 2.0, 3.0)])
    if name == "flat":
        rng = np.random.default_rng(3)
        pos = rng.uniform(-5, 5, (600, 3)).astype(F)
        pos[:, 2] = 0
        return np.arange(600, dtype=np.int32).reshape(-1, 3), pos
    raise KeyError(name)


def _spec(name, tri, pos, params=None):
    key = (name, tuple(sorted((params or {}).items())))
    if key not in _specs:
        _specs[key] = kb.build(tri, pos, params)
    return _specs[key]


def _device_build(tri, pos, params=None, stream=0):
    d_tri, d_pos = up(np.ascontiguousarray(tri, np.int32)), up(np.ascontiguousarray(pos, F))
    t = nt.kdtree_device_build(d_tri.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0], params, stream)
    return t, (d_tri, d_pos)


def _assert_equal_to_spec(t, ref):
    nodes, woop, idx = t.download()
    assert np.array_equal(nodes, ref["nodes"]), "nodes differ"
    assert np.array_equal(idx, ref["tri_index"]), "triIndex differs"
    assert np.array_equal(woop, ref["woop"]), "triWoop differs"
    assert t.scene_min.view(np.uint32).tolist() == ref["scene_min"].view(np.uint32).tolist()
    assert t.scene_max.view(np.uint32).tolist() == ref["scene_max"].view(np.uint32).tolist()
    assert F(t.delta).view(np.uint32) == F(ref["delta"]).view(np.uint32)
    st = ref["stats"]
    for k in ("numInnerNodes", "numLeafNodes", "numEmptyLeaves", "numTriRefs", "maxDepth", "numLevels"):
        assert getattr(t, k) == st[k], (k, getattr(t, k), st[k])
    assert F(t.percentDuplicates) == F(st["percentDuplicates"])
    return nodes, woop, idx


@pytest.mark.parametrize("name", ["cornell", "soup1500", "atrium", "t16", "t17", "stacked", "one", "flat"])
def test_device_build_equals_spec(name):
    tri, pos = _scene(name)
    t, _keep = _device_build(tri, pos)
    try:
        _assert_equal_to_spec(t, _spec(name, tri, pos))
        print("%s: %d tris, %d inner, %d leaves, depth %d, %d levels, dup %.1f %%, %.3f ms (prep %.3f, levels %.3f, emit %.3f)"
              % (name, tri.shape[0], t.numInnerNodes, t.numLeafNodes, t.maxDepth, t.numLevels, t.percentDuplicates, t.seconds * 1e3,
                 t.prepMs, t.levelsMs, t.emitMs))
    finally:
        t.close()


def test_device_build_params_equal_spec():
    tri, pos = _scene("soup1500")
    for params in (dict(triLimit=4), dict(failureCount=2, failRq=0.6), dict(depthK1=0.0, depthK2=5.0), dict(ci=2.0, ct=0.5)):
        t, _keep = _device_build(tri, pos, params)
        try:
            _assert_equal_to_spec(t, kb.build(tri, pos, params))
        finally:
            t.close()


def test_randomised_soups_equal_spec():
    rng = np.random.default_rng(20261016)
    for i in range(200):
        n = int(rng.integers(1, 400))
        kind = i % 4
        if kind == 0:
            tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        elif kind == 1:   # a grid of coordinates: planes meet vertices and faces often
            pos = rng.integers(-4, 5, (3 * n, 3)).astype(F)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        elif kind == 2:   # shared vertices, some degenerate triangles
            pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
            tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
        else:             # tiny extents and -0 / +0 coordinates
            pos = (rng.integers(-2, 3, (3 * n, 3)) * F(1e-30)).astype(F)
            pos[rng.random(pos.shape) < 0.2] = F(-0.0)
            tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        params = dict(triLimit=int(rng.integers(1, 20))) if i % 3 == 0 else None
        t, _keep = _device_build(tri, pos, params)
        try:
            _assert_equal_to_spec(t, kb.build(tri, pos, params))
        finally:
            t.close()


def test_determinism_and_streams():
    tri, pos = _scene("atrium")
    a, _k1 = _device_build(tri, pos)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b, _k2 = _device_build(tri, pos, stream=s.cuda_stream)
    c, _k3 = _device_build(tri, pos)
    try:
        da, db, dc = a.download(), b.download(), c.download()
        for x, y, z in zip(da, db, dc):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        # the trees coexist: each owns its buffers
        assert a.nodes != b.nodes != c.nodes
    finally:
        a.close()
        b.close()
        c.close()


def _rays(kind, pos, cam, t):
    if kind == "primary":
        return scenes.primary_rays(cam, 64, 64)[0]
    if kind == "random":
        return scenes.random_rays(4096, 5, extent=float(np.abs(pos).max()))
    if kind == "box":
        return scenes.box_rays(pos, 4096, 13)
    if kind == "edge":
        return ray_sets.edge_rays(float(np.abs(pos).max()))
    if kind == "split":   # rays along and onto the split planes of the first levels
        nodes, _, _ = t.download()
        rays = scenes.random_rays(2048, 9, extent=float(np.abs(pos).max()))
        for i in range(rays.shape[0]):
            nd = nodes[i % min(nodes.shape[0], 32)]
            a = (int(nd[3]) >> 28) & 3
            p = np.array([nd[2]], np.int32).view(F)[0]
            rays[("ox", "oy", "oz")[a]][i] = p
            if i % 2:
                rays[("dx", "dy", "dz")[a]][i] = 0
        return rays
    raise KeyError(kind)


@pytest.mark.parametrize("name", ["cornell", "soup1500", "atrium"])
def test_trace_records_equal_restatement(name):
    tri, pos = _scene(name)
    cam = {"cornell": scenes.cornell_box, "soup1500": lambda: scenes.random_soup(1500, seed=11), "atrium": scenes.atrium}[name]()[2]
    t, _keep = _device_build(tri, pos)
    try:
        nodes, woop, idx = t.download()
        for kind in ("primary", "random", "box", "edge", "split"):
            rays = _rays(kind, pos, cam, t)
            d_rays = up(rays)
            d_res = torch.full((rays.shape[0] * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
            t.trace(rays.shape[0], False, d_rays.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
            ref = np_kdtree.trace(nodes, woop, idx, t.scene_min, t.scene_max, rays)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, kind)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["cornell", "soup1500", "atrium"])
def test_agreement_with_bvh_tracer(name):
    """The device tree finds what the BVH finds, under exactly the exceptions of the SAH kd-tree's test
    (test_kdtree_gpu.py::test_agreement_with_bvh_tracer).  The tree is traced with the host's Woop rows -- the BVH's, by triangle
    id -- so that both tracers test the same rows: the device rows (woop_rows.h, pinned byte for byte by the spec tests) differ from
    them in the last bits, which decides the hit of a ray that grazes a triangle."""
    tri, pos = _scene(name)
    cam = {"cornell": scenes.cornell_box, "soup1500": lambda: scenes.random_soup(1500, seed=11), "atrium": scenes.atrium}[name]()[2]
    t, _keep = _device_build(tri, pos)
    try:
        nodes, _, idx = t.download()
        host_rows = nt.kdtree_build(tri, pos, "SpatialMedianKDTree", max_leaf=tri.shape[0]).woop   # one leaf: rows by triangle id
        kd = nt.host_kdtree_wrap(nodes, host_rows, idx, t.scene_min, t.scene_max)
        rays = np.concatenate([scenes.primary_rays(cam, 256, 256)[0], scenes.box_rays(pos, 1 << 15, 13)])
        d_rays, d_rows = up(rays), up(host_rows)
        d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        nt.trace_kdtree(rays.shape[0], False, t.scene_min, t.scene_max, d_rays.data_ptr(), d_res.data_ptr(), t.nodes, t.nodesBytes,
                        d_rows.data_ptr(), host_rows.nbytes, t.triIndex, t.triIndexBytes)
        torch.cuda.synchronize()
        got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
        bvh = nt.sah_build(tri, pos)
        d_nodes, d_woop, d_idx = up(bvh.nodes), up(bvh.woop), up(bvh.tri_index)
        d_ref = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        nt.trace_bvh("fermi_speculative_while_while", rays.shape[0], False, d_rays.data_ptr(), d_ref.data_ptr(), d_nodes.data_ptr(),
                     bvh.nodes.nbytes, d_woop.data_ptr(), bvh.woop.nbytes, d_idx.data_ptr())
        torch.cuda.synchronize()
        ref = d_ref.cpu().numpy().view(nt.RESULT_DTYPE)
        other, agree, counts = classify_disagreements(got, ref, rays, kd, tri, pos)
        print("%s: %s, ids agree on %.5f of the considered rays" % (name, counts, agree))
        assert other.size == 0, (name, other[:5], got[other[:5]], ref[other[:5]])
        assert agree >= 0.999
        # with its own rows the tree differs from the above only on rays that graze a triangle: the same id nearly everywhere
        d_own = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        t.trace(rays.shape[0], False, d_rays.data_ptr(), d_own.data_ptr())
        torch.cuda.synchronize()
        own = d_own.cpu().numpy().view(nt.RESULT_DTYPE)
        assert (own["id"] == got["id"]).mean() >= 0.9999
    finally:
        t.close()


def test_hairball_builds_and_traces():
    tri, pos, cam = scenes.hairball(1_000_000)
    t, _keep = _device_build(tri, pos)
    try:
        assert t.maxDepth <= kb.max_depth(tri.shape[0]) and t.numTriRefs >= tri.shape[0]
        rays = scenes.primary_rays(cam, 256, 256)[0]
        d_rays = up(rays)
        d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        nt.trace_status()   # clears the status word
        sec = t.trace(rays.shape[0], False, d_rays.data_ptr(), d_res.data_ptr())   # timed: overflow / layout bits raise
        assert sec > 0
        assert nt.trace_status() == 0
        got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
        assert (got["id"] >= 0).mean() > 0.1
        print("hairball 1M: depth %d, %d inner, dup %.1f %%, build %.2f ms" % (t.maxDepth, t.numInnerNodes, t.percentDuplicates,
                                                                                t.seconds * 1e3))
    finally:
        t.close()


def test_scratch_grows_and_is_released():
    nt.lbvh_release_workspace()
    assert nt.kdtree_device_scratch_bytes() == 0
    held = []
    for n in (100, 5000, 60000):
        tri, pos, _ = scenes.random_soup(n, seed=n)
        t, _keep = _device_build(tri, pos)
        if n <= 5000:
            _assert_equal_to_spec(t, kb.build(tri, pos))
        t.close()
        held.append(nt.kdtree_device_scratch_bytes())
    assert 0 < held[0] <= held[1] < held[2], held      # grow-only, and larger scenes need more
    # a smaller build after a larger one reuses the pool (and still equals the spec)
    tri, pos, _ = scenes.random_soup(3000, seed=1)
    t, _keep = _device_build(tri, pos)
    try:
        _assert_equal_to_spec(t, kb.build(tri, pos))
    finally:
        t.close()
    assert nt.kdtree_device_scratch_bytes() == held[2]
    nt.lbvh_release_workspace()
    assert nt.kdtree_device_scratch_bytes() == 0
    # a build after the release allocates again
    t, _keep = _device_build(tri, pos)
    try:
        _assert_equal_to_spec(t, kb.build(tri, pos))
        assert nt.kdtree_device_scratch_bytes() > 0
    finally:
        t.close()


def test_bad_parameters_invalid():
    tri, pos = _scene("cornell")
    d_tri, d_pos = up(tri), up(pos)
    for kw in (dict(triLimit=0), dict(failRq=float("nan")), dict(depthK1=40.0), dict(failureCount=-3)):
        with pytest.raises(nt.NtrError) as e:
            nt.kdtree_device_build(d_tri.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0], kw)
        assert e.value.code == -1
    bad = tri.copy()
    bad[3, 1] = pos.shape[0]   # vertex index out of range: found on the device, no fault
    d_bad = up(bad)
    with pytest.raises(nt.NtrError) as e:
        nt.kdtree_device_build(d_bad.data_ptr(), tri.shape[0], d_pos.data_ptr(), pos.shape[0])
    assert e.value.code == -1
