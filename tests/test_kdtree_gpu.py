"""ntr_trace_kdtree on the device: records bit for bit equal to the numpy restatement (tests/np_kdtree.py) for both builders,
any-hit identical to closest-hit, the SAH tree of a 1 M-triangle hairball without stack overflow, and agreement with the BVH
tracer over a SAH BVH of the same scene."""
import time

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import np_kdtree
import ray_sets
from gpu_util import up

pytestmark = pytest.mark.gpu

BUILDERS = ("SpatialMedianKDTree", "SAHKDTree")
_trees = {}


def _scene(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "soup1500":
        return scenes.random_soup(1500, seed=11)
    if name == "atrium":
        return scenes.atrium()
    raise KeyError(name)


def _tree(scene, builder):
    key = (scene, builder)
    if key not in _trees:
        tri, pos, cam = _scene(scene)
        _trees[key] = (tri, pos, cam, nt.kdtree_build(tri, pos, builder))
    return _trees[key]


class DeviceKdtree:
    def __init__(self, kd):
        self.kd = kd
        self.nodes, self.woop, self.idx = up(kd.nodes), up(kd.woop), up(kd.tri_index)

    def trace(self, rays, any_hit=False, prefill=0xCD, timed=True):
        n = rays.shape[0]
        d_rays = up(rays) if n else torch.zeros(32, dtype=torch.uint8, device="cuda:0")
        d_res = torch.full((max(n, 1) * 16,), prefill, dtype=torch.uint8, device="cuda:0")
        sec = self.kd.trace(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.nodes.data_ptr(), self.woop.data_ptr(),
                            self.idx.data_ptr(), torch.cuda.current_stream().cuda_stream, timed)
        torch.cuda.synchronize()
        return d_res.cpu().numpy().view(nt.RESULT_DTYPE)[:n], sec


def _rays(scene, pos, cam, kind, n=None):
    if kind == "primary":
        return scenes.primary_rays(cam, 64, 64)[0]
    if kind == "random":
        return scenes.random_rays(n or 4096, 5, extent=float(np.abs(pos).max()))
    if kind == "box":
        return scenes.box_rays(pos, n or 4096, 7)
    if kind == "edge":
        return ray_sets.edge_rays(cam_extent=float(np.abs(pos).max()))
    raise KeyError(kind)


def _assert_records(got, ref, what):
    for f in ("id", "t", "padA", "padB"):
        a, b = got[f].view(np.uint32), ref[f].view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "%s: %d %s mismatches of %d, first at %d: got %r ref %r" % (what, bad.size, f, got.shape[0], bad[0],
                                                                                       got[bad[0]], ref[bad[0]])


def _split_plane_rays(kd, count=512):
    """Rays whose origins lie on split planes of the tree (axis-parallel and oblique)."""
    rng = np.random.default_rng(3)
    nodes = kd.nodes
    pick = rng.integers(0, nodes.shape[0], size=count)
    lo, hi = kd.scene_min.astype(np.float64), kd.scene_max.astype(np.float64)
    o = lo + rng.uniform(0, 1, size=(count, 3)) * (hi - lo)
    axis = (nodes[pick, 3] >> 28) & 0xF
    o[np.arange(count), axis] = nodes[pick, 2].view(np.float32)
    d = rng.normal(size=(count, 3))
    d[::4, :] = 0.0
    d[::4, 0] = 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(count, dtype=nt.RAY_DTYPE)
    for k, a in zip(("ox", "oy", "oz"), o.T):
        r[k] = a.astype(np.float32)
    for k, a in zip(("dx", "dy", "dz"), d.T):
        r[k] = a.astype(np.float32)
    r["tmin"] = 0.0
    r["tmax"] = np.float32(np.linalg.norm(hi - lo))
    return r


def _extra_edge_rays(pos):
    """tmin > 0, tmax = -1, denormal and zero direction components."""
    c = pos.mean(axis=0).astype(np.float32)
    rows = []
    for dvec in ((1e-40, 1.0, 0.0), (0.0, -1e-39, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.3, -0.4, 0.5)):
        rows.append((c[0], c[1], c[2], 0.0) + dvec + (1e30,))
        rows.append((c[0], c[1], c[2], 5.0) + dvec + (1e30,))
        rows.append((c[0], c[1], c[2], 0.0) + dvec + (-1.0,))
    return np.array(rows, dtype=np.float32).view(nt.RAY_DTYPE).reshape(-1)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("scene", ["cornell", "soup1500", "atrium"])
def test_records_bit_exact(scene, builder):
    tri, pos, cam, kd = _tree(scene, builder)
    dk = DeviceKdtree(kd)
    sets = [_rays(scene, pos, cam, k) for k in ("primary", "random", "box", "edge")]
    sets += [_split_plane_rays(kd), _extra_edge_rays(pos)]
    rays = np.concatenate(sets)
    ref = np_kdtree.trace(kd.nodes, kd.woop, kd.tri_index, kd.scene_min, kd.scene_max, rays)
    got, _ = dk.trace(rays)
    _assert_records(got, ref, "%s/%s" % (scene, builder))
    assert (got["id"] >= 0).any()
    for n in (1, 63, 65):
        g, _ = dk.trace(rays[:n])
        _assert_records(g, ref[:n], "%s/%s batch %d" % (scene, builder, n))
    got_any, _ = dk.trace(rays, any_hit=True)
    _assert_records(got_any, ref, "%s/%s anyHit" % (scene, builder))


@pytest.mark.parametrize("builder", BUILDERS)
def test_large_batch_bit_exact(builder):
    tri, pos, cam, kd = _tree("cornell", builder)
    prim = scenes.primary_rays(cam, 1024, 1024)[0]
    rays = np.concatenate([prim, prim[:3]])
    assert rays.shape[0] == (1 << 20) + 3
    got, sec = DeviceKdtree(kd).trace(rays)
    ref = np_kdtree.trace(kd.nodes, kd.woop, kd.tri_index, kd.scene_min, kd.scene_max, rays)
    _assert_records(got, ref, "cornell/%s 2^20+3" % builder)
    assert sec > 0.0


def test_empty_batch_and_async_status():
    tri, pos, cam, kd = _tree("cornell", "SAHKDTree")
    dk = DeviceKdtree(kd)
    got, sec = dk.trace(scenes.primary_rays(cam, 4, 4)[0][:0])
    assert got.shape[0] == 0 and sec == 0.0
    rays = scenes.primary_rays(cam, 32, 32)[0]
    got, sec = dk.trace(rays, timed=False)
    assert sec is None
    assert nt.trace_status(torch.cuda.current_stream().cuda_stream) == 0
    ref = np_kdtree.trace(kd.nodes, kd.woop, kd.tri_index, kd.scene_min, kd.scene_max, rays)
    _assert_records(got, ref, "async")


def test_deep_sah_tree_hairball():
    tri, pos, cam = scenes.hairball(1_000_000, seed=4)
    t0 = time.time()
    kd = nt.kdtree_build(tri, pos, "SAHKDTree")
    build = time.time() - t0
    print("hairball 1M SAH kd-tree: build %.1f s (%s)" % (build, kd.info))
    limit = int(np.float32(1.2) * np.float32(np.log(np.float32(tri.shape[0])) / np.log(np.float32(2.0))) + np.float32(2.0))
    assert kd.info["maxDepth"] <= limit
    assert build < 400.0
    rays = np.concatenate([scenes.primary_rays(cam, 256, 256)[0], scenes.box_rays(pos, 1 << 16, 9)])
    got, sec = DeviceKdtree(kd).trace(rays)   # timed: NTR_ERR_OVERFLOW would raise
    assert nt.trace_status(torch.cuda.current_stream().cuda_stream) == 0
    assert (got["id"] >= 0).sum() > rays.shape[0] // 10
    sub = np.arange(0, rays.shape[0], 37)
    ref = np_kdtree.trace(kd.nodes, kd.woop, kd.tri_index, kd.scene_min, kd.scene_max, rays[sub])
    _assert_records(got[sub], ref, "hairball sample")


def _flat_cell_triangles(kd, num_tris):
    """True for triangles referenced by a leaf whose cell has zero width on some axis."""
    out = np.zeros(num_tris, dtype=bool)
    for lo, hi, ids in np_kdtree.leaf_cells(kd.nodes, kd.tri_index, kd.scene_min, kd.scene_max):
        if ids and np.any(hi - lo == 0.0):
            out[ids] = True
    return out


def _on_box_face(tri, pos, kd):
    """True for triangles that lie in a face plane of the kd-tree's scene box."""
    v = pos[tri]
    out = np.zeros(tri.shape[0], dtype=bool)
    for a in range(3):
        for b in (kd.scene_min[a], kd.scene_max[a]):
            out |= np.all(v[:, :, a] == b, axis=1)
    return out


def classify_disagreements(got, ref, rays, kd, tri, pos):
    """(unexplained ray indices, agreement over the rays whose BVH hit is not a flat-cell or box-face triangle, counts)."""
    dis = np.nonzero(got["id"] != ref["id"])[0]
    delta = float(kd.delta)
    slack = 2e-4 + 2 * delta
    kt, bt = got["t"][dis].astype(np.float64), ref["t"][dis].astype(np.float64)
    same_t = np.abs(kt - bt) <= slack
    # outside the BVH's open interval (tmin, tmax) -- t == tmin included: a ray starting on a triangle -- by at most 1e-4 + delta
    outside = (got["id"][dis] >= 0) & (((kt <= rays["tmin"][dis]) & (kt >= rays["tmin"][dis] - 1e-4 - delta)) |
                                       ((kt >= rays["tmax"][dis]) & (kt <= rays["tmax"][dis] + 1e-4 + delta)))
    special_tri = _flat_cell_triangles(kd, tri.shape[0]) | _on_box_face(tri, pos, kd)
    ref_special = (ref["id"] >= 0) & special_tri[np.maximum(ref["id"], 0)]
    special = ref_special[dis] & ((got["id"][dis] < 0) | (kt >= bt - slack))
    # a hit on a triangle's edge, by one tracer's barycentrics (the two Woop tests order their operations differently)
    def on_edge(rec):
        u, v = rec["padA"].view(np.float32).astype(np.float64), rec["padB"].view(np.float32).astype(np.float64)
        return (rec["id"] >= 0) & (np.minimum(np.minimum(u, v), 1.0 - u - v) <= 1e-5)
    edge = on_edge(got[dis]) | on_edge(ref[dis])
    other = dis[~(same_t | outside | special | edge)]
    counts = dict(rays=int(rays.shape[0]), disagree=int(dis.size), same_t=int(same_t.sum()), outside=int(outside.sum()),
                  special=int(special.sum()), edge=int(edge.sum()), considered=int((~ref_special).sum()))
    agree = float((got["id"] == ref["id"])[~ref_special].mean())
    return other, agree, counts


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("scene", ["cornell", "soup1500", "atrium"])
def test_agreement_with_bvh_tracer(scene, builder):
    """The kd-tree finds what the BVH finds.  Allowed differences: a different triangle at the same distance within the kd
    kernel's slack (|dt| <= 2e-4 + 2 delta); a kd hit at most 1e-4 + delta outside the BVH's open interval (ray.tmin, ray.tmax)
    (the kernel accepts t >= tmin - delta and does not clip beyond its slack); a hit within 1e-5 (barycentric) of a triangle's
    edge by either tracer (the two Woop tests order their operations differently); and -- the reference kernel's arithmetic -- a kd
    miss or farther hit where the BVH hit a triangle lying in a face of the scene box or one the builder put into a zero-width
    cell (planar triangles on a split plane, the SAH builder's choice).  Such a cell's interval is [t, t] with t from
    (split - o) * idir, and the Woop t must lie within delta of it (delta is 0 for a box centred on the origin; a grazing ray's
    Woop t is far less accurate than delta); a face of the scene box is reached only within the root interval's 1e-4 slack of
    bmax * idir - o * idir, which (split - o) * idir need not meet.  Any other disagreement -- a triangle some leaf dropped --
    fails, and >= 99.9 % of the rays whose BVH record is not such a hit must agree."""
    tri, pos, cam, kd = _tree(scene, builder)
    prim = scenes.primary_rays(cam, 256, 256)[0]
    rays = np.concatenate([prim, scenes.box_rays(pos, 1 << 15, 13)])
    got, _ = DeviceKdtree(kd).trace(rays)
    bvh = nt.sah_build(tri, pos)
    d_nodes, d_woop, d_idx, d_rays = up(bvh.nodes), up(bvh.woop), up(bvh.tri_index), up(rays)
    d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
    nt.trace_bvh("fermi_speculative_while_while", rays.shape[0], False, d_rays.data_ptr(), d_res.data_ptr(), d_nodes.data_ptr(),
                 bvh.nodes.nbytes, d_woop.data_ptr(), bvh.woop.nbytes, d_idx.data_ptr())
    torch.cuda.synchronize()
    ref = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
    other, agree, counts = classify_disagreements(got, ref, rays, kd, tri, pos)
    print("%s/%s: %s, ids agree on %.5f of the considered rays" % (scene, builder, counts, agree))
    assert other.size == 0, (scene, builder, other[:5], got[other[:5]], ref[other[:5]])
    assert agree >= 0.999
