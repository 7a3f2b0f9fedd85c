"""On-device HLBVH build (ntr_hlbvh_build) against the restatement tests/np_hlbvh.py, in canonical form, and traces through its trees."""
import numpy as np
import pytest

import np_hlbvh as H
import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def dev_build(tri, pos, bits, leaf_size=8, eps=0.001, bbox=None, bufs=None):
    tri = np.ascontiguousarray(tri, np.int32)
    pos = np.ascontiguousarray(pos, np.float32)
    n = tri.shape[0]
    mn, mx = bbox if bbox is not None else oracle.scene_bbox(pos)
    capn, capw, capi = nt.lbvh_capacity(n)
    d_tri, d_pos = up(tri), up(pos)
    ln = torch.zeros(capn, dtype=torch.uint8, device="cuda")
    lw = torch.zeros(capw, dtype=torch.uint8, device="cuda")
    li = torch.zeros(capi, dtype=torch.uint8, device="cuda")
    res = nt.hlbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, leaf_size, eps, bits, ln.data_ptr(), capn,
                         lw.data_ptr(), capw, li.data_ptr(), capi, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = res.lbvh
    return dict(nodes=ln.cpu().numpy()[:r.nodesBytes], woop=lw.cpu().numpy()[:r.triWoopBytes],
                tri_index=li.cpu().numpy()[:r.triIndexBytes].view(np.int32), res=res)


def hash_of(t):
    return oracle.bvh_canonical_hash(t["nodes"], t["woop"], t["tri_index"])


def check_same(tri, pos, bits, leaf_size, bbox=None):
    ref = H.hlbvh_build(tri, pos, bits, leaf_size=leaf_size, bbox=bbox)
    got = dev_build(tri, pos, bits, leaf_size, bbox=bbox)
    assert hash_of(got) == H.canonical_hash(ref), (tri.shape[0], bits, leaf_size)
    r = got["res"]
    assert r.lbvh.numNodes == ref["num_inner"] and r.lbvh.numLeaves == ref["num_leaves"]
    assert r.lbvh.nodesBytes == ref["nodes"].nbytes and r.lbvh.triWoopBytes == ref["woop"].nbytes
    if not ref["lbvh_path"]:
        assert r.numClusters == ref["num_clusters"] and r.topLevels == ref["top_levels"] and r.topNodes == ref["top_nodes"]
    return got, ref


@pytest.mark.parametrize("bits,leaf_size,n,seed", [
    (0, 1, 1500, 1), (0, 4, 4000, 2), (1, 8, 8000, 3), (1, 32, 5000, 4), (4, 1, 8000, 5), (4, 8, 20000, 6), (4, 4, 30000, 7),
    (7, 8, 30000, 8), (7, 32, 100000, 9), (9, 1, 3000, 10), (9, 8, 50000, 11), (2, 8, 8000, 12), (4, 32, 12000, 13)])
def test_random_soups_match_restatement(bits, leaf_size, n, seed):
    tri, pos, _ = scenes.random_soup(n, seed=seed)
    check_same(tri, pos, bits, leaf_size)


def tris_at(points, size=1.0):
    pos, tri = [], []
    for i, p in enumerate(points):
        p = np.asarray(p, np.float32)
        pos += [p + (size, 0, 0), p + (0, size, 0), p]
        tri.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(tri, np.int32), np.array(pos, np.float32)


def test_special_scenes_match_restatement():
    rng = np.random.default_rng(3)
    box = (np.zeros(3, np.float32), np.full(3, 1024.0, np.float32))
    # clustered: a few dense blobs
    centers = rng.uniform(0, 1000, size=(12, 3))
    pts = np.concatenate([c + rng.normal(0, 8, size=(700, 3)) for c in centers]).clip(0, 1020)
    tri, pos = tris_at(pts)
    for bits in (1, 4, 7):
        check_same(tri, pos, bits, 8)
    # flat floor
    flat = rng.integers(0, 1000, size=(3000, 3)).astype(np.float32)
    flat[:, 2] = 0
    tri, pos = tris_at(flat)
    for bits in (0, 2, 4):
        check_same(tri, pos, bits, 4)
    # all identical triangles (one cluster, equal codes) and one cluster of distinct codes
    tri, pos = tris_at([(100, 100, 100)] * 2000)
    for bits in (1, 4, 9):
        check_same(tri, pos, bits, 2, bbox=box)
    tri, pos = tris_at(rng.integers(0, 500, size=(3000, 3)))
    got, ref = check_same(tri, pos, 9, 4, bbox=box)
    assert ref["num_clusters"] == 1
    # n <= leafSize and n = 1
    tri, pos = tris_at(rng.integers(0, 1000, size=(8, 3)))
    check_same(tri, pos, 4, 8)
    tri, pos = tris_at([(5, 5, 5)])
    check_same(tri, pos, 4, 1)
    check_same(tri, pos, 0, 1)


def test_bits10_is_lbvh_and_builds_are_deterministic():
    tri, pos, _ = scenes.random_soup(30000, seed=21)
    a = dev_build(tri, pos, 10)
    ln = oracle.lbvh_build(tri, pos, 8, 0.001)
    assert hash_of(a) == oracle.bvh_canonical_hash(ln["nodes"], ln["woop"], ln["tri_index"])
    hashes = {hash_of(dev_build(tri, pos, 4)) for _ in range(3)}
    assert len(hashes) == 1


@pytest.mark.parametrize("name", ["atrium", "hairball"])
def test_large_scenes_every_triangle_once(name):
    if name == "atrium":
        tri, pos, _ = scenes.atrium()
    else:
        tri, pos, _ = scenes.hairball()
    n = tri.shape[0]
    t = dev_build(tri, pos, 4)
    r = t["res"].lbvh
    idx = t["tri_index"]
    woop = t["woop"].view(np.uint32).reshape(-1, 4)
    live = woop[:, 0] != 0x80000000
    # entries 3k of a leaf hold triangle ids; terminators are single entries: walk leaf by leaf
    ids = []
    i = 0
    while i < idx.shape[0]:
        if not live[i]:
            i += 1
            continue
        ids.append(idx[i])
        i += 3
    ids = np.array(ids)
    assert ids.shape[0] == n and np.array_equal(np.sort(ids), np.arange(n))
    assert r.numNodes == r.numLeaves - 1
    assert r.triWoopBytes == (3 * n + r.numLeaves) * 16 and r.nodesBytes == 64 * r.numNodes


def test_trace_parity_on_hlbvh_trees():
    tri, pos, cam = scenes.random_soup(20000, seed=31)
    t = dev_build(tri, pos, 4)
    rays, _ = scenes.primary_rays(cam, 96, 96)
    d_nodes, d_woop, d_idx = up(t["nodes"]), up(t["woop"]), up(t["tri_index"])
    view = nt.BvhView(d_nodes.data_ptr(), t["nodes"].nbytes, d_woop.data_ptr(), t["woop"].nbytes, d_idx.data_ptr())
    view.validate()
    prim, _ = oracle.trace(t["nodes"], t["woop"], t["tri_index"], rays)
    hit = prim["id"] >= 0
    # an AO-like batch: short any-hit rays
    ray_sets = {"primary": (rays, False), "ao": (scenes.random_rays(rays.shape[0], 5, tmax=3.0), True)}
    for kernel in nt.KERNELS:
        for name, (rs, any_hit) in ray_sets.items():
            d_rays = up(rs)
            d_res = torch.zeros(rs.shape[0] * 16, dtype=torch.uint8, device="cuda")
            view.trace(kernel, rs.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
            got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
            ref, _ = oracle.trace(t["nodes"], t["woop"], t["tri_index"], rs, any_hit=any_hit)
            assert np.array_equal(got["id"], ref["id"]), (kernel, name)
            assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), (kernel, name)
    assert hit.any()
