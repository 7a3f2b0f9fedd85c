"""On-device HLBVH build (ntr_hlbvh_build) against the restatement tests/np_hlbvh.py, in canonical form, and traces through its trees."""
import time

import numpy as np
import pytest

import hlbvh_scenes as S
import np_hlbvh as H
import ray_sets
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


def assert_same_tree(got, ref, what):
    """The canonical hash is the criterion; on a mismatch the message names the first differing node."""
    if hash_of(got) != H.canonical_hash(ref):
        ref_bufs = dict(nodes=ref["nodes"], woop=ref["woop"], tri_index=ref["tri_index"])
        pytest.fail("%s: canonical hashes differ; %s" % (what, S.first_difference(got, ref_bufs) or "no node differs in the walk"))


def check_same(tri, pos, bits, leaf_size, bbox=None):
    ref = H.hlbvh_build(tri, pos, bits, leaf_size=leaf_size, bbox=bbox)
    got = dev_build(tri, pos, bits, leaf_size, bbox=bbox)
    assert_same_tree(got, ref, (tri.shape[0], bits, leaf_size))
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


# ---- the named scenes of hlbvh_scenes.py: kernel seams and decision cases (their claims are asserted on the CPU tier) ----
def build_scene(name):
    tri, pos, bits, leaf_size, eps, bbox = S.scene(name)
    return dev_build(tri, pos, bits, leaf_size, eps=eps, bbox=bbox)


def fields(t):
    r = t["res"]
    return (r.numClusters, r.topLevels, r.topNodes, r.lbvh.numNodes, r.lbvh.numLeaves, r.lbvh.nodesBytes, r.lbvh.triWoopBytes,
            r.lbvh.triIndexBytes)


def spec_fields(ref):
    top = (0, 0, 0) if ref["lbvh_path"] else (ref["num_clusters"], ref["top_levels"], ref["top_nodes"])
    return top + (ref["num_inner"], ref["num_leaves"], ref["nodes"].nbytes, ref["woop"].nbytes, ref["tri_index"].nbytes)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_named_scene_matches_restatement(name):
    t0 = time.perf_counter()
    ref = S.build_spec(name)      # built anew, so that the printed time is a build's and not a cache look-up's
    t1 = time.perf_counter()
    got = build_scene(name)
    t2 = time.perf_counter()
    print("%s (%s): spec %.2f s, device %.3f s" % (name, S.claim(name), t1 - t0, t2 - t1))
    assert_same_tree(got, ref, name)
    assert fields(got) == spec_fields(ref), name


def test_builds_are_the_same_on_every_stream_and_after_a_release():
    name = "cluster_box"
    ref = S.spec(name)
    seen = []
    for stream in (None, torch.cuda.Stream(), torch.cuda.Stream()):
        if stream is None:
            t = build_scene(name)
        else:
            with torch.cuda.stream(stream):
                t = build_scene(name)
        seen.append((hash_of(t), fields(t)))
    nt.lbvh_release_workspace()
    t = build_scene(name)
    seen.append((hash_of(t), fields(t)))
    assert seen == [(H.canonical_hash(ref), spec_fields(ref))] * 4


@pytest.mark.parametrize("name", ["part_c1025", "cluster_box", "leaf_exact"])
def test_exact_capacity_is_enough_and_nothing_else_is_written(name):
    """part_c1025 is the worst case of the capacity (bits 0 and leaf size 1 give n leaves and n - 1 inner nodes); the other two leave
    real slack between the reported extents and the capacity (leaf size 4), which must keep its prefill."""
    tri, pos, bits, leaf_size, eps, bbox = S.scene(name)
    n = tri.shape[0]
    ref = S.spec(name)
    worst = name == "part_c1025"
    assert (bits == 0 and leaf_size == 1 and ref["num_leaves"] == n and ref["num_inner"] == n - 1) == worst
    caps = nt.lbvh_capacity(n)
    guard, fill = 4096, 0xAB
    d_tri, d_pos = up(tri), up(pos)
    bufs = [torch.full((c + 2 * guard,), fill, dtype=torch.uint8, device="cuda") for c in caps]
    ptrs = [b.data_ptr() + guard for b in bufs]
    res = nt.hlbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), bbox[0], bbox[1], leaf_size, eps, bits, ptrs[0], caps[0],
                         ptrs[1], caps[1], ptrs[2], caps[2], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    ext = (res.lbvh.nodesBytes, res.lbvh.triWoopBytes, res.lbvh.triIndexBytes)
    assert ext == (ref["nodes"].nbytes, ref["woop"].nbytes, ref["tri_index"].nbytes)
    if worst:
        assert ext == (64 * (n - 1), 16 * 4 * n, 4 * 4 * n)
    else:      # at least a quarter of the node slots and a tenth of the entries stay unused
        assert ext[0] < 0.75 * caps[0] and ext[1] < 0.9 * caps[1] and ext[2] < 0.9 * caps[2]
    for h, c, e in zip(host, caps, ext):
        assert e <= c
        assert (h[:guard] == fill).all() and (h[guard + c:] == fill).all()      # nothing outside the capacity
        assert (h[guard + e:guard + c] == fill).all()                            # nor past the reported extents (see the header)
    got = dict(nodes=host[0][guard:guard + ext[0]], woop=host[1][guard:guard + ext[1]],
               tri_index=host[2][guard:guard + ext[2]].copy().view(np.int32), res=res)
    assert_same_tree(got, ref, name)


@pytest.mark.parametrize("name", ["cluster_box", "missed_1025", "host_slivers"])
def test_traces_through_named_trees_match_the_oracle(name):
    tri, pos = S.scene(name)[:2]
    t = build_scene(name)
    assert_same_tree(t, S.spec(name), name)
    d_nodes, d_woop, d_idx = up(t["nodes"]), up(t["woop"]), up(t["tri_index"])
    view = nt.BvhView(d_nodes.data_ptr(), t["nodes"].nbytes, d_woop.data_ptr(), t["woop"].nbytes, d_idx.data_ptr())
    view.validate()
    edge = ray_sets.edge_rays()
    rays = np.concatenate([edge, S.aimed_rays(tri, pos, 4096 - edge.shape[0], 11)])
    assert rays.shape[0] == 4096
    d_rays = up(rays)
    refs = {any_hit: oracle.trace(t["nodes"], t["woop"], t["tri_index"], rays, any_hit=any_hit)[0] for any_hit in (False, True)}
    assert (refs[False]["id"] >= 0).sum() > 500
    for kernel in nt.KERNELS:
        for any_hit in (False, True):
            d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda")
            view.trace(kernel, rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
            got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
            assert np.array_equal(got["id"], refs[any_hit]["id"]), (kernel, any_hit)
            assert np.array_equal(got["t"].view(np.uint32), refs[any_hit]["t"].view(np.uint32)), (kernel, any_hit)


def test_a_capturing_stream_is_refused():
    """Both builds read counts back and synchronise: inside a capture they are refused before anything is allocated or launched, the
    capture stays valid and replays, and the output buffers keep their prefill."""
    tri, pos, bits, leaf_size, eps, bbox = S.scene("leaf_exact")
    n = tri.shape[0]
    caps = nt.lbvh_capacity(n)
    d_tri, d_pos = up(tri), up(pos)
    outs = [torch.full((c,), 0xAB, dtype=torch.uint8, device="cuda") for c in caps]
    marker = torch.zeros(64, dtype=torch.uint8, device="cuda")
    nt.lbvh_release_workspace()      # a call that got past the check would have to allocate
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        marker.fill_(7)              # the one other node of the graph
        for call in ("hlbvh", "lbvh"):
            args = (n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), bbox[0], bbox[1], leaf_size, eps)
            tail = (outs[0].data_ptr(), caps[0], outs[1].data_ptr(), caps[1], outs[2].data_ptr(), caps[2], cs)
            try:
                if call == "hlbvh":
                    nt.hlbvh_build(*args, bits, *tail)
                else:
                    nt.lbvh_build(*args, *tail)
            except nt.NtrError as e:
                errs.append((call, e.code, "captured" in str(e)))
    assert errs == [("hlbvh", -1, True), ("lbvh", -1, True)]
    torch.cuda.synchronize()
    assert int(marker.max()) == 0    # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert (marker == 7).all()
    for o in outs:
        assert (o == 0xAB).all()
    # and outside a capture the same arguments build
    assert_same_tree(build_scene("leaf_exact"), S.spec("leaf_exact"), "after the capture")
