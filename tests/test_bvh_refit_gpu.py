"""ntr_bvh_refit on the device: nodes (all 64 bytes of every slot), triWoop and the scene box equal the numpy spec
(tests/np_bvh_refit.py) byte for byte for trees of every builder, every deformation and two epsilons; refits are deterministic and
carry no state but the scratch; triIndex, link words, terminators and the bytes around the buffers stay; trace records over the
refitted tree equal the oracle's for every kernel name; the asynchronous form chains with a trace on one stream and replays from a
HIP graph; the hairball refits, validates and traces; the scratch grows, is reported and released.

Brute force (oracle.bruteforce_closest) runs over the edge rays and every 512th of the 1080p primary rays: all 2 M rays against
262 k triangles are 5e11 triangle tests on the CPU; the oracle's traversal, which every ray is compared with, is itself held to brute
force on the CPU tier."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_bvh_refit as rf
import ray_sets
import test_persistent_bvh_gpu as tp
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256
BUILDERS = ("sah", "lbvh", "hlbvh", "binned")
SCENES = ("cornell", "soup1500", "atrium", "one", "stacked", "flat", "zero_area")
DEFORMATIONS = (0.0, 0.02, 0.3, "collapse")
_trees = {}


def _bbox(pos):
    mn, mx = oracle.scene_bbox(np.ascontiguousarray(pos, F))
    return np.asarray(mn, F), np.asarray(mx, F)


def _build(kind, tri, pos):
    """Host copies (nodes uint8, woop uint8, tri_index int32) of a tree of `kind` over the mesh."""
    tri, pos = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F)
    if kind == "sah":
        h = nt.sah_build(tri, pos)
        return h.nodes.copy(), h.woop.copy(), h.tri_index.copy()
    n = tri.shape[0]
    d_tri, d_pos = up(tri), up(pos)
    capn, capw, capi = nt.lbvh_capacity(n)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
    mn, mx = _bbox(pos)
    ptrs = (bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw, bufs[2].data_ptr(), capi)
    if kind == "lbvh":
        r = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, *ptrs)
    elif kind == "hlbvh":
        r = nt.hlbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, 4, *ptrs).lbvh
    else:
        r = nt.persistent_bvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, *ptrs)
    torch.cuda.synchronize()
    return (bufs[0].cpu().numpy()[:r.nodesBytes].copy(), bufs[1].cpu().numpy()[:r.triWoopBytes].copy(),
            bufs[2].cpu().numpy()[:r.triIndexBytes].view(np.int32).copy())


def _tree(name, kind):
    if (name, kind) not in _trees:
        tri, pos = tp._scene(name)
        _trees[(name, kind)] = _build(kind, tri, pos)
    return _trees[(name, kind)]


def _guarded(a):
    """A device copy of `a` with GUARD bytes of 0xAB on either side."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = np.full(GUARD, 0xAB, np.uint8)
    return up(np.concatenate([g, a, g]))


class _Dev:
    """A tree and a mesh on the device, the tree between guard bytes."""

    def __init__(self, nodes, woop, idx, tri, pos):
        self.nb, self.wb, self.ib = nodes.nbytes, woop.nbytes, idx.nbytes
        self.d_nodes, self.d_woop, self.d_idx = _guarded(nodes), _guarded(woop), _guarded(idx)
        self.d_box = _guarded(np.zeros(6, F))
        self.tri = np.ascontiguousarray(tri, np.int32)
        self.d_tri, self.d_pos = up(self.tri), up(np.ascontiguousarray(pos, F))
        self.num_verts = np.asarray(pos).reshape(-1, 3).shape[0]

    def ptr(self, t):
        return t.data_ptr() + GUARD

    def refit(self, eps, stream=0, blocking=True, box=True):
        return nt.bvh_refit(self.ptr(self.d_nodes), self.nb, self.ptr(self.d_woop), self.wb, self.ptr(self.d_idx), self.ib, self.tri.shape[0],
                            self.d_tri.data_ptr(), self.num_verts, self.d_pos.data_ptr(), eps, self.ptr(self.d_box) if box else 0, stream,
                            blocking)

    def set_pos(self, pos):
        self.d_pos.copy_(up(np.ascontiguousarray(pos, F)))

    def download(self):
        torch.cuda.synchronize()
        out = []
        for t in (self.d_nodes, self.d_woop, self.d_idx, self.d_box):
            h = t.cpu().numpy()
            assert (h[:GUARD] == 0xAB).all() and (h[-GUARD:] == 0xAB).all(), "bytes outside the buffer were written"
            out.append(h[GUARD:-GUARD].copy())
        return out[0], out[1], out[2].view(np.int32), out[3].view(F)


def _assert_equals_spec(d, idx, spec, res=None, what=""):
    nodes, woop, gidx, box = d.download()
    assert np.array_equal(gidx, idx), "%s: triIndex changed" % (what,)
    assert np.array_equal(nodes.view(np.int32).reshape(-1, 16), spec["nodes"]), "%s: nodes differ" % (what,)
    assert np.array_equal(woop, spec["woop"]), "%s: triWoop differs" % (what,)
    assert box.tobytes() == spec["scene_box"].tobytes(), "%s: scene box differs" % (what,)
    if res is not None:
        assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == spec["stats"], what
        assert res.seconds > 0


@pytest.mark.parametrize("kind", BUILDERS)
@pytest.mark.parametrize("name", SCENES)
def test_device_refit_equals_spec(name, kind):
    tri, pos = tp._scene(name)
    nodes, woop, idx = _tree(name, kind)
    for how in DEFORMATIONS:
        p = rf.moved(pos, how)
        for eps in (0.0, 0.001):
            d = _Dev(nodes, woop, idx, tri, p)
            res = d.refit(eps)
            _assert_equals_spec(d, idx, rf.refit(nodes, woop, idx, tri, p, eps), res, (name, kind, how, eps))
    print("%s %s: %d tris, %d nodes, refit %.1f us" % (name, kind, tri.shape[0], res.numNodes, res.seconds * 1e6))


def test_seeded_soups_equal_spec():
    rng = np.random.default_rng(20261016)
    for i in range(50):
        n = int(rng.integers(20000, 50001)) if i % 10 == 9 else int(rng.integers(1, 3000))
        if i == 0:
            n = 1
        tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        p = rf.deform(pos, 0.02)
        for kind in ("lbvh", "binned"):
            nodes, woop, idx = _build(kind, tri, pos)
            nodes = np.concatenate([nodes, np.zeros(64, np.uint8)])   # a slot no link reaches, inside the extent
            d = _Dev(nodes, woop, idx, tri, p)
            res = d.refit(0.001)
            spec = rf.refit(nodes, woop, idx, tri, p, 0.001)
            _assert_equals_spec(d, idx, spec, res, (i, n, kind))
            assert not spec["nodes"][-1].any()


def test_deterministic_across_streams_and_stateless():
    tri, pos = tp._scene("atrium")
    nodes, woop, idx = _tree("atrium", "lbvh")
    pa, pb = rf.deform(pos, 0.02), rf.deform(pos, 0.3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = _Dev(nodes, woop, idx, tri, pb), _Dev(nodes, woop, idx, tri, pb)
    torch.cuda.synchronize()
    # one refit per device at a time (they share the scratch): the second stream waits for the first
    with torch.cuda.stream(s1):
        a.refit(0.001, s1.cuda_stream, blocking=False)
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        b.refit(0.001, s2.cuda_stream, blocking=False)
    ga, gb = a.download(), b.download()
    for x, y in zip(ga, gb):
        assert x.tobytes() == y.tobytes()
    c = _Dev(nodes, woop, idx, tri, pa)
    c.refit(0.001)
    c.set_pos(pb)
    c.refit(0.001)
    for x, y in zip(c.download(), ga):
        assert x.tobytes() == y.tobytes()
    _assert_equals_spec(c, idx, rf.refit(nodes, woop, idx, tri, pb, 0.001))


def test_links_terminators_and_tri_index_are_unchanged():
    tri, pos = tp._scene("soup1500")
    for kind in BUILDERS:
        nodes, woop, idx = _tree("soup1500", kind)
        d = _Dev(nodes, woop, idx, tri, rf.deform(pos, 0.3))
        d.refit(0.001, box=False)
        gn, gw, gi, gbox = d.download()
        assert not gbox.view(np.uint32).any()          # no scene box asked for, none written
        assert np.array_equal(gi, idx)
        assert np.array_equal(gn.view(np.int32).reshape(-1, 16)[:, 12:], nodes.view(np.int32).reshape(-1, 16)[:, 12:])
        w0, w1 = woop.view(np.uint32).reshape(-1, 4), gw.view(np.uint32).reshape(-1, 4)
        ni = nodes.view(np.int32).reshape(-1, 16)
        rows = rf.leaf_rows(ni, w0, rf.levels_of(ni))[3]
        keep = np.ones(w0.shape[0], bool)
        for j in range(3):
            keep[rows + j] = False
        assert keep.sum() == ni.shape[0] + 1 or kind in ("lbvh", "hlbvh")   # one terminator per leaf (LBVH extents may hold spare rows)
        assert np.array_equal(w0[keep], w1[keep]) and (w1[keep][:, 0] == rf.TERM).sum() >= ni.shape[0] + 1


def _trace(d, flags, d_rays, n, kernel, any_hit, stream=0, timed=True):
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    nt.trace_bvh(kernel, n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d.ptr(d.d_nodes), d.nb, d.ptr(d.d_woop), d.wb, d.ptr(d.d_idx),
                 bvh_flags=flags, stream=stream, timed=timed)
    return d_res


def _records(d_res):
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(nt.RESULT_DTYPE)


def _check_records(d, rays, what, monkeypatch, brute=None):
    flags = nt.bvh_validate(d.ptr(d.d_nodes), d.nb)
    gn, gw, gi, _ = d.download()
    d_rays = up(rays)
    refs = {ah: oracle.trace(gn, gw, gi, rays, any_hit=ah, threads=16)[0] for ah in (False, True)}
    if brute is not None:
        bf = oracle.bruteforce_closest(gw, gi, rays[brute])
        assert np.array_equal(refs[False]["t"][brute].view(np.uint32), bf["t"].view(np.uint32)), what
    try:
        for route in ("0", "1"):
            monkeypatch.setenv("NTR_TRACE_ROUTE", route)
            nt.set_tunables()
            for kernel in nt.KERNELS:
                for ah in (False, True):
                    tp._assert_records(_records(_trace(d, flags, d_rays, rays.shape[0], kernel, ah)), refs[ah], ah, (what, route, kernel, ah))
    finally:
        monkeypatch.delenv("NTR_TRACE_ROUTE", raising=False)
        nt.set_tunables()
    assert nt.trace_status() == 0


@pytest.mark.parametrize("kind", BUILDERS)
def test_trace_records_over_the_refitted_tree_equal_oracle(kind, monkeypatch):
    tri, pos, cam = scenes.atrium()
    nodes, woop, idx = _tree("atrium", kind)
    p = rf.deform(pos, 0.02)
    d = _Dev(nodes, woop, idx, tri, p)
    d.refit(0.0 if kind == "sah" else 0.001)
    edge = ray_sets.edge_rays(float(np.abs(p).max()))
    _check_records(d, edge, (kind, "edge"), monkeypatch, brute=np.arange(edge.shape[0]))
    if kind in ("sah", "lbvh"):
        prim = scenes.primary_rays(cam, 1920, 1080)[0]
        _check_records(d, prim, (kind, "1080p"), monkeypatch, brute=np.arange(0, prim.shape[0], 512))


def test_asynchronous_refit_then_trace_on_one_stream_and_from_a_graph():
    tri, pos, cam = scenes.atrium()
    nodes, woop, idx = _tree("atrium", "lbvh")
    rays = np.concatenate([scenes.primary_rays(cam, 320, 240)[0], scenes.random_rays(20000, 5, extent=float(np.abs(pos).max()))])
    n = rays.shape[0]
    d_rays = up(rays)
    uploads = [rf.deform(pos, 0.02), rf.deform(pos, 0.3)]
    refs = []
    for p in uploads:
        spec = rf.refit(nodes, woop, idx, tri, p, 0.001)
        refs.append((spec, oracle.trace(spec["nodes"].view(np.uint8).reshape(-1), spec["woop"], idx, rays, threads=16)[0]))
    kernel = "fermi_speculative_while_while"
    d = _Dev(nodes, woop, idx, tri, uploads[0])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # result = NULL on a non-default stream, the trace behind it without a host synchronisation in between
    with torch.cuda.stream(s):
        _trace(d, 0, d_rays, n, kernel, False, s.cuda_stream, timed=False)   # the trace's scratch and tables exist from here on
        d.refit(0.001, s.cuda_stream, blocking=False)
        d_res = _trace(d, 0, d_rays, n, kernel, False, s.cuda_stream, timed=False)
    tp._assert_records(_records(d_res), refs[0][1], False, "asynchronous pair")
    _assert_equals_spec(d, idx, refs[0][0])
    # the same pair as a graph: one stream, a linear chain; replayed after each vertex upload (the scratch and the trace's tables exist)
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d.refit(0.001, cs, blocking=False)
        nt.trace_bvh(kernel, n, False, d_rays.data_ptr(), d_res.data_ptr(), d.ptr(d.d_nodes), d.nb, d.ptr(d.d_woop), d.wb, d.ptr(d.d_idx),
                     stream=cs, timed=False)
    for rep, which in enumerate((1, 0, 1)):
        d.set_pos(uploads[which])
        d_res.fill_(0xCD)
        torch.cuda.synchronize()
        g.replay()
        tp._assert_records(_records(d_res), refs[which][1], False, "graph replay %d" % rep)
        _assert_equals_spec(d, idx, refs[which][0], what="graph replay %d" % rep)
    del g
    # a captured call cannot allocate or read back
    nt.lbvh_release_workspace()
    g2 = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g2, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d_res.fill_(0xCD)   # so that the graph is not empty
        for blocking in (False, True):
            try:
                d.refit(0.001, cs, blocking=blocking)
            except nt.NtrError as e:
                errs.append(e.code)
    assert errs == [-1, -1]


def test_hairball_refits_validates_and_traces_and_the_scratch_is_released():
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_scratch_bytes() == 0
    tri, pos, _ = scenes.random_soup(2000, seed=3)
    nodes, woop, idx = _build("lbvh", tri, pos)
    _Dev(nodes, woop, idx, tri, pos).refit(0.001)
    small = nt.bvh_refit_scratch_bytes()
    assert small >= 8 * (nodes.nbytes // 64)
    tri, pos, cam = scenes.hairball()
    nodes, woop, idx = _build("lbvh", tri, pos)
    p = rf.deform(pos, 0.02)
    d = _Dev(nodes, woop, idx, tri, p)
    res = d.refit(0.001)
    big = nt.bvh_refit_scratch_bytes()
    assert big > small and big >= 8 * (nodes.nbytes // 64)
    assert res.numLeaves == res.numNodes + 1 and res.numRows == 3 * tri.shape[0] + res.numLeaves
    flags = nt.bvh_validate(d.ptr(d.d_nodes), d.nb)
    assert flags & nt.BVH_FINITE and flags & nt.BVH_ORDERED
    rays = scenes.primary_rays(cam, 256, 256)[0]
    nt.trace_status()
    got = _records(_trace(d, flags, up(rays), rays.shape[0], "fermi_speculative_while_while", False))
    assert nt.trace_status() == 0
    gn, gw, gi, box = d.download()
    ref, _ = oracle.trace(gn, gw, gi, rays, threads=16)
    tp._assert_records(got, ref, False, "hairball")
    assert (got["id"] >= 0).mean() > 0.1
    mn, mx = _bbox(p)
    assert np.array_equal(box, np.concatenate([mn - F(0.001), mx + F(0.001)]).astype(F))
    print("hairball %d: %d nodes, refit %.3f ms" % (tri.shape[0], res.numNodes, res.seconds * 1e3))
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_scratch_bytes() == 0
