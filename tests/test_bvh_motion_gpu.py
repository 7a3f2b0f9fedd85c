"""Deformation motion blur on the device: ntr_bvh_motion_refit equals the numpy spec (tests/np_bvh_motion.py) byte for byte -- both node
buffers, the Woop rows, both vertex-row buffers, the scene box -- and what ntr_bvh_refit itself leaves for either key, with triIndex,
the links and the bytes around every buffer untouched; ntr_trace_bvh_motion equals ntr_trace_bvh over either key's tree at the
shutter's ends, and inside the shutter the spec in all four result words and the static trace over the uploaded posed tree; the
instrumented kernel's counters are the spec's; per-ray times clamp; a collapsing key degenerates cleanly; the asynchronous pair chains
on one stream and replays from a HIP graph over new positions and times; the scratch grows, is reported and released.
Every comparison is bitwise."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
from oracle import oracle

import bvh_motion_cases as mc
import np_bvh_motion as bm
import np_bvh_refit as rf
from gpu_util import up

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256
KERNEL = "fermi_speculative_while_while"
TREES = [(name, "sah") for name in mc.SCENES] + [("cornell", "lbvh"), ("soup1500", "lbvh")]
_trees = {}


def _tree(name, kind):
    """Host copies (nodes uint8, woop uint8, tri_index int32) of the host SAH tree or the device LBVH over the scene."""
    if (name, kind) not in _trees:
        tri, pos = mc.scene(name)
        if kind == "sah":
            h = nt.sah_build(tri, pos)
            _trees[(name, kind)] = (h.nodes.copy(), h.woop.copy(), h.tri_index.copy())
        else:
            n = tri.shape[0]
            d_tri, d_pos = up(tri), up(pos)
            capn, capw, capi = nt.lbvh_capacity(n)
            bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
            mn, mx = oracle.scene_bbox(pos)
            r = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), np.asarray(mn, F), np.asarray(mx, F), 8, 0.001,
                              bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw, bufs[2].data_ptr(), capi)
            torch.cuda.synchronize()
            _trees[(name, kind)] = (bufs[0].cpu().numpy()[:r.nodesBytes].copy(), bufs[1].cpu().numpy()[:r.triWoopBytes].copy(),
                                    bufs[2].cpu().numpy()[:r.triIndexBytes].view(np.int32).copy())
    return _trees[(name, kind)]


def _spec(name, kind, how, eps):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    return mc.spec_of((name, kind), nodes, woop, idx, tri, pos, how, eps)


def _guarded(a):
    """A device copy of `a` with GUARD bytes of 0xAB on either side."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = np.full(GUARD, 0xAB, np.uint8)
    return up(np.concatenate([g, a, g]))


class _Dev:
    """A tree, its second-key buffers and a mesh with two position arrays on the device, every written buffer between guard bytes.
    nodes1 and the vertex rows start as 0xEE: the call initialises them."""
    NAMES = ("nodes0", "nodes1", "woop", "idx", "vrows0", "vrows1", "box")

    def __init__(self, nodes, woop, idx, tri, pos0, pos1):
        self.nb, self.wb, self.ib = nodes.nbytes, woop.nbytes, idx.nbytes
        self.t = dict(nodes0=_guarded(nodes), nodes1=_guarded(np.full(self.nb, 0xEE, np.uint8)), woop=_guarded(woop), idx=_guarded(idx),
                      vrows0=_guarded(np.full(self.wb, 0xEE, np.uint8)), vrows1=_guarded(np.full(self.wb, 0xEE, np.uint8)),
                      box=_guarded(np.zeros(6, F)))
        self.tri = np.ascontiguousarray(tri, np.int32)
        self.d_tri, self.d_pos0, self.d_pos1 = up(self.tri), _guarded(np.ascontiguousarray(pos0, F)), _guarded(np.ascontiguousarray(pos1, F))
        self.num_verts = np.asarray(pos0).reshape(-1, 3).shape[0]

    def p(self, name):
        return self.t[name].data_ptr() + GUARD

    def refit(self, eps, stream=0, blocking=True, box=True):
        return nt.bvh_motion_refit(self.p("nodes0"), self.nb, self.p("nodes1"), self.p("woop"), self.wb, self.p("idx"), self.ib, self.p("vrows0"),
                                   self.p("vrows1"), self.tri.shape[0], self.d_tri.data_ptr(), self.num_verts, self.d_pos0.data_ptr() + GUARD,
                                   self.d_pos1.data_ptr() + GUARD, eps, self.p("box") if box else 0, stream, blocking)

    def static_refit(self, key, eps):
        """ntr_bvh_refit itself, in place on nodes0 / woop, to the key's positions."""
        d_pos = (self.d_pos0, self.d_pos1)[key]
        return nt.bvh_refit(self.p("nodes0"), self.nb, self.p("woop"), self.wb, self.p("idx"), self.ib, self.tri.shape[0], self.d_tri.data_ptr(),
                            self.num_verts, d_pos.data_ptr() + GUARD, eps, self.p("box"))

    def set_pos1(self, pos):
        self.d_pos1.copy_(_guarded(np.ascontiguousarray(pos, F)))

    def motion(self, d_times=0, time=0.0):
        return nt.BvhMotion(self.p("nodes1"), self.p("vrows0"), self.p("vrows1"), d_times, time)

    def trace(self, d_rays, n, any_hit=False, d_times=0, time=0.0, stream=0, timed=True, d_res=None):
        if d_res is None:
            d_res = torch.full((max(n, 1) * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
        nt.trace_bvh_motion(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.p("nodes0"), self.nb, self.wb, self.p("idx"),
                            self.motion(d_times, time), stream, timed)
        return d_res

    def trace_stats(self, d_rays, n, any_hit=False, d_times=0, time=0.0):
        d_res = torch.full((max(n, 1) * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
        st = nt.trace_bvh_motion_stats(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.p("nodes0"), self.nb, self.wb, self.p("idx"),
                                       self.motion(d_times, time))
        return d_res, st

    def static_trace(self, d_rays, n, any_hit=False):
        d_res = torch.full((max(n, 1) * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
        nt.trace_bvh(KERNEL, n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), self.p("nodes0"), self.nb, self.p("woop"), self.wb, self.p("idx"))
        return d_res

    def download(self):
        torch.cuda.synchronize()
        out = {}
        for name in list(self.NAMES) + ["pos0", "pos1"]:
            h = (self.t[name] if name in self.t else getattr(self, "d_" + name)).cpu().numpy()
            assert (h[:GUARD] == 0xAB).all() and (h[-GUARD:] == 0xAB).all(), "bytes outside %s were written" % name
            out[name] = h[GUARD:-GUARD].copy()
        return out


def _records(d_res, n=None):
    torch.cuda.synchronize()
    r = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
    return r if n is None else r[:n]


def _assert_refit_equals_spec(d, nodes, idx, m, res=None, what=""):
    g = d.download()
    assert np.array_equal(g["idx"].view(np.int32), idx), (what, "triIndex changed")
    for key in ("nodes0", "nodes1"):
        gn = g[key].view(np.int32).reshape(-1, 16)
        assert np.array_equal(gn[:, 12:], nodes.view(np.int32).reshape(-1, 16)[:, 12:]), (what, key, "links changed")
        assert np.array_equal(gn, m[key]), (what, key)
    assert np.array_equal(g["woop"], m["woop"]), (what, "triWoop")
    for key in ("vrows0", "vrows1"):
        assert np.array_equal(g[key].view(np.uint32).reshape(-1, 4), m[key]), (what, key)
    assert g["box"].tobytes() == m["scene_box"].tobytes(), (what, "scene box")
    if res is not None:
        assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == m["stats"], what
        assert res.seconds > 0
    return g


@pytest.fixture
def route0(monkeypatch):
    monkeypatch.setenv("NTR_TRACE_ROUTE", "0")
    nt.set_tunables()
    yield
    monkeypatch.delenv("NTR_TRACE_ROUTE", raising=False)
    nt.set_tunables()


# ---- 1. the refit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", TREES)
def test_motion_refit_equals_spec_and_the_static_refit(name, kind):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    for how in mc.DEFORMATIONS:
        for eps in mc.EPSILONS:
            what = (name, kind, how, eps)
            m, pos1 = _spec(name, kind, how, eps)
            d = _Dev(nodes, woop, idx, tri, pos, pos1)
            res = d.refit(eps)
            g = _assert_refit_equals_spec(d, nodes, idx, m, res, what)
            # deterministic: a second object, and a second call on the first (the refit of a refitted tree to the same keys)
            e = _Dev(nodes, woop, idx, tri, pos, pos1)
            e.refit(eps)
            d.refit(eps)
            ge, gd = e.download(), d.download()
            for key in _Dev.NAMES:
                assert g[key].tobytes() == ge[key].tobytes() == gd[key].tobytes(), (what, key, "not deterministic")
            # what ntr_bvh_refit itself leaves on a copy of the input, key by key
            for key, nk in ((0, "nodes0"), (1, "nodes1")):
                s = _Dev(nodes, woop, idx, tri, pos, pos1)
                s.static_refit(key, eps)
                gs = s.download()
                assert gs["nodes0"].tobytes() == g[nk].tobytes(), (what, "ntr_bvh_refit's nodes, key %d" % key)
                if key == 0:
                    assert gs["woop"].tobytes() == g["woop"].tobytes(), (what, "ntr_bvh_refit's rows")
    print("%s %s: %d tris, %d nodes, motion refit %.1f us" % (name, kind, tri.shape[0], res.numNodes, res.seconds * 1e6))


def test_motion_refit_without_a_scene_box_writes_none():
    tri, pos = mc.scene("soup1500")
    nodes, woop, idx = _tree("soup1500", "sah")
    d = _Dev(nodes, woop, idx, tri, pos, rf.deform(pos, 0.3))
    d.refit(0.0, box=False)
    assert not d.download()["box"].any()


# ---- 2. the ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", TREES)
def test_ends_equal_the_static_trace_over_either_key(name, kind, route0):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    eps = 0.0 if kind == "sah" else 0.001
    rays = np.concatenate([mc.rays_of(name, "box"), mc.rays_of(name, "edge")])
    n, d_rays = rays.shape[0], up(rays)
    nt.trace_status()
    for how in (0.02, 0.3):
        m, pos1 = _spec(name, kind, how, eps)
        d = _Dev(nodes, woop, idx, tri, pos, pos1)
        d.refit(eps)
        for key, time in ((0, 0.0), (1, 1.0)):
            s = _Dev(nodes, woop, idx, tri, pos, pos1)
            s.static_refit(key, eps)
            for any_hit in (False, True):
                got, ref = _records(d.trace(d_rays, n, any_hit, time=time)), _records(s.static_trace(d_rays, n, any_hit))
                bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != ref.view(np.uint32).reshape(-1, 4)).any(axis=1))
                print("%s %s %s key %d any_hit %d: %d of %d records differ" % (name, kind, how, key, any_hit, bad.size, n))
                assert bad.size == 0, (name, kind, how, key, any_hit, bad[:4])
    assert nt.trace_status() == 0


# ---- 3. inside the shutter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", TREES)
def test_inside_the_shutter_equals_spec_and_the_posed_static_tree(name, kind, route0):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    eps = 0.0 if kind == "sah" else 0.001
    rays = np.concatenate([mc.rays_of(name, "box"), mc.rays_of(name, "edge")])
    n, d_rays = rays.shape[0], up(rays)
    nt.trace_status()
    for how in (0.02, 0.3):
        m, pos1 = _spec(name, kind, how, eps)
        d = _Dev(nodes, woop, idx, tri, pos, pos1)
        d.refit(eps)
        for time in mc.TIMES:
            what = (name, kind, how, time)
            ref = mc.spec_trace(m, idx, rays, time=time, stats=True)
            mc.assert_records_equal_spec(_records(d.trace(d_rays, n, time=time)), ref, what)
            d_res, st = d.trace_stats(d_rays, n, time=time)
            mc.assert_records_equal_spec(_records(d_res), ref, (what, "stats kernel"))
            got = dict(numInnerVisits=st.numInnerVisits, numTriTests=st.numTriTests, numLeafVisits=st.numLeafVisits, numHits=st.numHits)
            assert got == ref[4] and st.numRays == n, (what, got, ref[4])
            # the uploaded posed static tree under ntr_trace_bvh
            pn, pw = bm.posed_static_tree(m, idx, tri, pos, pos1, time)
            s = _Dev(pn.view(np.uint8).reshape(-1), pw, idx, tri, pos, pos1)
            posed = _records(s.static_trace(d_rays, n))
            mc.assert_records_equal_spec(posed, ref, (what, "posed static tree"))
        ah = mc.spec_trace(m, idx, rays, any_hit=True, time=0.37, stats=True)
        d_res, st = d.trace_stats(d_rays, n, any_hit=True, time=0.37)
        mc.assert_records_equal_spec(_records(d_res), ah, (name, kind, how, "any hit"))
        assert dict(numInnerVisits=st.numInnerVisits, numTriTests=st.numTriTests, numLeafVisits=st.numLeafVisits, numHits=st.numHits) == ah[4]
        mc.assert_records_equal_spec(_records(d.trace(d_rays, n, any_hit=True, time=0.37)), ah, (name, kind, how, "any hit"))
    assert nt.trace_status() == 0


def test_the_middle_of_the_shutter_differs_from_both_keys_on_the_device():
    tri, pos = mc.scene("soup1500")
    nodes, woop, idx = _tree("soup1500", "sah")
    m, pos1 = _spec("soup1500", "sah", 0.02, 0.0)
    d = _Dev(nodes, woop, idx, tri, pos, pos1)
    d.refit(0.0)
    rays = mc.rays_of("soup1500", "box")
    d_rays = up(rays)
    mid, k0, k1 = (_records(d.trace(d_rays, rays.shape[0], time=t)).view(np.uint32).reshape(-1, 4) for t in (0.5, 0.0, 1.0))
    both = (mid != k0).any(axis=1) & (mid != k1).any(axis=1)
    print("records at t = 0.5 that differ from both keys': %d of %d" % (both.sum(), rays.shape[0]))
    assert both.any()


# ---- 4. per-ray times --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("soup1500", "sah"), ("soup1500", "lbvh"), ("cornell", "sah"), ("one", "sah")])
def test_per_ray_times_equal_spec(name, kind):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    eps = 0.0 if kind == "sah" else 0.001
    m, pos1 = _spec(name, kind, 0.02, eps)
    d = _Dev(nodes, woop, idx, tri, pos, pos1)
    d.refit(eps)
    nt.trace_status()
    for batch in ("box", "tail", "single", "edge"):
        rays = mc.rays_of(name, batch)
        n = rays.shape[0]
        times = mc.hashed_times(n)
        d_rays, d_times = up(rays), up(times)
        for any_hit in (False, True):
            ref = mc.spec_trace(m, idx, rays, any_hit, times=times, time=0.9, stats=True)
            got = _records(d.trace(d_rays, n, any_hit, d_times.data_ptr(), time=0.9), n)
            mc.assert_records_equal_spec(got, ref, (name, kind, batch, any_hit))
        d_res, st = d.trace_stats(d_rays, n, True, d_times.data_ptr())
        mc.assert_records_equal_spec(_records(d_res, n), ref, (name, kind, batch, "stats"))
        assert (st.numInnerVisits, st.numTriTests, st.numLeafVisits, st.numHits) == tuple(ref[4][k] for k in bm.COUNTERS)
    assert nt.trace_status() == 0


# ---- 5. a collapsing key -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("soup1500", "sah"), ("cornell", "lbvh"), ("stacked", "sah")])
def test_collapse_as_key_1_equals_spec_and_the_status_stays_clean(name, kind):
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    eps = 0.0 if kind == "sah" else 0.001
    m, pos1 = _spec(name, kind, "collapse", eps)
    d = _Dev(nodes, woop, idx, tri, pos, pos1)
    d.refit(eps)
    rays = np.concatenate([mc.rays_of(name, "box"), mc.rays_of(name, "edge")])
    n, d_rays = rays.shape[0], up(rays)
    nt.trace_status()
    for time in (0.5, 0.999, float(np.nextafter(F(1), F(0))), 1.0):
        ref = mc.spec_trace(m, idx, rays, time=time)
        mc.assert_records_equal_spec(_records(d.trace(d_rays, n, time=time)), ref, (name, kind, time))
    times = (1.0 - np.random.default_rng(3).random(n) ** 8).astype(F)      # crowded toward 1
    ref = mc.spec_trace(m, idx, rays, times=times)
    d_times = up(times)
    mc.assert_records_equal_spec(_records(d.trace(d_rays, n, d_times=d_times.data_ptr())), ref, (name, kind, "per ray"))
    print("%s %s: %d of %d rays hit the collapsing mesh" % (name, kind, int((ref[0] >= 0).sum()), n))
    assert nt.trace_status() == 0


# ---- 6. asynchronous, and from a graph ---------------------------------------------------------------------------------------------
def test_asynchronous_pair_on_one_stream_and_from_a_graph():
    name, kind, eps = "soup1500", "sah", 0.0
    tri, pos = mc.scene(name)
    nodes, woop, idx = _tree(name, kind)
    rays = mc.rays_of(name, "tail")
    n, d_rays = rays.shape[0], up(rays)
    keys = [rf.deform(pos, 0.02), rf.deform(pos, 0.3)]
    times = [mc.hashed_times(n, 9), mc.hashed_times(n, 10)]
    refs = []
    for p1, t in zip(keys, times):
        m = bm.motion_refit(nodes, woop, idx, tri, pos, p1, eps)
        refs.append((m, mc.spec_trace(m, idx, rays, times=t)))
    d = _Dev(nodes, woop, idx, tri, pos, keys[0])
    d_times = up(times[0])
    s = torch.cuda.Stream()
    nt.trace_status()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d.refit(eps, s.cuda_stream, blocking=False)
        d_res = d.trace(d_rays, n, d_times=d_times.data_ptr(), stream=s.cuda_stream, timed=False)
    s.synchronize()
    assert nt.trace_status() == 0
    mc.assert_records_equal_spec(_records(d_res), refs[0][1], "asynchronous pair")
    _assert_refit_equals_spec(d, nodes, idx, refs[0][0], what="asynchronous pair")
    # the same two calls as a graph (the uncaptured call above has grown the pool), replayed after key 1 and the times changed
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda:0")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d.refit(eps, cs, blocking=False)
        d.trace(d_rays, n, d_times=d_times.data_ptr(), stream=cs, timed=False, d_res=d_res)
    for rep, which in enumerate((1, 0, 1)):
        d.set_pos1(keys[which])
        d_times.copy_(up(times[which]))
        d_res.fill_(0xCD)
        torch.cuda.synchronize()
        g.replay()
        mc.assert_records_equal_spec(_records(d_res), refs[which][1], "graph replay %d" % rep)
        _assert_refit_equals_spec(d, nodes, idx, refs[which][0], what="graph replay %d" % rep)
    assert nt.trace_status() == 0
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
                d.refit(eps, cs, blocking=blocking)
            except nt.NtrError as e:
                errs.append(e.code)
    assert errs == [-1, -1]


# ---- 7. the scratch ----------------------------------------------------------------------------------------------------------------
def test_scratch_grows_is_reported_and_released():
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_scratch_bytes() == 0
    sizes = []
    for name in ("cornell", "soup1500"):
        tri, pos = mc.scene(name)
        nodes, woop, idx = _tree(name, "sah")
        _Dev(nodes, woop, idx, tri, pos, rf.deform(pos, 0.02)).refit(0.0)
        sizes.append(nt.bvh_motion_refit_scratch_bytes())
        assert sizes[-1] >= 12 * (nodes.nbytes // 64)
    assert sizes[1] > sizes[0]
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_scratch_bytes() == 0
