"""ntr_pool_wide_refit and ntr_tlas_wide_refit on the device against the numpy rule (tests/np_wide_refit.py), byte for byte.  Pools are
built on the device as in test_refit_batch_gpu.py (PLOC BLASes by ntr_ploc_build_batch, LBVH BLASes of leafSize 8 and epsilon 0.001 by
ntr_lbvh_build at pool + offset) and widened by ntr_pool_widen; top-level trees are built by ntr_tlas_build and widened by ntr_tlas_widen;
the downloaded bytes are the rule's input.  Every buffer carries slack filled with 0xAB that must stay; every byte outside the listed
ranges, the binary pool's nodes and the whole triIndex must be what they were; Woop words that are NaN on both sides compare equal."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_scenes as isc
import np_bvh_refit as rf
import np_instanced as ni
import np_instanced_wide as niw
import np_wide_refit as wr
from gpu_util import up
from test_ploc_batch_gpu import _woop_equal
from test_refit_batch_gpu import _Pool, _soups
from test_tlas_refit_cpu import moved, placed

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 256
HOWS = (0.02, 0.3, "collapse")


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


def lanes_of(entries):
    """ntr_bvh_refit's thresholds over numTris / leaves of the selection, a leaf being a terminator row (include/ntrace_amd.h)"""
    mean = sum(e[5] for e in entries) / sum(max(e[3] // 16 - 3 * e[5], 1) for e in entries)
    return 1 if mean < 1.5 else (4 if mean < 3.0 else 8)


class _WidePool:
    """test_refit_batch_gpu._Pool and its wide pool, widened on the device.  entries[k]: NtrWideRefitEntry's fields of BLAS k."""

    def __init__(self, **meshes):
        self.pool = p = _Pool(**meshes)
        self.ranges = [e[0] for e in p.entries]
        cap = nt.pool_widen_capacity(self.ranges)
        self.d_wide = _filled(cap)
        self.wide_ranges, res = nt.pool_widen(self.ranges, p.bufs[0].data_ptr(), p.caps[0], self.d_wide.data_ptr(), cap)
        torch.cuda.synchronize()
        self.wide_bytes = int(res.nodesBytes)
        self.d_wide = self.d_wide[:self.wide_bytes + SLACK].clone()     # exactly the extent, then the border
        self.wide_built = self.d_wide.clone()
        self.wide_host = self.d_wide.cpu().numpy()
        assert (self.wide_host[self.wide_bytes:] == 0xAB).all()
        self.entries = [(w[0], w[1], e[0][2], e[0][3], e[1], e[2], e[3]) for w, e in zip(self.wide_ranges, p.entries)]

    def reset(self):
        self.pool.reset()
        self.d_wide.copy_(self.wide_built)

    def call(self, sel, d_pos, rewrite, d_boxes=None, **kw):
        p = self.pool
        return nt.pool_wide_refit([self.entries[k] for k in sel], self.d_wide.data_ptr(), self.wide_bytes, p.bufs[1].data_ptr(), p.caps[1],
                                  p.bufs[2].data_ptr(), p.tri.shape[0], p.d_tri.data_ptr(), p.pos.shape[0], d_pos.data_ptr(), rewrite,
                                  d_boxes.data_ptr() if d_boxes is not None else 0, **kw)

    def spec(self, sel, pos, rewrite, wide=None):
        p = self.pool
        return wr.refit_wide_pool([self.entries[k] for k in sel], (self.wide_host if wide is None else wide)[:self.wide_bytes],
                                  p.host[1][:p.caps[1]], p.host[2][:p.caps[2]].view(np.int32), p.tri, pos, rewrite)

    def download(self):
        torch.cuda.synchronize()
        return self.d_wide.cpu().numpy(), [b.cpu().numpy() for b in self.pool.bufs]

    def assert_equals(self, sel, spec, rewrite, boxes, what, skip=()):
        """The device's buffers against the spec's; skip: entries (malformed) whose own ranges are not compared"""
        p = self.pool
        wide, (nodes, woop, idx) = self.download()
        assert np.array_equal(nodes, p.host[0]) and np.array_equal(idx, p.host[2]), ("the binary nodes or triIndex changed", what)
        assert (wide[self.wide_bytes:] == 0xAB).all() and (woop[p.caps[1]:] == 0xAB).all(), ("slack written", what)
        keep_n, keep_w = np.ones(self.wide_bytes, bool), np.ones(p.caps[1], bool)
        for k in skip:
            no, nb, wo, wb = self.entries[k][:4]
            keep_n[no:no + nb] = False
            keep_w[wo:wo + wb] = False
        for k in sel:                                                    # entry by entry, so that a failure names the entry
            if k in skip:
                continue
            no, nb, wo, wb = self.entries[k][:4]
            assert np.array_equal(wide[no:no + nb], spec["nodes"][no:no + nb]), ("wide nodes differ", what, k, self.entries[k])
            assert _woop_equal(woop[wo:wo + wb], spec["woop"][wo:wo + wb]), ("triWoop differs", what, k)
        assert np.array_equal(wide[:self.wide_bytes][keep_n], spec["nodes"][keep_n]), ("wide bytes outside the listed ranges changed", what)
        w4, s4 = woop[:p.caps[1]].view(np.uint32), spec["woop"].view(np.uint32)
        same = (w4 == s4) | (np.isnan(w4.view(F)) & np.isnan(s4.view(F)))
        assert same[keep_w.reshape(-1, 4).all(axis=1)].all(), ("row bytes outside the listed ranges changed", what)
        if not rewrite:
            assert np.array_equal(woop, p.host[1]), ("rewriteRows = 0 wrote a row", what)
        if boxes is not None:
            ok = [j for j, k in enumerate(sel) if k not in skip]
            assert boxes[ok].tobytes() == spec["boxes"][ok].tobytes(), ("boxes differ", what)

    def check(self, sel=None, hows=HOWS, rewrites=(1, 0), what="", lanes=None, batch=True):
        """Refit the selection (default: all) to every deformation, blocking, with and without the rows, and compare"""
        p = self.pool
        sel = list(range(len(self.entries))) if sel is None else list(sel)
        res = None
        for how in hows:
            pos = rf.moved(p.pos, how)
            d_pos = up(pos)
            for rewrite in rewrites:
                self.reset()
                d_boxes = _filled(24 * len(sel))
                res = self.call(sel, d_pos, rewrite, d_boxes)
                hb = d_boxes.cpu().numpy()
                assert (hb[24 * len(sel):] == 0xAB).all()
                boxes = hb[:24 * len(sel)].view(F).reshape(-1, 6)
                spec = self.spec(sel, pos, rewrite)
                self.assert_equals(sel, spec, rewrite, boxes, (what, how, rewrite))
                assert (res.numEntries, res.firstBadEntry, res.errBits) == (len(sel), -1, 0) and res.seconds > 0
                assert dict(numNodes=res.numNodes, numLeafLinks=res.numLeafLinks, numRows=res.numRows) == spec["stats"], (what, how)
                assert res.lanesPerLeaf == lanes_of([self.entries[k] for k in sel]), (what, res.lanesPerLeaf)
                if lanes is not None:
                    assert res.lanesPerLeaf == lanes, (what, res.lanesPerLeaf)
                if rewrite and batch:                                    # the rows and the boxes ntr_bvh_refit_batch gives on a copy of the pool
                    woop = p.bufs[1].cpu().numpy()
                    copy = [b.clone() for b in p.built]
                    d_bb = torch.zeros(6 * len(sel), dtype=torch.float32, device="cuda:0")
                    nt.bvh_refit_batch(*p.args(copy, [p.entries[k] for k in sel], d_pos, d_bb))
                    assert _woop_equal(woop, copy[1].cpu().numpy()), ("rows differ from ntr_bvh_refit_batch's", what, how)
                    assert boxes.tobytes() == d_bb.cpu().numpy().tobytes(), ("boxes differ from ntr_bvh_refit_batch's", what, how)
        assert nt.trace_status() == 0
        return res


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------
def test_small_blases_root_counts_and_the_empty_leaf():
    """1..5 triangles: one wide node with 2 (one of them the empty leaf), 2, 3 and 4 slots, and two levels"""
    wp = _WidePool(ploc=_soups((1, 2, 3, 4, 5), 21))
    counts = [int(wp.wide_host[w[0]:w[0] + 128].view(np.int32)[28]) for w in wp.wide_ranges]
    assert counts[:4] == [2, 2, 3, 4] and [w[2] for w in wp.wide_ranges][:4] == [1, 1, 1, 1] and wp.wide_ranges[4][2] == 2
    wp.check(what="small", lanes=1)


def test_leaf_links_across_wave_and_workgroup_edges_and_a_larger_mesh():
    """64 / 65 and 256 / 257 triangles: leaf links either side of a wave's and a workgroup's edge in the one-lane climb; 1 000 triangles"""
    wp = _WidePool(ploc=_soups((64, 65, 256, 257, 1000), 22))
    wp.check(what="edges", hows=(0.3,), lanes=1)
    wp.check(sel=[4], what="one 1000-triangle mesh", rewrites=(1,))


def test_each_lanes_per_leaf_is_reached():
    wp = _WidePool(ploc=_soups((300, 1, 77), 23), lbvh=_soups((400, 9, 1000, 64), 24))
    ploc, lbvh = [0, 1, 2], [3, 4, 5, 6]
    wp.check(ploc, what="ploc only", hows=(0.3,), lanes=1)
    wp.check(lbvh, what="lbvh only", lanes=8)
    mixes = [m for m in ([3] + ploc, lbvh + ploc, [5] + ploc, [3, 4, 0], [5, 0], lbvh + [0], [6] + ploc, [4] + ploc)
             if lanes_of([wp.entries[k] for k in m]) == 4]
    assert mixes, "no selection of these BLASes has a mean leaf size for four lanes"
    wp.check(mixes[0], what="mix", hows=(0.3,), lanes=4)


def test_more_entries_than_a_workgroup_and_a_subset_in_scrambled_order():
    rng = np.random.default_rng(20261201)
    wp = _WidePool(ploc=_soups([int(x) for x in rng.integers(2, 6, 300)], 25))
    res = wp.check(what="300 entries", hows=(0.3,), rewrites=(1,))
    print("300 entries: %.1f us" % (res.seconds * 1e6))
    sel = [int(x) for x in rng.permutation(300)[:37]]
    wp.check(sel, what="subset", hows=(0.02,))


def test_unmoved_vertices_change_no_byte_and_the_asynchronous_form_gives_the_same_bytes():
    wp = _WidePool(ploc=_soups((40, 1, 300, 7, 2, 129), 26))
    sel = list(range(6))
    d_pos = up(wp.pool.pos)
    res = wp.call(sel, d_pos, 1)
    wide, (nodes, woop, idx) = wp.download()
    assert res.errBits == 0 and np.array_equal(wide, wp.wide_host) and _woop_equal(woop, wp.pool.host[1]) and np.array_equal(idx, wp.pool.host[2])
    pos = rf.moved(wp.pool.pos, 0.3)
    d_pos = up(pos)
    for rewrite in (1, 0):
        wp.reset()
        wp.call(sel, d_pos, rewrite)
        a = wp.download()
        wp.reset()
        d_boxes = _filled(24 * 6)
        assert wp.call(sel, d_pos, rewrite, d_boxes, blocking=False) is None
        b = wp.download()
        assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
        wp.assert_equals(sel, wp.spec(sel, pos, rewrite), rewrite, d_boxes.cpu().numpy()[:144].view(F).reshape(-1, 6), ("async", rewrite))


def test_a_malformed_entry_is_named_and_the_others_are_refitted():
    """Malformed data that the kernels must skip: a link that names no wide node is never followed"""
    wp = _WidePool(ploc=_soups((40, 300, 129, 1, 25), 27))
    wi = wp.wide_host[:wp.wide_bytes].view(np.int32).reshape(-1, 32)
    base = wp.entries[2][0] // 128
    n, k = (int(x) for x in np.argwhere(wi[base:base + wp.wide_ranges[2][2], 12:16] > 0)[3])
    wi[base + n, 12 + k] = 0x7FFFFF80
    wp.wide_built.copy_(torch.from_numpy(wp.wide_host))
    wp.reset()
    pos = rf.moved(wp.pool.pos, 0.3)
    d_pos = up(pos)
    sel = list(range(5))
    d_boxes = torch.zeros(6 * 5, dtype=torch.float32, device="cuda:0")
    with pytest.raises(nt.NtrError) as e:
        wp.call(sel, d_pos, 1, d_boxes)
    assert e.value.code == -4 and "entry 2" in str(e.value), str(e.value)
    res = e.value.result
    assert (res.numEntries, res.firstBadEntry, res.errBits) == (5, 2, 1)
    spec = wp.spec(sel, pos, 1)
    assert spec["first_bad_entry"] == 2 and spec["err_bits"] == 1
    wp.assert_equals(sel, spec, 1, d_boxes.cpu().numpy().reshape(-1, 6), "malformed", skip=(2,))
    wide = wp.download()[0]
    got = wide[:wp.wide_bytes].view(np.int32).reshape(-1, 32)
    assert np.array_equal(got[:, 12:16], wi[:, 12:16]) and np.array_equal(got[:, 28:], wi[:, 28:])      # rule 1 holds for the bad tree too
    # the asynchronous form skips the malformed part silently and gives the same bytes
    wp.reset()
    assert wp.call(sel, d_pos, 1, blocking=False) is None
    again = wp.download()[0]
    assert np.array_equal(again, wide)
    # two bad entries, one of them a node named twice: the lowest is named
    wi2 = wi.copy()
    b1 = wp.entries[1][0] // 128
    inner = np.argwhere(wi2[b1:b1 + wp.wide_ranges[1][2], 12:16] > 0)
    (n0, k0), (n1, k1) = (int(x) for x in inner[0]), (int(x) for x in inner[5])
    wi2[b1 + n1, 12 + k1] = wi2[b1 + n0, 12 + k0]
    wp.d_wide[:wp.wide_bytes] = up(wi2)
    with pytest.raises(nt.NtrError) as e:
        wp.call(sel, d_pos, 0)
    assert e.value.code == -4 and e.value.result.firstBadEntry == 1 and e.value.result.errBits == 1 and "entry 1" in str(e.value)
    assert nt.trace_status() == 0


# ---- the top level ------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _scene_pool():
    """The three BLASes of test_tlas_refit_cpu.pool() as a device pool over one shared index and vertex array, and its wide pool"""
    if "wp" not in _cache:
        _cache["wp"] = _WidePool(ploc=[isc.blas(nm)[:2] for nm in ("cornell", "soup1000", "one")])
    return _cache["wp"]


class _WideTlas:
    """Instances on the device, the top-level tree ntr_tlas_build makes of them over wp's binary pool and its widening by ntr_tlas_widen,
    in 0xAB-bordered buffers of exactly the extents.  built_*: the downloaded wide tree, the rule's input."""

    def __init__(self, wp, inst):
        self.wp, self.n = wp, inst.shape[0]
        p = wp.pool
        self.d_inst = up(inst)
        caps = nt.tlas_capacity(self.n)
        d_tlas, d_rec = _filled(caps[0]), _filled(caps[1])
        t = nt.tlas_build(self.n, self.d_inst.data_ptr(), wp.ranges, p.bufs[0].data_ptr(), p.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(), caps[1])
        self.root = t.rootLink
        cap = max(nt.bvh_widen_capacity(t.nodesBytes), 128) if self.n > 1 else 128
        d_wt, d_wrec = _filled(cap), _filled(64 * self.n)
        w = nt.tlas_widen(self.n, self.d_inst.data_ptr(), d_tlas.data_ptr(), t.nodesBytes, t.rootLink, wp.ranges, wp.wide_ranges, d_wt.data_ptr(), cap,
                          d_wrec.data_ptr(), 64 * self.n)
        torch.cuda.synchronize()
        self.nodes_bytes, self.rec_bytes, self.widened = int(w.nodesBytes), 64 * self.n, w
        self.d_wt, self.d_rec, self.d_scene = _filled(self.nodes_bytes), d_wrec, _filled(24)
        self.d_wt[:self.nodes_bytes] = d_wt[:self.nodes_bytes]
        torch.cuda.synchronize()
        self.built_nodes = self.d_wt.cpu().numpy()[:self.nodes_bytes].view(np.int32).reshape(-1, 32).copy()
        self.built_records = self.d_rec.cpu().numpy()[:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy()
        self.built_scene = np.concatenate([np.array(list(t.sceneMin), F), np.array(list(t.sceneMax), F)])

    def refit(self, blocking=True, stream=0):
        wp = self.wp
        return nt.tlas_wide_refit(self.n, self.d_inst.data_ptr(), wp.ranges, wp.wide_ranges, wp.d_wide.data_ptr(), wp.wide_bytes, self.d_wt.data_ptr(),
                                  self.nodes_bytes, self.root, self.d_rec.data_ptr(), self.rec_bytes, self.d_scene.data_ptr(), stream=stream,
                                  blocking=blocking)

    def download(self):
        torch.cuda.synchronize()
        raw = [b.cpu().numpy() for b in (self.d_wt, self.d_rec, self.d_scene)]
        for x, e in zip(raw, (self.nodes_bytes, self.rec_bytes, 24)):
            assert (x[e:] == 0xAB).all(), "bytes beyond the extents were written"
        return (raw[0][:self.nodes_bytes].view(np.int32).reshape(-1, 32).copy(), raw[1][:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy(),
                raw[2][:24].copy())

    def spec(self, wide_pool_nodes, inst):
        return wr.refit_wide_tlas(self.built_nodes, self.root, self.built_records, wide_pool_nodes, self.wp.ranges, self.wp.wide_ranges, inst)

    def assert_equals(self, want, res=None, what=""):
        nodes, records, sb = self.download()
        bad = np.flatnonzero((nodes != want["nodes"]).any(axis=1))
        assert bad.size == 0, ("wide nodes differ", what, int(bad[0]), nodes[bad[0]], want["nodes"][bad[0]])
        assert np.array_equal(records, want["records"]), ("records differ", what)
        assert sb.tobytes() == want["scene_box"].tobytes(), ("d_sceneBox differs", what)
        if res is not None:
            assert (res.numNodes, res.numLeaves, res.errBits) == (want["stats"]["numNodes"], want["stats"]["numLeaves"], want["err_bits"]), what
            got = np.concatenate([np.array(list(res.sceneMin), F), np.array(list(res.sceneMax), F)])
            assert got.tobytes() == want["scene_box"].tobytes(), ("sceneMin / sceneMax differ", what)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, nt.PLOC_TAIL + 1])
def test_tlas_wide_refit_equals_spec(n):
    wp = _scene_pool()
    wp.reset()
    inst = placed(n, 500 + n)
    s = _WideTlas(wp, inst)
    # the refit of a fresh widening with unchanged instances changes no byte
    before = [b.clone() for b in (s.d_wt, s.d_rec)]
    res = s.refit()
    torch.cuda.synchronize()
    assert torch.equal(before[0], s.d_wt) and torch.equal(before[1], s.d_rec), ("the refit of a fresh widening changed a byte", n)
    assert res.errBits == 0 and (res.numNodes, res.numLeaves) == (s.widened.numNodes, n) and res.seconds > 0
    assert s.download()[2].tobytes() == s.built_scene.tobytes(), n
    # moved transforms, every third instance on another BLAS
    new = moved(inst, 900 + n)
    s.d_inst.copy_(up(new))
    s.d_scene.fill_(0xAB)
    res = s.refit()
    want = s.spec(wp.wide_host, new)
    assert want["err_bits"] == 0
    s.assert_equals(want, res, (n, "moved"))
    print("N=%d: %.1f us" % (n, res.seconds * 1e6))
    # a pool refitted by ntr_pool_wide_refit first
    pos = rf.moved(wp.pool.pos, 0.05)
    sel = [0, 1, 2]
    wp.call(sel, up(pos), 1)
    wide_now = wp.download()[0]
    assert np.array_equal(wide_now[:wp.wide_bytes], wp.spec(sel, pos, 1)["nodes"])
    s.d_scene.fill_(0xAB)
    assert s.refit(blocking=False) is None
    s.assert_equals(s.spec(wide_now, new), None, (n, "refitted pool"))
    # a blas index out of range keeps its leaf box and is reported with bit 1
    bad = new.copy()
    bad["blas"][n // 2] = 3
    s.d_inst.copy_(up(bad))
    s.d_wt[:s.nodes_bytes] = up(s.built_nodes)
    s.d_rec[:s.rec_bytes] = up(s.built_records)
    s.d_scene.fill_(0xAB)
    with pytest.raises(nt.NtrError) as e:
        s.refit()
    want = s.spec(wide_now, bad)
    assert e.value.code == -1 and e.value.result.errBits == 1 and want["err_bits"] == 1
    nodes, records, sb = s.download()
    assert np.array_equal(nodes, want["nodes"]) and np.array_equal(records, want["records"]) and sb.tobytes() == bytes([0xAB]) * 24
    wp.reset()
    assert nt.trace_status() == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _trace(wp, s, rays, d_rays, stream=0):
    out = {}
    for any_hit in (False, True):
        d_res, d_ids = _filled(16 * rays.shape[0]), _filled(4 * rays.shape[0])
        nt.trace_instanced_wide(rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_wt.data_ptr(), s.nodes_bytes, s.root,
                                s.d_rec.data_ptr(), s.n, wp.d_wide.data_ptr(), wp.wide_bytes, wp.pool.bufs[1].data_ptr(), wp.pool.caps[1],
                                wp.pool.bufs[2].data_ptr(), stream=stream, timed=False)
        out[any_hit] = (d_res, d_ids)
    return out


def _assert_trace(wp, s, rays, pool_spec, tlas_spec, got, what):
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    p = wp.pool
    spool = dict(nodes=p.host[0][:p.caps[0]], woop=pool_spec["woop"], tri_index=p.host[2][:p.caps[2]].view(np.int32), ranges=wp.ranges)
    hits = 0
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst, _ = niw.trace(tlas_spec["nodes"], s.root, tlas_spec["records"], spool, pool_spec["nodes"], rays, any_hit)
        d_res, d_ids = got[any_hit]
        gid, gt, gu, gv = isc.result_words(d_res.cpu().numpy()[:16 * rays.shape[0]].view(nt.RESULT_DTYPE))
        ids = d_ids.cpu().numpy()[:4 * rays.shape[0]].view(np.int32)
        for name, g, e in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                           ("instance", ids, rinst)):
            assert np.array_equal(g, e), (what, name, any_hit)
        hits += int((rid >= 0).sum())
    assert hits > 0, what


def _frame(wp, s, inst0, step):
    """vertex positions (BLAS 0 deformed) and instances (moved) of frame `step`"""
    p = wp.pool
    pos = p.pos.copy()
    first, num = wp.entries[0][4], wp.entries[0][5]
    verts = np.unique(p.tri[first:first + num])
    pos[verts] = rf.moved(p.pos[verts], 0.02 * (step + 1))
    tf = inst0["objectToWorld"].copy()
    tf[:, 3] += np.linspace(-0.4, 0.4, inst0.shape[0]).astype(F) * F(step + 1)
    tf[:, 7] += F(0.2 * (step + 1))
    return pos, ni.instances(tf, inst0["blas"])


@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_refit_both_levels_and_trace_uncaptured_and_as_one_graph(name):
    sc = isc.scene(name)
    wp = _WidePool(ploc=[isc.blas(nm)[:2] for nm in sc["names"]])
    inst0 = ni.instances(sc["transforms"], sc["blas"])
    s = _WideTlas(wp, inst0)
    rays = isc.scene_rays(primary=(32, 16), random=256)
    d_rays = up(rays)
    sel = list(range(len(wp.entries)))
    pos, inst = _frame(wp, s, inst0, 0)
    d_pos, stream = up(pos), torch.cuda.Stream()
    s.d_inst.copy_(up(inst))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):                 # the warm-up: one uncaptured call of each, asynchronous on one stream
        wp.call(sel, d_pos, 1, stream=stream.cuda_stream, blocking=False)
        s.refit(blocking=False, stream=stream.cuda_stream)
        got = _trace(wp, s, rays, d_rays, stream.cuda_stream)
    pool_spec = wp.spec(sel, pos, 1)
    tlas_spec = s.spec(pool_spec["nodes"], inst)
    wp.assert_equals(sel, pool_spec, 1, None, (name, "uncaptured"))
    s.assert_equals(tlas_spec, None, (name, "uncaptured"))
    _assert_trace(wp, s, rays, pool_spec, tlas_spec, got, (name, "uncaptured"))
    held = (nt.pool_wide_refit_scratch_bytes(), nt.tlas_wide_refit_scratch_bytes())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        cs = torch.cuda.current_stream().cuda_stream
        wp.call(sel, d_pos, 1, stream=cs, blocking=False)
        s.refit(blocking=False, stream=cs)
        got = _trace(wp, s, rays, d_rays, cs)
    assert (nt.pool_wide_refit_scratch_bytes(), nt.tlas_wide_refit_scratch_bytes()) == held
    for step in (1, 2):                             # the buffers rewritten between replays; the wide trees carry on from the last frame
        wide_before = wp.download()[0]
        tl_before = s.download()
        pos, inst = _frame(wp, s, inst0, step)
        d_pos.copy_(up(pos))
        s.d_inst.copy_(up(inst))
        torch.cuda.synchronize()
        g.replay()
        pool_spec = wp.spec(sel, pos, 1, wide=wide_before)
        tlas_spec = wr.refit_wide_tlas(tl_before[0], s.root, tl_before[1], pool_spec["nodes"], wp.ranges, wp.wide_ranges, inst)
        _assert_trace(wp, s, rays, pool_spec, tlas_spec, got, (name, "replay", step))
        assert np.array_equal(wp.download()[0][:wp.wide_bytes], pool_spec["nodes"]) and np.array_equal(s.download()[0], tlas_spec["nodes"])
    del g


def test_a_captured_call_with_another_table_is_refused_and_the_scratch_does_not_grow():
    nt.lbvh_release_workspace()
    assert nt.pool_wide_refit_scratch_bytes() == 0 and nt.tlas_wide_refit_scratch_bytes() == 0
    wp = _WidePool(ploc=_soups((40, 1, 300), 28))
    s = _WideTlas(wp, placed(5, 77, blas=[0, 1, 2, 0, 2]))
    d_pos = up(rf.moved(wp.pool.pos, 0.02))
    stream = torch.cuda.Stream()
    held = None
    with torch.cuda.stream(stream):
        for rep in range(20):
            wp.call([0, 1, 2], d_pos, 1, stream=stream.cuda_stream, blocking=False)
            s.refit(blocking=False, stream=stream.cuda_stream)
            now = (nt.pool_wide_refit_scratch_bytes(), nt.tlas_wide_refit_scratch_bytes())
            assert held is None or now == held
            held = now
    torch.cuda.synchronize()
    nodes = sum(w[2] for w in wp.wide_ranges)
    assert held[0] >= 8 * nodes + 36 * 3 + 16384 and held[1] >= 8 * s.nodes_bytes // 128 + 16 * 3 + 16384
    errs = []

    def capture(fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            s.d_scene.zero_()        # so that the graph is not empty
            try:
                fn(torch.cuda.current_stream().cuda_stream)
            except nt.NtrError as e:
                errs.append((e.code, str(e)))
        torch.cuda.synchronize()

    capture(lambda cs: wp.call([2, 0], d_pos, 1, stream=cs, blocking=False))
    capture(lambda cs: wp.call([0, 1, 2], d_pos, 1, stream=cs, blocking=True))
    other = _WideTlas(wp, placed(9, 78, blas=[0, 1, 2] * 3))
    capture(lambda cs: other.refit(blocking=False, stream=cs))
    nt.lbvh_release_workspace()
    assert nt.pool_wide_refit_scratch_bytes() == 0 and nt.tlas_wide_refit_scratch_bytes() == 0
    capture(lambda cs: wp.call([0, 1, 2], d_pos, 1, stream=cs, blocking=False))
    capture(lambda cs: s.refit(blocking=False, stream=cs))
    assert [c for c, _ in errs] == [-1] * 5 and all("uncaptured call" in m for (_, m), k in zip(errs, range(5)) if k != 1), errs
    wp.reset()
    assert wp.call([0, 1, 2], d_pos, 1).errBits == 0 and s.refit().errBits == 0     # the library works afterwards
    nt.lbvh_release_workspace()
