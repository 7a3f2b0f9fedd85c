"""The full-sweep SAH build's rule on the CPU: the numpy spec (tests/np_sah_sweep.py) builds the host SAH builder's tree
(nt.sah_build), node for node and triangle for triangle, compared by walking both trees in lockstep; the spec's own layout is the
canonical level order and a valid BVH over its rows; and ntr_sah_device_build checks its arguments before any device work."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

import np_sah_sweep as sw
import sah_sweep_scenes as ss

F = np.float32


def _spec_equals_host(tri, pos, mn, mx):
    r = sw.build(tri, pos, mn, mx)
    h = nt.sah_build(tri, pos, mn, mx)
    inner, leaves = sw.walk_equal(ss.buffers(r), ss.buffers(h))
    st = r["stats"]
    assert inner == st["numInnerNodes"] == h.nodes.nbytes // 64 and leaves == st["numLeaves"]
    assert r["woop"].nbytes == h.woop.nbytes and r["tri_index"].nbytes == h.tri_index.nbytes
    return r


@pytest.mark.parametrize("prefs", ss.LEAF_PREFS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_spec_equals_host_tree(name, prefs):
    tri, pos = ss.scene(name)
    r = _spec_equals_host(tri, pos, *prefs)
    st = r["stats"]
    if name == "all_dropped":
        assert st["numDropped"] == tri.shape[0] and st["numInnerNodes"] == 1 and st["numLeaves"] == 2
        assert r["woop"].nbytes == 32
    if name == "one_live":
        assert st["numDropped"] == tri.shape[0] - 1 and st["numInnerNodes"] == 1 and sw.check_layout(r) == 1
    if name == "dropped_mix":
        assert st["numDropped"] == int(sw.tri_terms(tri, pos)[3].sum()) > 60
        assert sw.check_layout(r) == tri.shape[0] - st["numDropped"]
    if name == "huge":            # the all-right chain: one inner node and one empty leaf per level down to the depth cap
        assert st["maxDepth"] == sw.MAX_DEPTH and st["numInnerNodes"] == sw.MAX_DEPTH and st["numLevels"] == sw.MAX_DEPTH + 1
        assert (r["nodes"][:, 14] == 0).all()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_soups_over_seeds(seed):
    rng = np.random.default_rng(seed)
    for n in (1, 2, 3, 7, 64, 1000):
        tri, pos, _ = scenes.random_soup(n, seed=int(rng.integers(1 << 30)), walls=False)
        for prefs in ss.LEAF_PREFS:
            _spec_equals_host(tri, pos, *prefs)


def test_soup_20000():
    tri, pos, _ = scenes.random_soup(20000, seed=77, walls=False)
    r = _spec_equals_host(tri, pos, 1, 1)
    assert sw.check_layout(r) == 20000


@pytest.mark.parametrize("name", ["cornell", "soup1000", "dropped_mix", "identical", "grid", "one_live", "all_dropped"])
def test_spec_layout_and_validity(name):
    tri, pos = ss.scene(name)
    cam = scenes.cornell_box()[2]
    for prefs in ((1, 1), (4, 8)):
        r = sw.build(tri, pos, *prefs)
        st = r["stats"]
        live = sw.check_layout(r)
        assert live == tri.shape[0] - st["numDropped"]
        assert r["nodes"].nbytes == 64 * st["numInnerNodes"]
        assert r["woop"].nbytes == 16 * (3 * live + st["numLeaves"]) and r["tri_index"].nbytes * 4 == r["woop"].nbytes
        # every live triangle in exactly one leaf
        links = r["nodes"][:, 12:14].reshape(-1)
        ids = [i for c in links[links < 0] for i in sw.leaf_ids(r["woop"], r["tri_index"], ~int(c))]
        assert sorted(ids) == np.flatnonzero(~sw.tri_terms(tri, pos)[3]).tolist()
        for rays in (scenes.primary_rays(cam, 48, 48)[0], scenes.random_rays(2048, 5, extent=float(np.abs(pos).max()) + 1.0)):
            got, _ = oracle.trace(r["nodes"], r["woop"], r["tri_index"], rays)
            ref = oracle.bruteforce_closest(r["woop"], r["tri_index"], rays)
            assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), (name, prefs)
            assert np.array_equal(got["id"] >= 0, ref["id"] >= 0)


def _call(L, res, num=4, tri=1, nv=12, pos=1, mn=1, mx=1, nodes=1, cn=None, woop=1, cw=None, idx=1, ci=None):
    capn, capw, capi = nt.lbvh_capacity(max(num, 1))
    return L.ntr_sah_device_build(num, tri, nv, pos, mn, mx, nodes, capn if cn is None else cn, woop, capw if cw is None else cw, idx,
                                  capi if ci is None else ci, C.byref(res) if res is not None else None, None)


def test_argument_errors_precede_device_work():
    L = nt.lib()
    capn, capw, capi = nt.lbvh_capacity(4)
    for kw in (dict(num=0), dict(num=-3), dict(num=1 << 28), dict(nv=0), dict(tri=None), dict(pos=None), dict(mn=0), dict(mn=3, mx=2),
               dict(nodes=None), dict(woop=None), dict(idx=None), dict(cn=capn - 1), dict(cw=capw - 1), dict(ci=capi - 1)):
        res = nt.SahDeviceResult()
        res.numNodes = res.numDropped = 77
        res.seconds = 1.0
        assert _call(L, res, **kw) == -1, kw
        assert bytes(res) == bytes(C.sizeof(res)), kw          # a failed call zeroes its result
    assert _call(L, None) == -1
    assert L.ntr_sah_device_scratch_bytes(None) == -1
    assert C.sizeof(nt.SahDeviceResult) == 80


def test_no_cpu_fallback_without_device():
    cnt = C.c_int(-1)
    rc = nt.lib().ntr_device_count(C.byref(cnt))
    if rc == 0 and cnt.value > 0:
        pytest.skip("a GPU is present")
    tri, pos = ss.scene("cornell")
    capn, capw, capi = nt.lbvh_capacity(tri.shape[0])
    bufs = [np.zeros(c, np.uint8) for c in (capn, capw, capi)]
    res = nt.SahDeviceResult()
    res.numNodes = 5
    rc = nt.lib().ntr_sah_device_build(tri.shape[0], tri.ctypes.data, pos.shape[0], pos.ctypes.data, 1, 1, bufs[0].ctypes.data, capn,
                                       bufs[1].ctypes.data, capw, bufs[2].ctypes.data, capi, C.byref(res), None)
    assert rc in (-2, -3), rc
    assert bytes(res) == bytes(C.sizeof(res))
    assert not any(b.any() for b in bufs)
    assert nt.sah_device_scratch_bytes() == 0
