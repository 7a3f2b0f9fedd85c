"""ntr_pool_widen_batch on the device.  Every case widens its pool into 0xAB-filled buffers through BOTH calls -- the batched pass and
ntr_pool_widen, the host loop of ntr_bvh_widen -- and demands that the batch's bytes, wideRanges and result fields (all but seconds,
which is > 0) equal np_instanced_wide.widen_pool's and the loop's, and that nothing beyond the extent is written.  The pools are the
smallest at which the pass can still go wrong: very different heights, entry boundaries inside workgroups and waves, ranges in any
order and aliased, unreached slots, more entries than a workgroup has threads, an entry across the scan's chunk boundary, and a
malformed tree between two sound ones."""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_wide as bw
import np_instanced as ni
import np_instanced_wide as nw
import np_ploc_batch as pb
import wide_trees as wt
from gpu_util import up
from test_bvh_wide_gpu import _device_build
from test_instanced_gpu import _Scene, _filled
from test_instanced_wide_gpu import _Wide, _assert_equals_spec

pytestmark = pytest.mark.gpu

NAMES = ["one", "soup2", "soup64", "cornell", "nested90", "soup1000"]
_cache = {}


def _fields(r):
    return (r.nodesBytes, r.numNodes, list(r.counts), r.numLeafLinks, r.height, r.stackBound)


def _call(name, ranges, d_nodes, pool_bytes):
    """One of the two entry points, raw, into a 0xAB-filled buffer of the capacity plus a guard -> dict(rc, msg, raw, ranges, res, buf)."""
    n = len(ranges)
    arr = (nt.BlasRange * n)(*[nt.BlasRange(*[int(x) for x in r]) for r in ranges])
    out = (nt.WideBlasRange * n)()
    res = nt.BvhWideResult()
    cap = nt.pool_widen_capacity(ranges)
    buf = _filled(cap + 256)
    rc = getattr(nt.lib(), name)(n, C.cast(arr, C.c_void_p), d_nodes.data_ptr(), pool_bytes, buf.data_ptr(), cap, C.cast(out, C.c_void_p),
                                 C.byref(res), None)
    msg = nt.lib().ntr_last_error() if rc else b""
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert 0 <= res.nodesBytes <= cap and (raw[res.nodesBytes:] == 0xAB).all(), "%s wrote beyond its extent" % name
    return dict(rc=rc, msg=msg, raw=raw[:res.nodesBytes].copy(), ranges=[(w.nodesOffset, w.nodesBytes, w.numNodes, w.stackBound) for w in out],
                res=res, buf=buf)


def _both(pool_nodes, ranges, spec=True, what=""):
    """Widen through the loop and through the batch; the batch equals the loop, and with spec=True both equal widen_pool."""
    nodes = np.ascontiguousarray(pool_nodes).view(np.uint8).reshape(-1)
    d_nodes = up(nodes)
    loop = _call("ntr_pool_widen", ranges, d_nodes, nodes.size)
    batch = _call("ntr_pool_widen_batch", ranges, d_nodes, nodes.size)
    assert batch["rc"] == loop["rc"], (what, batch["rc"], loop["rc"], batch["msg"], loop["msg"])
    assert batch["ranges"] == loop["ranges"], (what, batch["ranges"], loop["ranges"])
    assert _fields(batch["res"]) == _fields(loop["res"]), (what, _fields(batch["res"]), _fields(loop["res"]))
    assert batch["res"].seconds > 0 and loop["res"].seconds > 0
    if batch["raw"].tobytes() != loop["raw"].tobytes():
        a, b = batch["raw"].view(np.int32).reshape(-1, 32), loop["raw"].view(np.int32).reshape(-1, 32)
        bad = np.flatnonzero((a != b).any(axis=1))
        raise AssertionError("%s: %d wide nodes differ from the loop's, first %d: %r != %r" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]]))
    if spec:
        ref = nw.widen_pool(dict(nodes=nodes, ranges=ranges))
        st = ref["stats"]
        assert batch["rc"] == 0, batch["msg"]
        assert batch["ranges"] == ref["ranges"], what
        assert _fields(batch["res"]) == (st["nodesBytes"], st["numNodes"], st["counts"], st["numLeafLinks"], st["height"], st["stackBound"]), what
        assert batch["raw"].tobytes() == ref["nodes"].tobytes(), what
        batch["spec"] = ref
    batch["loop"] = loop
    batch["d_nodes"] = d_nodes
    return batch


def _six(gap):
    if ("six", gap) not in _cache:
        _cache[("six", gap)] = isc.pool_of(NAMES, gap_nodes=gap) if gap else isc.pool_of(NAMES)
    return _cache[("six", gap)]


# ---- 1, 2, 3: heights, order, aliases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [0, 3])
def test_six_blases_of_very_different_heights(gap):
    pool = _six(gap)
    b = _both(pool["nodes"], pool["ranges"], what="six, gap %d" % gap)
    assert b["ranges"][4][3] == 89 and b["res"].stackBound == 89 and b["ranges"][0][:3] == (0, 128, 1)


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_placement_is_by_k_not_by_pool_offset(order):
    pool = _six(3)
    ranges = list(pool["ranges"])
    if order == "reversed":
        ranges.reverse()
    else:
        np.random.default_rng(2024).shuffle(ranges)
        assert ranges != pool["ranges"] and ranges != pool["ranges"][::-1]
    b = _both(pool["nodes"], ranges, what=order)
    offs = [r[0] for r in b["ranges"]]
    assert offs == list(np.cumsum([0] + [r[1] for r in b["ranges"]][:-1]))


def test_aliased_ranges_give_identical_blases_at_three_offsets():
    pool = _six(0)
    r0, r1 = pool["ranges"][2], pool["ranges"][5]
    b = _both(pool["nodes"], [r0, r1, r0, r0], what="aliased")
    (o0, e0, _, _), _, (o2, e2, _, _), (o3, e3, _, _) = b["ranges"]
    assert e0 == e2 == e3 and len({o0, o2, o3}) == 3
    assert b["raw"][o0:o0 + e0].tobytes() == b["raw"][o2:o2 + e2].tobytes() == b["raw"][o3:o3 + e3].tobytes()


# ---- 4: unreached all-zero slots --------------------------------------------------------------------------------------------------------
def test_a_spread_tree_between_two_blases():
    pool = ni.make_pool([wt.tree("soup64"), wt.tree("spread"), wt.tree("soup3")])
    b = _both(pool["nodes"], pool["ranges"], what="spread")
    assert b["ranges"][1][1:] == b["ranges"][0][1:]          # the spread tree is soup64's tree: the unreached slots are dropped


# ---- 5: more entries than a workgroup has threads ---------------------------------------------------------------------------------------
def test_three_hundred_small_blases():
    names = ["soup2", "soup3", "one"]
    pool = ni.make_pool([wt.tree(names[k % 3]) for k in range(300)])
    b = _both(pool["nodes"], pool["ranges"], what="300")
    single = [bw.widen(wt.tree(nm)[0])["stats"] for nm in names]
    for k, r in enumerate(b["ranges"]):
        assert r[3] == single[k % 3]["stackBound"] and r[2] == single[k % 3]["numNodes"], (k, r)
    assert b["res"].numNodes == 100 * sum(s["numNodes"] for s in single)


# ---- 6: an entry across the scan's chunk boundary -----------------------------------------------------------------------------------------
def test_a_large_blas_between_two_small_ones():
    tri, pos = scenes.random_soup(66000, seed=66, walls=False)[:2]
    nodes, woop, idx = _device_build("ploc", tri, pos)
    assert nodes.shape[0] > 65536 + 256
    pool = ni.make_pool([wt.tree("soup64"), (nodes, woop, idx), wt.tree("soup64")])
    b = _both(pool["nodes"], pool["ranges"], what="66000")
    assert b["ranges"][0][1:] == b["ranges"][2][1:] and b["ranges"][1][2] > 20000


# ---- 7: a malformed tree in the middle ------------------------------------------------------------------------------------------------
def _malformed(kind):
    a, mid, c = wt.tree("soup64")[0], wt.tree("soup64")[0].copy(), wt.tree("soup3")[0]
    n = mid.shape[0]
    inner = np.argwhere(mid[:, 12:14] > 0)
    leaf = np.argwhere(mid[:, 12:14] < 0)
    s, k = (int(x) for x in inner[-1])
    if kind == "next":            # beyond its own slots, inside the next BLAS's range (soup3's tree has two slots)
        assert c.shape[0] == 2
        mid[s, 12 + k] = 64 * (n + 1)
    elif kind == "outside":       # beyond the pool
        mid[s, 12 + k] = 64 * (a.shape[0] + n + c.shape[0] + 5)
    elif kind == "twice":         # a slot named by two links
        ls, lk = (int(x) for x in leaf[0])
        mid[ls, 12 + lk] = mid[s, 12 + k]
    else:                         # a two-node cycle: the child names its parent (not the root: offset 0 is nobody's child)
        ps, pk = next((int(p), int(q)) for p, q in inner if p > 0)
        child = mid[ps, 12 + pk] >> 6
        mid[child, 12] = 64 * ps
    return ni.make_pool([(a, *wt.tree("soup64")[1:]), (mid, *wt.tree("soup64")[1:]), (c, *wt.tree("soup3")[1:])])


@pytest.mark.parametrize("kind", ["next", "outside", "twice", "cycle"])
def test_a_malformed_blas_between_two_sound_ones(kind):
    pool = _malformed(kind)
    b = _both(pool["nodes"], pool["ranges"], spec=False, what=kind)   # the call has ended; bytes, ranges and result are the loop's
    if kind in ("next", "outside"):
        assert b["rc"] == -4 and b"BLAS 1" in b["msg"] and b"1 child links" in b["msg"], b["msg"]
    print("%s: rc %d (the loop: %d) %s" % (kind, b["rc"], b["loop"]["rc"], b["msg"].decode()))
    for k in (0, 2):              # the neighbours are their fresh single widenings
        o, n = pool["ranges"][k][:2]
        single = bw.widen(pool["nodes"][o:o + n])
        wo, wn, num, bound = b["ranges"][k]
        assert b["raw"][wo:wo + wn].tobytes() == single["nodes"].tobytes() and (num, bound) == (single["stats"]["numNodes"], single["stats"]["stackBound"])
    assert b["ranges"][1][1] >= 128 and b["ranges"][2][0] == b["ranges"][1][0] + b["ranges"][1][1]


# ---- 8: downstream ----------------------------------------------------------------------------------------------------------------------
class _BatchWide(_Wide):
    """test_instanced_wide_gpu's _Wide with the pool widened by the batch."""

    def __init__(self, s):
        self.s = s
        pool = s.pool
        cap = nt.pool_widen_capacity(pool["ranges"])
        self.d_wpool = _filled(cap + 128)
        self.wide_ranges, self.pool_res = nt.pool_widen_batch(pool["ranges"], s.d_nodes.data_ptr(), pool["nodes"].size, self.d_wpool.data_ptr(), cap)
        self.wpool = nw.widen_pool(pool)
        raw = self.d_wpool.cpu().numpy()
        ext = self.pool_res.nodesBytes
        assert ext == self.wpool["stats"]["nodesBytes"] and (raw[ext:] == 0xAB).all() and raw[:ext].tobytes() == self.wpool["nodes"].tobytes()
        assert self.wide_ranges == self.wpool["ranges"]
        self.wpool_bytes = ext
        self.widen_tlas()


def test_trace_and_wide_refit_over_a_pool_widened_by_the_batch():
    sc = isc.scene("three")
    pool = isc.pool_of(sc["names"])
    w = _BatchWide(_Scene(pool, ni.instances(sc["transforms"], sc["blas"])))
    rays = isc.scene_rays((64, 32), 2048)
    out = _assert_equals_spec(w, rays, "three over the batch's pool")
    assert (np.frombuffer(out[False][1], np.int32) >= 0).sum() > 200
    # ntr_pool_wide_refit with unmoved vertices changes no byte of the wide pool
    tri, pos, meshes = pb.concat([isc.blas(nm)[:2] for nm in sc["names"]])
    entries = [(wr[0], wr[1], r[2], r[3], m[0], m[1], 0.0) for wr, r, m in zip(w.wide_ranges, pool["ranges"], meshes)]
    d_tri, d_pos = up(np.ascontiguousarray(tri, np.int32)), up(np.ascontiguousarray(pos, np.float32))
    before = w.d_wpool.cpu().numpy().copy()
    res = nt.pool_wide_refit(entries, w.d_wpool.data_ptr(), w.wpool_bytes, w.s.d_woop.data_ptr(), pool["woop"].size, w.s.d_idx.data_ptr(),
                             tri.shape[0], d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), rewrite_rows=False)
    torch.cuda.synchronize()
    assert res.errBits == 0 and res.numNodes == w.pool_res.numNodes and res.numLeafLinks == w.pool_res.numLeafLinks
    assert np.array_equal(w.d_wpool.cpu().numpy(), before)


# ---- 9, 10: scratch, determinism, capture -------------------------------------------------------------------------------------------------
def test_scratch_is_its_own_pool_and_two_calls_give_the_same_bytes():
    nt.lbvh_release_workspace()
    assert nt.pool_widen_batch_scratch_bytes() == 0 and nt.bvh_widen_scratch_bytes() == 0
    pool = _six(3)
    nodes = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1)
    d_nodes = up(nodes)
    a = _call("ntr_pool_widen_batch", pool["ranges"], d_nodes, nodes.size)
    held = nt.pool_widen_batch_scratch_bytes()
    assert a["rc"] == 0 and held > 0 and nt.bvh_widen_scratch_bytes() == 0      # ntr_bvh_widen's pool is what it was before the call
    b = _call("ntr_pool_widen_batch", pool["ranges"], d_nodes, nodes.size)
    assert b["raw"].tobytes() == a["raw"].tobytes() and b["ranges"] == a["ranges"] and _fields(b["res"]) == _fields(a["res"])
    assert nt.pool_widen_batch_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.pool_widen_batch_scratch_bytes() == 0
    c = _call("ntr_pool_widen_batch", pool["ranges"], d_nodes, nodes.size)
    assert c["raw"].tobytes() == a["raw"].tobytes()
    nt.lbvh_release_workspace()


def test_a_capturing_stream_is_refused_and_the_capture_stays_valid():
    pool = _six(0)
    nodes = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1)
    d_nodes = up(nodes)
    cap = nt.pool_widen_capacity(pool["ranges"])
    d_out, d_mark = _filled(cap), _filled(64)
    stream = torch.cuda.Stream()                         # a fresh stream, a single linear branch
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=stream):
        d_mark.fill_(0x11)                               # so that the graph is not empty
        try:
            nt.pool_widen_batch(pool["ranges"], d_nodes.data_ptr(), nodes.size, d_out.data_ptr(), cap, stream=torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            errs.append((e.code, "captured" in str(e)))
    assert errs == [(-1, True)]
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xAB).all()           # refused before any device work
    g.replay()
    torch.cuda.synchronize()
    assert (d_mark.cpu().numpy() == 0x11).all() and (d_out.cpu().numpy() == 0xAB).all()
    ranges, res = nt.pool_widen_batch(pool["ranges"], d_nodes.data_ptr(), nodes.size, d_out.data_ptr(), cap)
    assert res.nodesBytes == sum(r[1] for r in ranges) and res.seconds > 0
