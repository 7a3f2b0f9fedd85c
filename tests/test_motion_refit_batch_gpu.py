"""ntr_bvh_motion_refit_batch on the device.  Pools are built on the device as tests/test_refit_batch_gpu.py builds them (its _Pool: PLOC
BLASes by one ntr_ploc_build_batch, LBVH BLASes of leafSize 8 and epsilon 0.001 by ntr_lbvh_build behind them); the three key-1 pools
are prefilled with 0xCD and every buffer carries 256 bytes of 0xAB slack.  After every call the five buffers are compared twice: with
the numpy spec (tests/np_motion_refit_batch.py) and with the loop this call replaces -- one ntr_bvh_motion_refit per entry at pool +
offset on a copy of the pool as built -- byte for byte (Woop words that are NaN on both sides compare equal).  The slack, triIndex and
every byte outside the listed ranges must be what they were.  Key 0 is the mesh as built, key 1 np_bvh_refit.moved(pos, how).  The shapes
are the smallest where the segmented kernels can go wrong: entry edges of the slot space and of the ROW space on wave and workgroup edges,
one-triangle BLASes, every lanesPerLeaf, subsets in scrambled order, more entries than a workgroup, a malformed entry, one stream, a graph."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_deform_cases as dc
import instanced_scenes as isc
import np_bvh_ploc as pl
import np_bvh_refit as rf
import np_instanced_deform as nd
import np_motion_refit_batch as mb
from gpu_util import up
from test_instanced_deform_gpu import _Dev, _filled, _records
from test_motion_refit_batch_cpu import _shared
from test_ploc_batch_gpu import _seeded_mesh, _woop_equal
from test_refit_batch_gpu import HOWS, SLACK, _Pool, _soups, lanes_of

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xCD
NAMES = ("nodes0", "nodes1", "woop", "vrows0", "vrows1")


def _fresh(c):
    t = torch.full((c + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")
    t[:c] = FILL
    return t


def _same(name, a, b):
    return _woop_equal(a, b) if name == "woop" else a.tobytes() == b.tobytes()


class _MPool:
    """test_refit_batch_gpu._Pool and the three key-1 pools beside it.  five(): nodes0, nodes1, triWoop, vertRows0, vertRows1."""

    def __init__(self, **kw):
        self.p = _Pool(**kw)
        self.caps, self.entries, self.pos = self.p.caps, self.p.entries, self.p.pos
        self.ext = (self.caps[0], self.caps[0], self.caps[1], self.caps[1], self.caps[1])
        self.key1 = [_fresh(c) for c in (self.caps[0], self.caps[1], self.caps[1])]

    def five(self):
        return [self.p.bufs[0], self.key1[0], self.p.bufs[1], self.key1[1], self.key1[2]]

    def reset(self):
        self.p.reset()
        for t, c in zip(self.key1, (self.caps[0], self.caps[1], self.caps[1])):
            t[:c] = FILL
            t[c:] = 0xAB

    def call(self, entries, d_p0, d_p1, d_boxes=None, **kw):
        f, p = self.five(), self.p
        return nt.bvh_motion_refit_batch(entries, f[0].data_ptr(), self.caps[0], f[1].data_ptr(), f[2].data_ptr(), self.caps[1],
                                         p.bufs[2].data_ptr(), f[3].data_ptr(), f[4].data_ptr(), p.tri.shape[0], p.d_tri.data_ptr(),
                                         p.pos.shape[0], d_p0.data_ptr(), d_p1.data_ptr(), d_boxes.data_ptr() if d_boxes is not None else 0, **kw)

    def spec(self, entries, p0, p1):
        h, (cn, cw, ci) = self.p.host, self.caps
        return mb.motion_refit(entries, h[0][:cn], np.full(cn, FILL, np.uint8), h[1][:cw], np.full(cw, FILL, np.uint8), np.full(cw, FILL, np.uint8),
                               h[2][:ci].view(np.int32), self.p.tri, p0, p1)

    def loop(self, entries, d_p0, d_p1):
        """The path this call replaces: one ntr_bvh_motion_refit per entry at pool + offset, asynchronous, on a copy of the pool as
        built with fresh key-1 pools.  -> (the five buffers with their slack, boxes)"""
        p = self.p
        b = [x.clone() for x in p.built]
        k1 = [_fresh(self.caps[0]), _fresh(self.caps[1]), _fresh(self.caps[1])]
        d_box = torch.zeros(6 * len(entries), dtype=torch.float32, device="cuda:0")
        for k, ((no, nb, wo, wb), first, n, eps) in enumerate(entries):
            nt.bvh_motion_refit(b[0].data_ptr() + no, nb, k1[0].data_ptr() + no, b[1].data_ptr() + wo, wb, b[2].data_ptr() + wo // 4, wb // 4,
                                k1[1].data_ptr() + wo, k1[2].data_ptr() + wo, n, p.d_tri.data_ptr() + 12 * first, p.pos.shape[0], d_p0.data_ptr(),
                                d_p1.data_ptr(), eps, d_box.data_ptr() + 24 * k, 0, False)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (b[0], k1[0], b[1], k1[1], k1[2])], d_box.cpu().numpy().reshape(-1, 6)

    def download(self):
        torch.cuda.synchronize()
        assert np.array_equal(self.p.bufs[2].cpu().numpy(), self.p.host[2]), "triIndex or its slack changed"
        return [x.cpu().numpy() for x in self.five()]

    def assert_pool(self, entries, p0, p1, d_p0, d_p1, got_boxes, what, spec=None, loop=True):
        """The five device buffers against the spec over the pool as built, and against the loop of ntr_bvh_motion_refit calls."""
        spec = spec if spec is not None else self.spec(entries, p0, p1)
        got = self.download()
        for name, g, c in zip(NAMES, got, self.ext):
            assert (g[c:] == 0xAB).all(), ("slack written", name, what)
            for k, ((no, nb, wo, wb), _, _, _) in enumerate(entries):   # entry by entry, so that a failure names the entry
                o, n = (no, nb) if name.startswith("nodes") else (wo, wb)
                assert _same(name, g[o:o + n], spec[name][o:o + n]), (name + " differs", what, k, entries[k])
            assert _same(name, g[:c], spec[name]), (name + ": bytes outside the listed ranges changed", what)
        if got_boxes is not None:
            assert got_boxes.tobytes() == spec["boxes"].tobytes(), ("boxes differ", what)
        if loop:
            want, lb = self.loop(entries, d_p0, d_p1)
            for name, g, w in zip(NAMES, got, want):
                assert _same(name, g, w), (name + " differs from the loop of ntr_bvh_motion_refit", what)
            if got_boxes is not None:
                assert got_boxes.tobytes() == lb.tobytes(), ("boxes differ from the loop's", what)
        return spec

    def check(self, entries=None, hows=HOWS, what="", lanes=None, key0=None):
        """Refit `entries` (default: all) to (key 0, key 1 = moved(pos, how)) for every deformation, blocking, and compare; -> the last
        result.  key0: a deformation of key 0 too (default: the mesh as built)."""
        entries = self.entries if entries is None else entries
        p0 = self.pos if key0 is None else rf.moved(self.pos, key0)
        d_p0 = up(p0)
        res = None
        for how in hows:
            p1 = rf.moved(self.pos, how)
            d_p1 = up(p1)
            self.reset()
            d_boxes = torch.full((24 * len(entries) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")
            res = self.call(entries, d_p0, d_p1, d_boxes)
            hb = d_boxes.cpu().numpy()
            assert (hb[24 * len(entries):] == 0xAB).all()
            spec = self.assert_pool(entries, p0, p1, d_p0, d_p1, hb[:24 * len(entries)].view(F).reshape(-1, 6), (what, how))
            assert (res.numEntries, res.firstBadEntry, res.errBits) == (len(entries), -1, 0) and res.seconds > 0
            assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == spec["stats"], (what, how)
            assert res.lanesPerLeaf == lanes_of(entries), (what, res.lanesPerLeaf)
            if lanes is not None:
                assert res.lanesPerLeaf == lanes, (what, res.lanesPerLeaf)
        return res


# ---- 1. one entry: ntr_bvh_motion_refit's own bytes, box and counts ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 129, 1025])
def test_one_entry_equals_bvh_motion_refit(n):
    for kind in ("ploc", "lbvh"):
        pool = _MPool(**{kind: _soups((n,), 2)})
        res = pool.check(what=(kind, n))              # bytes and box against the one call the loop makes
        (no, nb, wo, wb), first, nt_, eps = pool.entries[0]
        b = [x.clone() for x in pool.p.built]
        k1 = [_fresh(nb), _fresh(wb), _fresh(wb)]
        d_p1 = up(rf.moved(pool.pos, HOWS[-1]))
        one = nt.bvh_motion_refit(b[0].data_ptr() + no, nb, k1[0].data_ptr(), b[1].data_ptr() + wo, wb, b[2].data_ptr() + wo // 4, wb // 4,
                                  k1[1].data_ptr(), k1[2].data_ptr(), nt_, pool.p.d_tri.data_ptr(), pool.pos.shape[0], pool.p.d_pos.data_ptr(),
                                  d_p1.data_ptr(), eps)
        assert (res.numNodes, res.numLeaves, res.numRows) == (one.numNodes, one.numLeaves, one.numRows), (kind, n)


# ---- 2. slot edges against wave and workgroup edges ----------------------------------------------------------------------------------
def test_slot_edges_on_wave_and_workgroup_edges_one_lane_per_leaf():
    """A workgroup of 256 threads covers 256 node slots in the prepare launch and 128 in the one-lane climbs.  PLOC sizes
    (65, 64, 1, 129, 2, 1, 1, 257, 70) have 64, 63, 1, 128, 1, 1, 1, 256, 69 slots: running sums 64, 127, 128, 256, 257, ..."""
    sizes = (65, 64, 1, 129, 2, 1, 1, 257, 70)
    pool = _MPool(ploc=_soups(sizes, 3))
    sums = np.cumsum([e[0][1] // 64 for e in pool.entries]).tolist()
    assert sums[:5] == [64, 127, 128, 256, 257]
    pool.check(what=sizes, lanes=1)


# ---- 3. row edges: the index space only this call segments -----------------------------------------------------------------------------
def test_row_edges_on_wave_and_workgroup_edges():
    """The prepare launch zeroes one vertex row per thread and finds the row's entry in the running ROW sums.  A PLOC BLAS of n triangles
    has 4 n rows (5 for n = 1) and max(n - 1, 1) slots: sizes (16, 48, 1, 70, 1) have row sums 64, 256, 261, ... -- a wave's edge, a
    workgroup's edge, and a one-triangle BLAS right behind it -- while the slot sums 15, 62, 63, ... fall on neither."""
    sizes = (16, 48, 1, 70, 1)
    pool = _MPool(ploc=_soups(sizes, 13))
    rows = np.cumsum([e[0][3] // 16 for e in pool.entries]).tolist()
    slots = np.cumsum([e[0][1] // 64 for e in pool.entries]).tolist()
    assert rows[:3] == [64, 256, 261] and not set(slots) & {64, 128, 256}, (rows, slots)
    pool.check(what=("row edges", sizes), lanes=1)
    # the same edges with the entries in another order than the pool's: the row space follows the ENTRIES, not the addresses
    sel = [pool.entries[k] for k in (1, 0, 4, 3, 2)]
    rows = np.cumsum([e[0][3] // 16 for e in sel]).tolist()
    assert rows[:3] == [192, 256, 261]
    pool.check(sel, hows=(0.3,), what=("row edges, reordered", sizes), lanes=1)


# ---- 4. entry edges at 16 and 32 slots for the 8-lane kernel --------------------------------------------------------------------------
def test_entry_edges_at_16_and_32_slots_for_the_eight_lane_kernel():
    """test_refit_batch_gpu.py's construction: 256 threads of the 8-lane climb cover 16 node slots; a selection of small LBVH trees is
    ordered so that its running slot sums hit exactly 16 and exactly 32, and two larger trees keep the mean leaf size at 8 lanes'."""
    sizes = tuple(range(20, 120, 3)) + (700, 900)
    pool = _MPool(lbvh=_soups(sizes, 4))
    small, big = pool.entries[:-2], pool.entries[-2:]
    slots = [e[0][1] // 64 for e in small]

    def take(total, used):
        """indices (one tree or two) outside `used` whose slots sum to `total`; the largest trees that do"""
        best = None
        for i in range(len(slots)):
            if i in used:
                continue
            if slots[i] == total:
                return [i]
            for j in range(i + 1, len(slots)):
                if j not in used and slots[i] + slots[j] == total and (best is None or min(slots[i], slots[j]) > min(slots[k] for k in best)):
                    best = [i, j]
        return best

    first = take(16, set())
    assert first, ("no selection of these LBVH trees reaches 16 slots", slots)
    second = take(16, set(first))
    assert second, ("no second selection of these LBVH trees reaches 16 slots", slots)
    sel = [small[k] for k in first + second] + big + [small[k] for k in range(len(small)) if k not in first + second][:5]
    sums = np.cumsum([e[0][1] // 64 for e in sel]).tolist()
    assert 16 in sums and 32 in sums
    pool.check(sel, what=("lbvh edges", sums), lanes=8)


# ---- 5. one-triangle BLASes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(1, 1, 5, 1), (1,) * 9])
def test_one_triangle_blases_first_last_and_adjacent(sizes):
    pool = _MPool(ploc=_soups(sizes, 5))
    built = pool.p.host[0].view(np.int32)
    d_p0 = up(pool.pos)
    for how in HOWS:
        p1 = rf.moved(pool.pos, how)
        pool.reset()
        d_p1 = up(p1)
        d_boxes = torch.zeros(6 * len(sizes), dtype=torch.float32, device="cuda:0")
        pool.call(pool.entries, d_p0, d_p1, d_boxes)
        boxes = d_boxes.cpu().numpy().reshape(-1, 6)
        pool.assert_pool(pool.entries, pool.pos, p1, d_p0, d_p1, boxes, (sizes, how))
        got = pool.download()
        for k, ((no, nb, wo, wb), first, n, _) in enumerate(pool.entries):
            if n != 1:
                continue
            v = np.concatenate([pool.pos[pool.p.tri[first]], p1[pool.p.tri[first]]])
            assert np.array_equal(boxes[k], np.concatenate([v.min(axis=0), v.max(axis=0)])), (sizes, how, k)
            w = pool.p.host[1].view(np.uint32).reshape(-1, 4)
            for nodes in (got[0].view(np.int32), got[1].view(np.int32)):
                root = nodes[no // 4:no // 4 + 16]
                empty = 0 if w[wo // 16 + ~root[12], 0] == rf.TERM else 1
                assert np.array_equal(root[rf.BOX_WORDS[empty]], built[no // 4:no // 4 + 16][rf.BOX_WORDS[empty]]), "the empty child's box changed"


# ---- 6. every lanesPerLeaf --------------------------------------------------------------------------------------------------------------
def test_each_lanes_per_leaf_is_reached():
    pool = _MPool(ploc=_soups((300, 1, 77, 513), 6), lbvh=_soups((400, 1, 9, 1000, 64), 7))
    ploc, lbvh = pool.entries[:4], pool.entries[4:]
    pool.check(ploc, what="ploc only", lanes=1)
    pool.check(lbvh, what="lbvh only", lanes=8)
    mixes = [m for m in ([lbvh[0]] + ploc, lbvh + ploc, [lbvh[3]] + ploc, lbvh[:2] + ploc[:1], [lbvh[3], ploc[0]], lbvh + ploc[:1])
             if lanes_of(m) == 4]
    assert mixes, [lanes_of(m) for m in ([lbvh[0]] + ploc, lbvh + ploc, [lbvh[3]] + ploc)]
    pool.check(mixes[0], what="mix", lanes=4)
    # key 0 moved as well: the in-place half (nodes0, the Woop rows, vertRows0) leaves the bytes the builders wrote
    for sel, lanes in ((ploc, 1), (lbvh, 8), (mixes[0], 4)):
        pool.check(sel, hows=(0.3,), what=("key 0 moved", lanes), lanes=lanes, key0=0.05)


# ---- 7. a subset in scrambled order -----------------------------------------------------------------------------------------------------
def test_a_subset_in_scrambled_order_leaves_the_other_blases_alone():
    pool = _MPool(ploc=_soups((40, 1, 300, 7, 2, 129, 33), 8))
    sel = [pool.entries[k] for k in (5, 0, 3)]
    pool.check(sel, what="subset")       # boxes in entry order, every byte outside the three ranges as it was
    got = pool.download()
    for k in (1, 2, 4, 6):
        no, nb, wo, wb = pool.entries[k][0]
        assert np.array_equal(got[0][no:no + nb], pool.p.host[0][no:no + nb]) and np.array_equal(got[2][wo:wo + wb], pool.p.host[1][wo:wo + wb])
        assert (got[1][no:no + nb] == FILL).all() and (got[3][wo:wo + wb] == FILL).all() and (got[4][wo:wo + wb] == FILL).all()


# ---- 8. per-entry epsilon ---------------------------------------------------------------------------------------------------------------
def test_two_blases_of_one_triangle_range_with_two_epsilons():
    from test_ploc_batch_gpu import _soup
    tri, pos = _soup(500, 9)
    box = pl.scene_box(pos)
    pool = _MPool(concat=(tri, pos, [(0, 500, box[0], box[1]), (0, 500, box[0], box[1])]))
    a, b = pool.entries
    entries = [a, (b[0], b[1], b[2], 0.001)]
    pool.check(entries, what="epsilons")
    got = pool.download()
    (n0, nb, w0, wb), (n1, _, w1, _) = a[0], b[0]
    for key, nodes in (("nodes0", got[0]), ("nodes1", got[1])):
        x, y = nodes[n0:n0 + nb].view(F).reshape(-1, 16), nodes[n1:n1 + nb].view(F).reshape(-1, 16)
        assert np.array_equal(x.view(np.int32)[:, 12:], y.view(np.int32)[:, 12:])
        leaf = nodes[n0:n0 + nb].view(np.int32).reshape(-1, 16)[:, 12:14] < 0
        for k in (0, 1):
            lo, hi = rf.BOX_WORDS[k][rf.LO], rf.BOX_WORDS[k][rf.HI]
            m = leaf[:, k]
            assert np.array_equal(y[m][:, lo], (x[m][:, lo] - F(0.001)).astype(F)), key
            assert np.array_equal(y[m][:, hi], (x[m][:, hi] + F(0.001)).astype(F)), key
        assert not np.array_equal(x[:, :12], y[:, :12])
    for g in got[2:]:
        assert np.array_equal(g[w0:w0 + wb], g[w1:w1 + wb])


# ---- 9. more entries than one workgroup, in both index spaces ---------------------------------------------------------------------------
def test_more_entries_than_one_workgroup():
    rng = np.random.default_rng(20261121)
    sizes = [int(x) for x in rng.integers(1, 13, 1100)]
    n = sum(sizes)
    pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
    tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
    meshes, first = [], 0
    for s in sizes:
        box = pl.scene_box(pos[tri[first:first + s]])
        meshes.append((first, s, box[0], box[1]))
        first += s
    pool = _MPool(concat=(tri, pos, meshes))
    res = pool.check(hows=(0.3,), what="1100 entries", lanes=1)
    print("1100 entries, %d triangles: %.1f us" % (n, res.seconds * 1e6))


# ---- 10. seeded batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", range(3))
def test_seeded_batches_equal_spec(group):
    """12 batches (four per case) of 2 to 12 meshes of the four kinds of test_ploc_batch_gpu._seeded_mesh, each of 1 to 3000 triangles
    (log-uniform), every second mesh an LBVH BLAS, key 1 moved by a seeded amplitude; the pool stays under 20 k triangles."""
    rng = np.random.default_rng(20261122 + group)
    for i in range(4 * group, 4 * group + 4):
        parts, total = [], 0
        for _ in range(int(rng.integers(2, 13))):
            n = max(1, int(round(3000.0 ** rng.random())))
            n = min(n, max(1, 19000 - total))
            total += n
            parts.append(_seeded_mesh(rng, int(rng.integers(4)), n))
        pool = _MPool(ploc=parts[0::2], lbvh=parts[1::2])
        amp = float(F(rng.choice([0.0, 0.01, 0.05, 0.3, 1.0])))
        pool.check(hows=(amp,), what=(i, [e[2] for e in pool.entries], amp))


# ---- 11. a malformed entry --------------------------------------------------------------------------------------------------------------
def test_a_malformed_entry_is_named_and_the_others_are_refitted():
    pool = _MPool(ploc=_soups((40, 300, 129, 1, 25), 10))
    p = pool.p
    no = pool.entries[2][0][0]
    word = no // 4 + 16 * 5 + 12                  # child 0 of node 5 of entry 2
    p.host[0].view(np.int32)[word] = 0x7FFFFFC0   # a link that names no slot: rejected, never followed
    p.built[0].copy_(torch.from_numpy(p.host[0]))
    pool.reset()
    p1 = rf.moved(pool.pos, 0.3)
    d_p0, d_p1 = up(pool.pos), up(p1)
    d_boxes = torch.zeros(6 * 5, dtype=torch.float32, device="cuda:0")
    with pytest.raises(nt.NtrError) as e:
        pool.call(pool.entries, d_p0, d_p1, d_boxes)
    assert e.value.code == -4 and "entry 2" in str(e.value), str(e.value)
    res = e.value.result
    assert (res.numEntries, res.firstBadEntry, res.errBits) == (5, 2, 1)
    good = [pool.entries[k] for k in (0, 1, 3, 4)]
    spec = pool.spec(good, pool.pos, p1)
    got = pool.download()
    boxes = d_boxes.cpu().numpy().reshape(-1, 6)
    for name, g, c in zip(NAMES, got, pool.ext):
        assert (g[c:] == 0xAB).all(), name
        for (n0, nb, w0, wb), _, _, _ in good:
            o, n = (n0, nb) if name.startswith("nodes") else (w0, wb)
            assert _same(name, g[o:o + n], spec[name][o:o + n]), name
    assert boxes[[0, 1, 3, 4]].tobytes() == spec["boxes"].tobytes()
    assert got[0].view(np.int32)[word] == 0x7FFFFFC0 and got[1].view(np.int32)[word] == 0x7FFFFFC0
    # the loop's asynchronous result on the same malformed pool, byte for byte: the bad entry's partly written slices too
    want, _ = pool.loop(pool.entries, d_p0, d_p1)
    for name, g, w in zip(NAMES, got, want):
        assert _same(name, g, w), (name, "differs from the loop on the malformed pool")
    # the asynchronous form skips the malformed part silently and gives the same bytes
    pool.reset()
    assert pool.call(pool.entries, d_p0, d_p1, None, blocking=False) is None
    again = pool.download()
    for name, g, w in zip(NAMES, again, got):
        assert _same(name, g, w), (name, "the asynchronous form differs")
    # two bad entries: the lowest is named
    h = p.host[0].copy()
    h.view(np.int32)[pool.entries[1][0][0] // 4 + 13] = 0x7FFFFFC0
    pool.reset()
    p.bufs[0].copy_(torch.from_numpy(h))
    with pytest.raises(nt.NtrError) as e:
        pool.call(pool.entries, d_p0, d_p1, None)
    assert e.value.code == -4 and e.value.result.firstBadEntry == 1 and "entry 1" in str(e.value)
    assert e.value.result.errBits == 1


# ---- 12. one stream and a graph ---------------------------------------------------------------------------------------------------------
def test_batch_refit_top_level_refit_and_trace_on_one_stream_and_as_one_graph():
    """The asynchronous batch refit, ntr_tlas_deform_refit and ntr_trace_instanced_deform on one stream with no host wait in between,
    then the same three captured as one graph that is replayed after both vertex arrays were overwritten in place."""
    s = dc.named("three")
    d = _Dev(s)                                   # its constructor posed the pool by the loop: put the pool back as built
    base = isc.pool_of(s.names)
    tri, pos0, pos1, entries = _shared(s)
    d_tri, d_p0, d_p1 = up(tri), up(pos0), up(pos1)
    rays = dc.rays_of("tail")
    n = rays.shape[0]
    assert n == 4097
    d_rays, d_res, d_ids = up(rays), _filled(16 * n), _filled(4 * n)
    times = np.linspace(0.0, 1.0, n).astype(F)
    d_times = up(times)
    motion = nt.InstanceMotion(d.d_keys.data_ptr(), d.keys_bytes, d_times.data_ptr(), 0.0)
    st = torch.cuda.Stream()

    def unpose():
        d.d_nodes.copy_(up(base["nodes"]))
        d.d_woop.copy_(up(base["woop"]))
        for t, c in ((d.d_nodes1, d.nb), (d.d_v0, d.wb), (d.d_v1, d.wb)):
            t[:c] = FILL
        d.reset()
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        torch.cuda.synchronize()

    def batch(stream, ent=entries, blocking=False):
        return nt.bvh_motion_refit_batch(ent, d.d_nodes.data_ptr(), d.nb, d.d_nodes1.data_ptr(), d.d_woop.data_ptr(), d.wb, d.d_idx.data_ptr(),
                                         d.d_v0.data_ptr(), d.d_v1.data_ptr(), tri.shape[0], d_tri.data_ptr(), pos0.shape[0], d_p0.data_ptr(),
                                         d_p1.data_ptr(), 0, stream=stream, blocking=blocking)

    def frame(stream):
        assert batch(stream) is None
        d.refit(blocking=False, stream=stream)
        nt.trace_instanced_deform(*d.args(n, False, d_rays, d_res, d_ids), vis=None, motion=motion, deform=d.deform, stream=stream, timed=False)

    def check(scene, what):
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        for name, buf in (("nodes", d.d_nodes), ("woop", d.d_woop), ("nodes1", d.d_nodes1), ("vrows0", d.d_v0), ("vrows1", d.d_v1)):
            g = buf.cpu().numpy()
            c = scene.pool[name].size
            assert _same(name, g[:c], scene.pool[name]), ("the pool's " + name + " differs from the spec's", what)
            if name not in ("nodes", "woop"):
                assert (g[c:] == FILL).all(), (name, what)    # _Dev fills its key-1 buffers and their slack with one byte
        # the top-level tree is the device's own build (the refit keeps its topology): the rule runs over those bytes
        want = nd.deform_refit(d.built_nodes, d.root, d.built_records, scene.pool["nodes"], scene.pool["nodes1"], scene.ranges,
                               scene.pool["deforming"], scene.inst0, scene.inst1)
        d.assert_equals(want, None, what)
        rid, rt, ru, rv, rinst, _ = nd.trace(want["nodes"], d.root, want["records"], want["motion_keys"], scene.pool, rays, False, times=times)
        res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
        assert (res[16 * n:] == 0xAB).all() and (ids[4 * n:] == 0xAB).all()
        assert res[:16 * n].tobytes() == _records(rays, rid, rt, ru, rv) and ids[:4 * n].tobytes() == rinst.astype(np.int32).tobytes(), what
        assert (rid >= 0).any()
        return res[:16 * n].tobytes()

    unpose()
    with torch.cuda.stream(st):
        frame(st.cuda_stream)                       # uncaptured first: it uploads the tables and reserves the scratch
    seen = [check(s, "one stream")]
    held = nt.bvh_motion_refit_batch_scratch_bytes()
    assert held > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        frame(torch.cuda.current_stream().cuda_stream)
    assert nt.bvh_motion_refit_batch_scratch_bytes() == held
    # both vertex arrays overwritten in place with another deformation of BLAS 1, then the replay
    mesh = s.meshes[1]
    s2 = dc.DeformScene(s.names, s.inst0, s.inst1, {1: (rf.moved(mesh[1], 0.05), rf.moved(mesh[1], 0.15))})
    _, q0, q1, entries2 = _shared(s2)
    assert entries2 == entries
    unpose()
    d_p0.copy_(up(q0))
    d_p1.copy_(up(q1))
    torch.cuda.synchronize()
    g.replay()
    seen.append(check(s2, "graph replay over new keys"))
    assert seen[0] != seen[1]
    del g
    # a captured call with a result, with other entries than the held table, or after the workspace was released: refused
    errs = []

    def capture(ent, blocking=False):
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=st):
            d_ids.fill_(0xAB)    # so that the graph is not empty
            try:
                batch(torch.cuda.current_stream().cuda_stream, ent, blocking)
            except nt.NtrError as e:
                errs.append((e.code, str(e)))
        torch.cuda.synchronize()

    capture(entries, blocking=True)
    capture([(entries[0][0], entries[0][1], entries[0][2], 0.5)])
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_batch_scratch_bytes() == 0
    capture(entries)
    assert [c for c, _ in errs] == [-1, -1, -1], errs
    assert "a captured call cannot read a result back (pass result = NULL)" in errs[0][1]
    for _, text in errs[1:]:
        assert "the device must hold this entry table already -- make one uncaptured call with the same entries first (and none with other " \
               "entries, and no ntr_lbvh_release_workspace, between it and the capture)" in text, text
    # and the library works afterwards
    unpose()
    res = batch(0, blocking=True)
    assert res.firstBadEntry == -1 and res.numEntries == 1
    d.refit()
    nt.trace_instanced_deform(*d.args(n, False, d_rays, d_res, d_ids), vis=None, motion=motion, deform=d.deform, timed=False)
    assert check(s2, "after the refused captures") == seen[1]


# ---- 13. determinism and scratch --------------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_batch_scratch_bytes() == 0
    pool = _MPool(ploc=_soups((1500, 1, 700), 11), lbvh=_soups((2100, 30), 12))
    d_p0, d_p1 = up(pool.pos), up(rf.moved(pool.pos, 0.3))
    pool.call(pool.entries, d_p0, d_p1)
    a = pool.download()
    held = nt.bvh_motion_refit_batch_scratch_bytes()
    slots = sum(e[0][1] // 64 for e in pool.entries)
    assert held >= 16384 + 12 * slots + (32 + 8 + 48) * len(pool.entries)
    pool.reset()
    pool.call(pool.entries, d_p0, d_p1)            # the same entries: the held table is not uploaded again -- seen here by the bytes only
    b = pool.download()
    assert nt.bvh_motion_refit_batch_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_batch_scratch_bytes() == 0
    pool.reset()
    pool.call(pool.entries, d_p0, d_p1, blocking=False)
    c = pool.download()
    for other in (b, c):
        for x, y in zip(a, other):
            assert x.tobytes() == y.tobytes()
    print("scratch: %d B for %d slots and %d entries" % (held, slots, len(pool.entries)))
    nt.lbvh_release_workspace()
    assert nt.bvh_motion_refit_batch_scratch_bytes() == 0
