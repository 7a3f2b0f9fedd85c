"""ntr_bvh_refit_batch on the device.  Pools are built on the device -- PLOC BLASes by ntr_ploc_build_batch (one triangle per leaf,
epsilon 0), LBVH BLASes (leafSize 8, epsilon 0.001) by ntr_lbvh_build straight into pool + offset beside them -- and the downloaded bytes
are the spec's input.  After every call the pool is compared twice: with the numpy spec (tests/np_refit_batch.py: np_bvh_refit per
entry) and with a loop of ntr_bvh_refit calls at pool + offset on a copy of the pool, byte for byte (Woop words that are NaN on both
sides compare equal).  Pool buffers carry slack filled with 0xAB; the slack, every byte outside the listed ranges and the whole triIndex
must be what they were.  The shapes are the smallest where the segmented kernels can go wrong: entry edges on wave and workgroup edges,
one-triangle BLASes, every lanesPerLeaf, subsets in scrambled order, more entries than a workgroup, a malformed entry, graphs."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_scenes as isc
import np_bvh_ploc as pl
import np_bvh_refit as rf
import np_instanced as ni
import np_ploc_batch as pb
import np_refit_batch as rb
from gpu_util import up
from test_ploc_batch_gpu import _seeded_mesh, _soup, _woop_equal

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 256
HOWS = (0.02, 0.3, "collapse")
LBVH_EPS = 0.001


def _align(x, a):
    return (x + a - 1) // a * a


def lanes_of(entries):
    """ntr_bvh_refit's thresholds over the selection's mean leaf size (include/ntrace_amd.h): a tree has one leaf more than node slots."""
    leaves = sum(e[0][1] // 64 + 1 for e in entries)
    rows = sum(e[0][3] // 16 for e in entries)
    mean = (rows - leaves) / (3.0 * leaves)
    return 1 if mean < 1.5 else (4 if mean < 3.0 else 8)


class _Pool:
    """A pool on the device: `ploc` meshes built by one ntr_ploc_build_batch, then `lbvh` meshes each built by ntr_lbvh_build into its own
    region behind them.  entries[k] = (range, firstTri, numTris, epsilon) of BLAS k; the buffers have SLACK bytes of 0xAB at the end."""

    def __init__(self, ploc=(), lbvh=(), concat=None):
        self.tri, self.pos, meshes = concat if concat is not None else pb.concat(list(ploc) + list(lbvh))
        num_ploc = len(meshes) if concat is not None else len(ploc)
        self.tri, self.pos = np.ascontiguousarray(self.tri, np.int32), np.ascontiguousarray(self.pos, F)
        self.d_tri, self.d_pos = up(self.tri), up(self.pos)
        pm, lm = meshes[:num_ploc], meshes[num_ploc:]
        caps = nt.ploc_batch_capacity(pm) if pm else (0, 0, 0, [])
        ext_n, ext_w = caps[0], caps[1]
        regions = []
        for m in lm:
            cn, cw, _ = nt.lbvh_capacity(m[1])
            regions.append((ext_n, ext_w))
            ext_n, ext_w = ext_n + _align(cn, 64), ext_w + _align(cw, 16)
        self.caps = (ext_n, ext_w, ext_w // 4)
        self.bufs = [torch.full((c + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in self.caps]
        ranges = []
        if pm:
            _, ranges, _ = nt.ploc_build_batch(pm, self.tri.shape[0], self.d_tri.data_ptr(), self.pos.shape[0], self.d_pos.data_ptr(),
                                               self.bufs[0].data_ptr(), caps[0], self.bufs[1].data_ptr(), caps[1], self.bufs[2].data_ptr(), caps[2])
        self.entries = [(tuple(r), m[0], m[1], 0.0) for r, m in zip(ranges, pm)]
        for m, (no, wo) in zip(lm, regions):
            cn, cw, ci = nt.lbvh_capacity(m[1])
            r = nt.lbvh_build(m[1], self.d_tri.data_ptr() + 12 * m[0], self.pos.shape[0], self.d_pos.data_ptr(), m[2], m[3], 8, LBVH_EPS,
                              self.bufs[0].data_ptr() + no, cn, self.bufs[1].data_ptr() + wo, cw, self.bufs[2].data_ptr() + wo // 4, ci)
            self.entries.append(((no, r.nodesBytes, wo, r.triWoopBytes), m[0], m[1], LBVH_EPS))
        torch.cuda.synchronize()
        self.built = [b.clone() for b in self.bufs]                     # the pool as built, on the device
        self.host = [b.cpu().numpy() for b in self.bufs]                # ... and on the host: the spec's input
        for h, c in zip(self.host, self.caps):
            assert (h[c:] == 0xAB).all()

    def args(self, bufs, entries, d_pos, d_boxes):
        return (entries, bufs[0].data_ptr(), self.caps[0], bufs[1].data_ptr(), self.caps[1], bufs[2].data_ptr(), self.tri.shape[0],
                self.d_tri.data_ptr(), self.pos.shape[0], d_pos.data_ptr(), d_boxes.data_ptr() if d_boxes is not None else 0)

    def reset(self):
        for b, src in zip(self.bufs, self.built):
            b.copy_(src)

    def spec(self, entries, p):
        return rb.refit(entries, self.host[0][:self.caps[0]], self.host[1][:self.caps[1]], self.host[2][:self.caps[2]].view(np.int32), self.tri, p)

    def loop(self, entries, d_pos):
        """The parent's path: one ntr_bvh_refit per entry at pool + offset on a copy of the pool as built.  -> (nodes, woop, boxes)"""
        bufs = [b.clone() for b in self.built]
        d_box = torch.zeros(6 * len(entries), dtype=torch.float32, device="cuda:0")
        for k, ((no, nb, wo, wb), first, n, eps) in enumerate(entries):
            nt.bvh_refit(bufs[0].data_ptr() + no, nb, bufs[1].data_ptr() + wo, wb, bufs[2].data_ptr() + wo // 4, wb // 4, n,
                         self.d_tri.data_ptr() + 12 * first, self.pos.shape[0], d_pos.data_ptr(), eps, d_box.data_ptr() + 24 * k, 0, False)
        torch.cuda.synchronize()
        return bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), d_box.cpu().numpy().reshape(-1, 6)

    def download(self):
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in self.bufs]

    def assert_pool(self, entries, p, d_pos, got_boxes, what, spec=None, loop=True):
        """The device pool against the spec over the pool as built, and against the loop of ntr_bvh_refit calls."""
        spec = spec if spec is not None else self.spec(entries, p)
        nodes, woop, idx = self.download()
        cn, cw, _ = self.caps
        assert np.array_equal(idx, self.host[2]), ("triIndex or its slack changed", what)
        assert (nodes[cn:] == 0xAB).all() and (woop[cw:] == 0xAB).all(), ("slack written", what)
        for k, ((no, nb, wo, wb), _, _, _) in enumerate(entries):       # entry by entry, so that a failure names the entry
            assert np.array_equal(nodes[no:no + nb], spec["nodes"][no:no + nb]), ("nodes differ", what, k, entries[k])
            assert _woop_equal(woop[wo:wo + wb], spec["woop"][wo:wo + wb]), ("triWoop differs", what, k, entries[k])
        assert np.array_equal(nodes[:cn], spec["nodes"]), ("node bytes outside the listed ranges changed", what)
        assert _woop_equal(woop[:cw], spec["woop"]), ("row bytes outside the listed ranges changed", what)
        if got_boxes is not None:
            assert got_boxes.tobytes() == spec["boxes"].tobytes(), ("boxes differ", what)
        if loop:
            ln, lw, lb = self.loop(entries, d_pos)
            assert np.array_equal(nodes, ln) and _woop_equal(woop, lw), ("differs from the loop of ntr_bvh_refit", what)
            if got_boxes is not None:
                assert got_boxes.tobytes() == lb.tobytes(), ("boxes differ from the loop's", what)
        return spec

    def check(self, entries=None, hows=HOWS, what="", lanes=None):
        """Refit `entries` (default: all) to every deformation, blocking, and compare; -> the last result."""
        entries = self.entries if entries is None else entries
        res = None
        for how in hows:
            p = rf.moved(self.pos, how)
            d_pos = up(p)
            self.reset()
            d_boxes = torch.full((24 * len(entries) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")
            res = nt.bvh_refit_batch(*self.args(self.bufs, entries, d_pos, d_boxes))
            hb = d_boxes.cpu().numpy()
            assert (hb[24 * len(entries):] == 0xAB).all()
            spec = self.assert_pool(entries, p, d_pos, hb[:24 * len(entries)].view(F).reshape(-1, 6), (what, how))
            assert (res.numEntries, res.firstBadEntry, res.errBits) == (len(entries), -1, 0) and res.seconds > 0
            assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == spec["stats"], (what, how)
            assert res.lanesPerLeaf == lanes_of(entries), (what, res.lanesPerLeaf)
            if lanes is not None:
                assert res.lanesPerLeaf == lanes, (what, res.lanesPerLeaf)
        return res


def _soups(sizes, seed):
    return [_soup(n, 1000 * seed + 7 * k + n) for k, n in enumerate(sizes)]


# ---- 1. one entry: ntr_bvh_refit's own bytes and counts --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 129, 1025])
def test_one_entry_equals_bvh_refit(n):
    for kind in ("ploc", "lbvh"):
        pool = _Pool(**{kind: _soups((n,), 2)})
        res = pool.check(what=(kind, n))
        (no, nb, wo, wb), first, nt_, eps = pool.entries[0]
        bufs = [b.clone() for b in pool.built]
        d_pos = up(rf.moved(pool.pos, HOWS[-1]))
        one = nt.bvh_refit(bufs[0].data_ptr() + no, nb, bufs[1].data_ptr() + wo, wb, bufs[2].data_ptr() + wo // 4, wb // 4, nt_,
                           pool.d_tri.data_ptr(), pool.pos.shape[0], d_pos.data_ptr(), eps)
        assert (res.numNodes, res.numLeaves, res.numRows) == (one.numNodes, one.numLeaves, one.numRows), (kind, n)


# ---- 2. entry edges against wave and workgroup edges -----------------------------------------------------------------------------------
def test_entry_edges_on_wave_and_workgroup_edges_one_lane_per_leaf():
    """A workgroup of 256 threads covers 256 node slots in the topology launch and 128 in the one-lane climb.  PLOC sizes
    (65, 64, 1, 129, 2, 1, 1, 257, 70) have 64, 63, 1, 128, 1, 1, 1, 256, 69 slots: running sums 64, 127, 128, 256, 257, 258, 259, 515."""
    sizes = (65, 64, 1, 129, 2, 1, 1, 257, 70)
    pool = _Pool(ploc=_soups(sizes, 3))
    sums = np.cumsum([e[0][1] // 64 for e in pool.entries]).tolist()
    assert sums[:5] == [64, 127, 128, 256, 257]
    pool.check(what=sizes, lanes=1)


def test_entry_edges_at_16_and_32_slots_for_the_eight_lane_kernel():
    """256 threads of the 8-lane climb cover 32 child slots, that is 16 node slots.  How many slots an LBVH tree has is the builder's to
    say, so a pool of small LBVH BLASes is built first and the selection is then ordered (entries may come in any order) so that its
    running slot sums hit exactly 16 and exactly 32; two larger trees behind them keep the mean leaf size at the 8-lane kernel's."""
    sizes = tuple(range(20, 120, 3)) + (700, 900)
    pool = _Pool(lbvh=_soups(sizes, 4))
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


# ---- 3. one-triangle BLASes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(1, 1, 5, 1), (1,) * 9])
def test_one_triangle_blases_first_last_and_adjacent(sizes):
    pool = _Pool(ploc=_soups(sizes, 5))
    built = pool.host[0].view(np.int32)
    for how in HOWS:
        p = rf.moved(pool.pos, how)
        pool.reset()
        d_pos = up(p)
        d_boxes = torch.zeros(6 * len(sizes), dtype=torch.float32, device="cuda:0")
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, d_boxes))
        boxes = d_boxes.cpu().numpy().reshape(-1, 6)
        pool.assert_pool(pool.entries, p, d_pos, boxes, (sizes, how))
        nodes = pool.download()[0].view(np.int32)
        for k, ((no, nb, wo, wb), first, n, _) in enumerate(pool.entries):
            if n != 1:
                continue
            v = p[pool.tri[first]]
            assert np.array_equal(boxes[k], np.concatenate([v.min(axis=0), v.max(axis=0)])), (sizes, how, k)
            root, w = nodes[no // 4:no // 4 + 16], pool.host[1].view(np.uint32).reshape(-1, 4)
            empty = 0 if w[wo // 16 + ~root[12], 0] == rf.TERM else 1
            assert np.array_equal(root[rf.BOX_WORDS[empty]], built[no // 4:no // 4 + 16][rf.BOX_WORDS[empty]]), "the empty child's box changed"


# ---- 4. every lanesPerLeaf ----------------------------------------------------------------------------------------------------------------
def test_each_lanes_per_leaf_is_reached():
    pool = _Pool(ploc=_soups((300, 1, 77, 513), 6), lbvh=_soups((400, 1, 9, 1000, 64), 7))
    ploc, lbvh = pool.entries[:4], pool.entries[4:]
    pool.check(ploc, what="ploc only", lanes=1)
    pool.check(lbvh, what="lbvh only", lanes=8)
    mixes = [m for m in ([lbvh[0]] + ploc, lbvh + ploc, [lbvh[3]] + ploc, lbvh[:2] + ploc[:1], [lbvh[3], ploc[0]], lbvh + ploc[:1])
             if lanes_of(m) == 4]
    assert mixes, [lanes_of(m) for m in ([lbvh[0]] + ploc, lbvh + ploc, [lbvh[3]] + ploc)]
    pool.check(mixes[0], what="mix", lanes=4)


# ---- 5. a subset in scrambled order --------------------------------------------------------------------------------------------------------
def test_a_subset_in_scrambled_order_leaves_the_other_blases_alone():
    pool = _Pool(ploc=_soups((40, 1, 300, 7, 2, 129, 33), 8))
    sel = [pool.entries[k] for k in (5, 0, 3)]
    pool.check(sel, what="subset")       # boxes in entry order, every byte outside the three ranges as built
    nodes, woop, _ = pool.download()
    for k in (1, 2, 4, 6):
        no, nb, wo, wb = pool.entries[k][0]
        assert np.array_equal(nodes[no:no + nb], pool.host[0][no:no + nb]) and np.array_equal(woop[wo:wo + wb], pool.host[1][wo:wo + wb])


# ---- 6. per-entry epsilon ------------------------------------------------------------------------------------------------------------------
def test_two_blases_of_one_triangle_range_with_two_epsilons():
    tri, pos = _soup(500, 9)
    box = pl.scene_box(pos)
    pool = _Pool(concat=(tri, pos, [(0, 500, box[0], box[1]), (0, 500, box[0], box[1])]))
    a, b = pool.entries
    entries = [a, (b[0], b[1], b[2], 0.001)]
    pool.check(entries, what="epsilons")
    nodes, woop, _ = pool.download()
    (n0, nb, w0, wb), (n1, _, w1, _) = a[0], b[0]
    x, y = nodes[n0:n0 + nb].view(F).reshape(-1, 16), nodes[n1:n1 + nb].view(F).reshape(-1, 16)
    assert np.array_equal(x.view(np.int32)[:, 12:], y.view(np.int32)[:, 12:]) and np.array_equal(woop[w0:w0 + wb], woop[w1:w1 + wb])
    leaf = nodes[n0:n0 + nb].view(np.int32).reshape(-1, 16)[:, 12:14] < 0
    for k in (0, 1):
        lo, hi = rf.BOX_WORDS[k][rf.LO], rf.BOX_WORDS[k][rf.HI]
        m = leaf[:, k]
        assert np.array_equal(y[m][:, lo], (x[m][:, lo] - F(0.001)).astype(F)) and np.array_equal(y[m][:, hi], (x[m][:, hi] + F(0.001)).astype(F))
    assert not np.array_equal(x[:, :12], y[:, :12])


# ---- 7. more entries than one workgroup ----------------------------------------------------------------------------------------------------
def test_more_entries_than_one_workgroup():
    rng = np.random.default_rng(20261101)        # test_ploc_batch_gpu.py's generator of 1100 meshes, another seed
    sizes = [int(x) for x in rng.integers(1, 13, 1100)]
    n = sum(sizes)
    pos = rng.normal(0, 3, (n + 2, 3)).astype(F)
    tri = rng.integers(0, n + 2, (n, 3)).astype(np.int32)
    meshes, first = [], 0
    for s in sizes:
        box = pl.scene_box(pos[tri[first:first + s]])
        meshes.append((first, s, box[0], box[1]))
        first += s
    pool = _Pool(concat=(tri, pos, meshes))
    res = pool.check(hows=(0.3,), what="1100 entries", lanes=1)
    print("1100 entries, %d triangles: %.1f us" % (n, res.seconds * 1e6))


# ---- 8. seeded batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", range(3))
def test_seeded_batches_equal_spec(group):
    """12 batches (four per case) of 2 to 12 meshes of the four kinds of test_ploc_batch_gpu._seeded_mesh -- soup, integer grid, shared
    vertices with degenerate triangles, tiny extents with signed zeros -- each of 1 to 3000 triangles (log-uniform), every second mesh
    an LBVH BLAS, moved by a seeded amplitude; the pool stays under 20 k triangles."""
    rng = np.random.default_rng(20261102 + group)
    for i in range(4 * group, 4 * group + 4):
        parts, total = [], 0
        for _ in range(int(rng.integers(2, 13))):
            n = max(1, int(round(3000.0 ** rng.random())))
            n = min(n, max(1, 19000 - total))
            total += n
            parts.append(_seeded_mesh(rng, int(rng.integers(4)), n))
        pool = _Pool(ploc=parts[0::2], lbvh=parts[1::2])
        amp = float(F(rng.choice([0.0, 0.01, 0.05, 0.3, 1.0])))
        pool.check(hows=(amp,), what=(i, [e[2] for e in pool.entries], amp))


# ---- 9. a malformed entry ------------------------------------------------------------------------------------------------------------------
def test_a_malformed_entry_is_named_and_the_others_are_refitted():
    pool = _Pool(ploc=_soups((40, 300, 129, 1, 25), 10))
    no = pool.entries[2][0][0]
    word = no // 4 + 16 * 5 + 12                  # child 0 of node 5 of entry 2
    for b, h in ((pool.built[0], pool.host[0]),):
        h.view(np.int32)[word] = 0x7FFFFFC0       # a link that names no slot: rejected, never followed
        b.copy_(torch.from_numpy(h))
    pool.reset()
    p = rf.moved(pool.pos, 0.3)
    d_pos = up(p)
    d_boxes = torch.zeros(6 * 5, dtype=torch.float32, device="cuda:0")
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, d_boxes))
    assert e.value.code == -4 and "entry 2" in str(e.value), str(e.value)
    res = e.value.result
    assert (res.numEntries, res.firstBadEntry, res.errBits) == (5, 2, 1)
    good = [pool.entries[k] for k in (0, 1, 3, 4)]
    spec = pool.spec(good, p)
    nodes, woop, idx = pool.download()
    boxes = d_boxes.cpu().numpy().reshape(-1, 6)
    for k, ((n0, nb, w0, wb), _, _, _) in zip((0, 1, 3, 4), good):
        assert np.array_equal(nodes[n0:n0 + nb], spec["nodes"][n0:n0 + nb]) and _woop_equal(woop[w0:w0 + wb], spec["woop"][w0:w0 + wb]), k
    assert boxes[[0, 1, 3, 4]].tobytes() == spec["boxes"].tobytes()
    assert np.array_equal(idx, pool.host[2]) and (nodes[pool.caps[0]:] == 0xAB).all() and (woop[pool.caps[1]:] == 0xAB).all()
    assert nodes.view(np.int32)[word] == 0x7FFFFFC0
    # the asynchronous form skips the malformed part silently and gives the same bytes
    pool.reset()
    assert nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None), blocking=False) is None
    again = pool.download()
    assert np.array_equal(again[0], nodes) and _woop_equal(again[1], woop)
    # two bad entries: the lowest is named
    h = pool.host[0].copy()
    h.view(np.int32)[pool.entries[1][0][0] // 4 + 13] = 0x7FFFFFC0
    pool.bufs[0].copy_(torch.from_numpy(h))
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None))
    assert e.value.code == -4 and e.value.result.firstBadEntry == 1 and "entry 1" in str(e.value)


# ---- 10. asynchronous calls and graphs -------------------------------------------------------------------------------------------------------
def _instanced(pool, sc, rays, d_rays, stream=0):
    """ntr_tlas_build over the pool and both traces; -> (tlas nodes, records, TlasResult, {any_hit: (result words, instance ids)})"""
    inst = ni.instances(sc["transforms"], sc["blas"])
    n = inst.shape[0]
    d_inst = up(inst)
    caps = nt.tlas_capacity(n)
    d_tlas, d_rec = (torch.full((c + 64,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in caps)
    ranges = [e[0] for e in pool.entries]
    res = nt.tlas_build(n, d_inst.data_ptr(), ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(), caps[1],
                        stream=stream)
    out = {}
    for any_hit in (False, True):
        d_res = torch.full((16 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_ids = torch.full((4 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        nt.trace_instanced(rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d_tlas.data_ptr(), res.nodesBytes,
                           res.rootLink, d_rec.data_ptr(), n, pool.bufs[0].data_ptr(), pool.caps[0], pool.bufs[1].data_ptr(), pool.caps[1],
                           pool.bufs[2].data_ptr(), stream=stream, timed=False)
        out[any_hit] = (d_res, d_ids)
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    tlas = d_tlas.cpu().numpy()[:res.nodesBytes].view(np.int32).reshape(-1, 16)
    records = d_rec.cpu().numpy()[:res.recordsBytes].view(np.uint32).reshape(-1, 16)
    words = {ah: (isc.result_words(r.cpu().numpy().view(nt.RESULT_DTYPE)), i.cpu().numpy().view(np.int32)) for ah, (r, i) in out.items()}
    return tlas, records, res, inst, words


def _assert_instanced(pool, sc, rays, spec, got):
    tlas, records, res, inst, words = got
    spool = dict(nodes=spec["nodes"], woop=spec["woop"], tri_index=pool.host[2][:pool.caps[2]].view(np.int32), ranges=[e[0] for e in pool.entries])
    want = ni.tlas_build(spool["nodes"], spool["ranges"], inst, 8)
    assert res.rootLink == want["root_link"] and np.array_equal(tlas, want["nodes"]) and np.array_equal(records, want["records"])
    hits = 0
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst = ni.trace(want["nodes"], want["root_link"], want["records"], spool, rays, any_hit)
        (gid, gt, gu, gv), ids = words[any_hit]
        for name, g, e in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                           ("instance", ids, rinst)):
            assert np.array_equal(g, e), (name, any_hit)
        hits += int((rid >= 0).sum())
    assert hits > 0


def _three():
    sc = isc.scene("three")
    pool = _Pool(ploc=[isc.blas(name)[:2] for name in sc["names"]])
    rays = isc.scene_rays(primary=(48, 24), random=512)
    return sc, pool, rays


def test_asynchronous_refit_then_tlas_build_and_trace_on_one_stream_and_graph_replays():
    sc, pool, rays = _three()
    d_rays = up(rays)
    uploads = [rf.moved(pool.pos, 0.02), rf.moved(pool.pos, 0.3), rf.moved(pool.pos, "collapse")]
    specs = [pool.spec(pool.entries, p) for p in uploads]
    d_pos = up(uploads[0])
    d_boxes = torch.zeros(6 * len(pool.entries), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, d_boxes), stream=s.cuda_stream, blocking=False) is None
        got = _instanced(pool, sc, rays, d_rays, s.cuda_stream)
    pool.assert_pool(pool.entries, uploads[0], d_pos, d_boxes.cpu().numpy().reshape(-1, 6), "asynchronous", spec=specs[0])
    _assert_instanced(pool, sc, rays, specs[0], got)
    # the refit alone as a graph, after an identical uncaptured call (the one above): replayed after each of three vertex uploads
    held = nt.bvh_refit_batch_scratch_bytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, d_boxes), stream=cs, blocking=False)
    assert nt.bvh_refit_batch_scratch_bytes() == held
    for rep, which in enumerate((1, 2, 0)):
        d_pos.copy_(up(uploads[which]))
        pool.reset()
        d_boxes.zero_()
        torch.cuda.synchronize()
        g.replay()
        pool.assert_pool(pool.entries, uploads[which], d_pos, d_boxes.cpu().numpy().reshape(-1, 6), "graph replay %d" % rep, spec=specs[which],
                         loop=rep == 0)
    del g
    # a captured call with another table, with a result, or after the workspace was released: refused, and the library works afterwards
    errs = []

    def capture(entries, blocking=False):
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            cs = torch.cuda.current_stream().cuda_stream
            d_boxes.zero_()      # so that the graph is not empty
            try:
                nt.bvh_refit_batch(*pool.args(pool.bufs, entries, d_pos, d_boxes), stream=cs, blocking=blocking)
            except nt.NtrError as e:
                errs.append((e.code, str(e)))
        torch.cuda.synchronize()

    capture(pool.entries[::-1])
    capture(pool.entries, blocking=True)
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_batch_scratch_bytes() == 0
    capture(pool.entries)
    assert [c for c, _ in errs] == [-1, -1, -1] and "uncaptured call" in errs[0][1] and "uncaptured call" in errs[2][1], errs
    pool.reset()
    d_pos.copy_(up(uploads[1]))
    res = nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, d_boxes))
    assert res.firstBadEntry == -1
    pool.assert_pool(pool.entries, uploads[1], d_pos, d_boxes.cpu().numpy().reshape(-1, 6), "after the refused captures", spec=specs[1], loop=False)


# ---- 11. end to end ------------------------------------------------------------------------------------------------------------------------
def test_deform_refit_rebuild_the_tlas_and_trace():
    sc, pool, rays = _three()
    p = rf.moved(pool.pos, 0.05)
    d_pos = up(p)
    nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None))
    spec = pool.assert_pool(pool.entries, p, d_pos, None, "three")
    _assert_instanced(pool, sc, rays, spec, _instanced(pool, sc, rays, up(rays)))


# ---- 12. determinism and scratch -------------------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_batch_scratch_bytes() == 0
    pool = _Pool(ploc=_soups((1500, 1, 700), 11), lbvh=_soups((2100, 30), 12))
    d_pos = up(rf.moved(pool.pos, 0.3))
    nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None))
    a = pool.download()
    held = nt.bvh_refit_batch_scratch_bytes()
    slots = sum(e[0][1] // 64 for e in pool.entries)
    assert held >= 8 * slots + 36 * len(pool.entries)
    pool.reset()
    nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None))
    b = pool.download()
    assert nt.bvh_refit_batch_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_batch_scratch_bytes() == 0
    pool.reset()
    nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, d_pos, None), blocking=False)
    c = pool.download()
    for other in (b, c):
        for x, y in zip(a, other):
            assert x.tobytes() == y.tobytes()
    print("scratch: %d B for %d slots and %d entries" % (held, slots, len(pool.entries)))
    nt.lbvh_release_workspace()
    assert nt.bvh_refit_batch_scratch_bytes() == 0
