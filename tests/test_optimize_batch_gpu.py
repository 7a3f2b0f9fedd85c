"""ntr_bvh_optimize_batch and ntr_bvh_sah_cost_batch on the device.  Pools are built on the device as test_refit_batch_gpu.py builds them
-- PLOC BLASes by ntr_ploc_build_batch, one LBVH BLAS (leafSize 8) by ntr_lbvh_build into its own region, 256 bytes of 0xAB slack behind
every buffer -- then, for the deformed cases, moved by np_bvh_refit.deform and refitted by ntr_bvh_refit_batch; the downloaded bytes
are the spec's input.  After every call the node buffer is compared twice, byte for byte: with the numpy spec
(tests/np_optimize_batch.py: np_bvh_optimize per entry) and with a loop of ntr_bvh_optimize calls at pool + offset on a copy.  The slack,
the unlisted ranges, triWoop and triIndex must be what they were.  The shapes are the smallest where the segmented kernels can go
wrong: entry edges on wave and workgroup edges of the joint slot space, BLASes too small for a treelet, more entries than a workgroup
has threads, one large BLAS alone, a subset in scrambled order, malformed entries."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_scenes as isc
import np_bvh_optimize as opt
import np_bvh_refit as rf
import np_instanced as ni
import np_optimize_batch as ob
import np_refit_batch as rb
from gpu_util import up
from test_bvh_optimize_gpu import _same_float
from test_ploc_batch_gpu import _soup, _woop_equal
from test_refit_batch_gpu import _Pool, _soups

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 2, 6, 7, 8, 63, 64, 65, 129, 300, 1000)
HOWS = (None, 0.1, 0.3)                          # the vertices as built, and moved (then refitted on the device)
PASSES = (1, 2, 8)


def spec_steps(ranges, nodes, counts=PASSES):
    """np_optimize_batch.optimize(ranges, nodes, c) for every c of counts, at the cost of max(counts) passes: np_bvh_optimize.optimize
    one pass at a time (k single passes are one call of k: a pass carries no state but the tree, test_optimize_batch_cpu.py), and a
    pass that rewrites nothing has reached a fixed point, which every later pass repeats.  -> {c: dict(nodes, formed, rewritten,
    heightBefore, heightAfter)}"""
    nodes = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8)
    out = {c: dict(nodes=nodes.copy(), formed=[0] * c, rewritten=[0] * c, heightBefore=[], heightAfter=[]) for c in counts}
    for no, nb in ((int(r[0]), int(r[1])) for r in ranges):
        cur, stats = nodes[no:no + nb], []
        for p in range(max(counts)):
            if stats and stats[-1]["rewritten"] == 0:
                stats.append(stats[-1])
            else:
                r = opt.optimize(cur, 1)
                cur = r["nodes"].reshape(-1).view(np.uint8)
                stats.append(r["passes"][0])
            if p + 1 in counts:
                o = out[p + 1]
                o["nodes"][no:no + nb] = cur
                o["heightBefore"].append(stats[0]["heightBefore"])
                o["heightAfter"].append(stats[p]["heightAfter"])
                for q in range(p + 1):
                    o["formed"][q] += stats[q]["formed"]
                    o["rewritten"][q] += stats[q]["rewritten"]
    return out


class _Case:
    """A device pool brought to one of HOWS; base_*: its bytes on the device and on the host, the input of every call and of the spec."""

    def __init__(self, pool, how):
        self.pool, self.how = pool, how
        pool.reset()
        self.pos = pool.pos if how is None else rf.moved(pool.pos, how)
        if how is not None:
            nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, up(self.pos), None))
        torch.cuda.synchronize()
        self.base_dev = [b.clone() for b in pool.bufs]
        self.base = [b.cpu().numpy() for b in pool.bufs]
        self.ranges = [e[0] for e in pool.entries]
        self._spec = {}

    def restore(self):
        for b, src in zip(self.pool.bufs, self.base_dev):
            b.copy_(src)

    def spec(self, sel):
        key = tuple(sel)
        if key not in self._spec:
            self._spec[key] = spec_steps([self.ranges[k] for k in sel], self.base[0][:self.pool.caps[0]])
        return self._spec[key]

    def loop(self, sel, passes):
        """The parent's path: one ntr_bvh_optimize per entry at pool + offset on a copy.  -> the node buffer, slack included"""
        d = self.base_dev[0].clone()
        for k in sel:
            no, nb = self.ranges[k][:2]
            nt.bvh_optimize(d.data_ptr() + no, nb, passes)
        torch.cuda.synchronize()
        return d.cpu().numpy()

    def check(self, passes, sel=None, loop=True, entry_results=True):
        sel = list(range(len(self.ranges))) if sel is None else list(sel)
        pool, what = self.pool, (self.how, passes, len(sel))
        self.restore()
        res, per = nt.bvh_optimize_batch([self.ranges[k] for k in sel], pool.bufs[0].data_ptr(), pool.caps[0], passes, entry_results=entry_results)
        nodes, woop, idx = pool.download()
        spec = self.spec(sel)[passes]
        cn = pool.caps[0]
        assert np.array_equal(woop, self.base[1]) and np.array_equal(idx, self.base[2]), ("triWoop, triIndex or their slack changed", what)
        assert (nodes[cn:] == 0xAB).all(), ("slack written", what)
        for k in sel:                            # entry by entry, so that a failure names the entry
            no, nb = self.ranges[k][:2]
            assert np.array_equal(nodes[no:no + nb], spec["nodes"][no:no + nb]), ("nodes differ from the spec", what, k, self.pool.entries[k][2])
        assert np.array_equal(nodes[:cn], spec["nodes"]), ("node bytes outside the listed ranges changed", what)
        if loop:
            assert np.array_equal(nodes, self.loop(sel, passes)), ("differs from the loop of ntr_bvh_optimize", what)
        print("how %s passes %d, %d entries: formed %s rewritten %s, heights %d -> %d, %d launches, %d read-backs, %.1f us" % (
            self.how, passes, len(sel), list(res.formed)[:passes], list(res.rewritten)[:passes], res.maxHeightBefore, res.maxHeightAfter,
            res.launches, res.readBacks, res.seconds * 1e6))
        assert (res.numEntries, res.passes, res.firstBadEntry, res.errBits) == (len(sel), passes, -1, 0) and res.seconds > 0, what
        assert list(res.formed)[:passes] == spec["formed"] and list(res.rewritten)[:passes] == spec["rewritten"], what
        assert not any(list(res.formed)[passes:]) and not any(list(res.rewritten)[passes:])
        assert (res.maxHeightBefore, res.maxHeightAfter) == (max(spec["heightBefore"]), max(spec["heightAfter"])), what
        tallest = max(max(self.spec(sel)[c]["heightBefore"] + self.spec(sel)[c]["heightAfter"]) for c in PASSES if c <= passes)
        assert 5 * passes + 2 <= res.launches <= passes * (5 + tallest) + 2, (what, res.launches, tallest)
        assert res.readBacks == passes + 1 + (1 if entry_results else 0), (what, res.readBacks)      # no tree here is 1024 high
        if entry_results:
            assert [p.heightBefore for p in per] == spec["heightBefore"] and [p.heightAfter for p in per] == spec["heightAfter"], what
            for k, p in zip(sel, per):
                slots = opt.sah_cost(self.base[0][self.ranges[k][0]:][:self.ranges[k][1]], self.base[1][self.ranges[k][2]:][:self.ranges[k][3]])
                assert (p.numNodes, p.numLeafLinks, p.errBits) == (slots["numNodes"], slots["numNodes"] + 1, 0), (what, k)
        else:
            assert per is None
        return res


_pools = {}


def _pool(name):
    if name not in _pools:
        if name == "mixed":                      # PLOC BLASes of SIZES and an LBVH BLAS of wide leaves behind them
            _pools[name] = _Pool(ploc=_soups(SIZES, 21), lbvh=[_soup(700, 2121)])
        elif name == "many":                     # more entries than a workgroup has threads
            rng = np.random.default_rng(20261201)
            _pools[name] = _Pool(ploc=[_soup(int(n), 3000 + k) for k, n in enumerate(rng.integers(7, 10, 300))])
        else:
            _pools[name] = _Pool(ploc=[_soup(3000, 23)])
    return _pools[name]


# ---- 1. entry edges on wave and workgroup edges; BLASes too small for a treelet; an LBVH BLAS ---------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_mixed_sizes_equal_the_spec_and_the_loop(how):
    """PLOC BLASes of 1, 2, 6, 7, 8, 63, 64, 65, 129, 300, 1 000 triangles have 1, 1, 5, 6, 7, 62, 63, 64, 128, 299, 999 node slots: the
    running sums 1, 2, 7, 13, 20, 82, 145, 209, 337, 636 put entry edges inside waves, and the 64-slot and 128-slot entries end on wave
    edges of the joint slot space shifted by the small ones in front."""
    pool = _pool("mixed")
    assert [e[0][1] // 64 for e in pool.entries[:len(SIZES)]] == [max(n - 1, 1) for n in SIZES]
    case = _Case(pool, how)
    for passes in PASSES:
        res = case.check(passes)
        assert res.formed[0] >= 9                # every BLAS of 7 triangles or more roots at least one treelet
    if how is not None:
        assert res.rewritten[0] > 0
    # a subset in scrambled order: the others stay as they are, and the NULL entryResults form skips its read-back
    case.check(2, sel=(10, 3, 11, 0, 7, 5))
    case.check(2, sel=(9, 6), entry_results=False)
    for k in (0, 1, 2):                          # fewer than 7 leaf links: never a treelet, never a change
        no, nb = case.ranges[k][:2]
        assert np.array_equal(case.spec(range(len(case.ranges)))[8]["nodes"][no:no + nb], case.base[0][no:no + nb])


# ---- 2. more entries than a workgroup has threads -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_three_hundred_small_blases(how):
    case = _Case(_pool("many"), how)
    many = [case.check(passes, loop=passes == 2) for passes in PASSES]
    one = [case.check(passes, sel=(150,), loop=False) for passes in PASSES]
    # the host cost follows the tallest BLAS, not the number of BLASes
    assert [r.readBacks for r in many] == [r.readBacks for r in one] == [p + 2 for p in PASSES]
    assert all(r.launches <= p * (5 + 8) + 2 for r, p in zip(many, PASSES))      # a BLAS of at most 9 triangles is at most 8 high


# ---- 3. one large BLAS alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_one_blas_of_3000_triangles_alone(how):
    case = _Case(_pool("one"), how)
    for passes in PASSES:
        res = case.check(passes)
    copy = case.base_dev[0].clone()
    one = nt.bvh_optimize(copy.data_ptr(), case.ranges[0][1], 8)
    for key in ("formed", "rewritten"):          # one entry: ntr_bvh_optimize's own counts
        assert list(getattr(res, key)) == list(getattr(one, key)), key
    assert (res.maxHeightBefore, res.maxHeightAfter) == (one.heightBefore[0], one.heightAfter[7])


# ---- 4. malformed entries -------------------------------------------------------------------------------------------------------------------
def test_malformed_entries_are_named_and_the_others_are_optimised():
    pool = _Pool(ploc=_soups((40, 300, 129, 1, 25), 24))
    case = _Case(pool, 0.1)
    h = case.base[0].copy()
    no2, no1 = case.ranges[2][0], case.ranges[1][0]
    word = no2 // 4 + 16 * 5 + 12                 # child 0 of node 5 of entry 2: a link that names a slot of the pool, outside its own BLAS
    h.view(np.int32)[word] = 64 * (case.ranges[2][1] // 64 + 3)
    case.base[0] = h
    case.base_dev[0] = torch.from_numpy(h).cuda()
    case.restore()
    spec = ob.optimize(case.ranges, h[:pool.caps[0]], 2)
    assert spec["errBits"] == [0, 0, 1, 0, 0] and spec["per_entry"][2]["bad_links"] == 1
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_optimize_batch(case.ranges, pool.bufs[0].data_ptr(), pool.caps[0], 2)
    assert e.value.code == -4 and "entry 2" in str(e.value), str(e.value)
    res, per = e.value.result, e.value.entry_results
    assert (res.numEntries, res.passes, res.firstBadEntry, res.errBits) == (5, 2, 2, nt.OPT_ERR_LINK)
    assert [p.errBits for p in per] == spec["errBits"]
    assert list(res.formed)[:2] == spec["formed"] and list(res.rewritten)[:2] == spec["rewritten"]
    assert [p.heightAfter for p in per] == spec["heightAfter"]
    nodes = pool.download()[0]
    assert np.array_equal(nodes[:pool.caps[0]], spec["nodes"]) and (nodes[pool.caps[0]:] == 0xAB).all()   # the link was never followed
    d = case.base_dev[0].clone()                 # the loop of ntr_bvh_optimize writes the same bytes and reports the same entry
    codes = []
    for no, nb in (r[:2] for r in case.ranges):
        try:
            nt.bvh_optimize(d.data_ptr() + no, nb, 2)
            codes.append(0)
        except nt.NtrError as err:
            codes.append(err.code)
    assert codes == [0, 0, -4, 0, 0] and np.array_equal(nodes, d.cpu().numpy())
    # entry 1's slot 0 zero-filled on top: no tree.  It is named (the lower index), its bytes stay, every other entry equals the spec
    h2 = h.copy()
    h2[no1:no1 + 64] = 0
    case.base[0], case.base_dev[0] = h2, torch.from_numpy(h2).cuda()
    case.restore()
    spec = ob.optimize(case.ranges, h2[:pool.caps[0]], 2)
    assert spec["errBits"] == [0, nt.OPT_ERR_NO_TREE, nt.OPT_ERR_LINK, 0, 0]
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_optimize_batch(case.ranges, pool.bufs[0].data_ptr(), pool.caps[0], 2)
    assert e.value.code == -4 and "entry 1" in str(e.value), str(e.value)
    res, per = e.value.result, e.value.entry_results
    assert (res.firstBadEntry, res.errBits) == (1, nt.OPT_ERR_LINK | nt.OPT_ERR_NO_TREE)
    assert [p.errBits for p in per] == spec["errBits"]
    nodes = pool.download()[0]
    assert np.array_equal(nodes[no1:no1 + case.ranges[1][1]], h2[no1:no1 + case.ranges[1][1]])
    assert np.array_equal(nodes[:pool.caps[0]], spec["nodes"]) and (nodes[pool.caps[0]:] == 0xAB).all()
    assert list(res.formed)[:2] == spec["formed"] and list(res.rewritten)[:2] == spec["rewritten"]


# ---- 5. the SAH cost of every BLAS ------------------------------------------------------------------------------------------------------------
def _assert_costs(case, entries, what, code=None):
    pool = case.pool
    args = (pool.bufs[0].data_ptr(), pool.caps[0], pool.bufs[1].data_ptr(), pool.caps[1])
    got, res = nt.bvh_sah_cost_batch(entries, *args)
    nodes, woop, _ = pool.download()
    want = ob.sah_costs(entries, nodes[:pool.caps[0]], woop[:pool.caps[1]])
    assert (res.numEntries, res.firstBadEntry, res.errBits, res.launches, res.readBacks) == (len(entries), -1, 0, 2, 1) and res.seconds > 0
    for k, (g, w, (no, nb, wo, wb)) in enumerate(zip(got, want, entries)):
        one = nt.bvh_sah_cost(args[0] + no, nb, args[2] + wo, wb)
        assert _same_float(g.sahCost, w["sahCost"]) and _same_float(g.sahCost, one.sahCost), (what, k, g.sahCost, w["sahCost"], one.sahCost)
        assert (g.numNodes, g.numLeaves, g.numTris, g.height) == (w["numNodes"], w["numLeaves"], w["numTris"], w["height"]), (what, k)
        assert (g.numNodes, g.numLeaves, g.numTris, g.height) == (one.numNodes, one.numLeaves, one.numTris, one.height), (what, k)
        assert g.seconds == 0
    return got


@pytest.mark.parametrize("how", (None, 0.3, "collapse"))
def test_sah_costs_equal_the_spec_and_the_loop_before_and_after_optimising(how):
    case = _Case(_pool("mixed"), how)
    case.restore()
    dup = case.ranges + [case.ranges[9], case.ranges[0], case.ranges[9]]         # the call only reads: entries may repeat
    before = _assert_costs(case, dup, (how, "before"))
    assert [c.numTris for c in before[:len(SIZES)]] == list(SIZES)
    if how == "collapse":
        assert not all(np.isfinite(c.sahCost) for c in before)                   # zero areas: NaN or infinity, returned as they come
    nt.bvh_optimize_batch(case.ranges, case.pool.bufs[0].data_ptr(), case.pool.caps[0], 2)
    after = _assert_costs(case, dup, (how, "after"))
    if how == 0.3:
        # With one triangle per leaf the cost is the sum of the inner boxes' areas over the root's, plus the leaves' share, and every
        # rewritten treelet lowers that sum strictly; the hundreds rewritten in the 300- and 1 000-triangle BLASes lower their cost by a
        # tenth and more, far beyond binary32's rounding.  (The one- and two-triangle BLASes have an empty child box: their cost is NaN.)
        for k in (9, 10):
            assert np.isfinite(before[k].sahCost) and after[k].sahCost < before[k].sahCost, (k, before[k].sahCost, after[k].sahCost)
    # a scrambled subset
    _assert_costs(case, [case.ranges[k] for k in (11, 4, 8, 1)], (how, "subset"))


def test_a_malformed_entry_of_the_cost_is_named_and_every_result_is_filled():
    pool = _Pool(ploc=_soups((40, 129, 25), 25))
    case = _Case(pool, None)
    h = case.base[0].copy()
    h.view(np.int32)[case.ranges[1][0] // 4 + 16 * 3 + 13] = 0x7FFFFFC0
    pool.bufs[0].copy_(torch.from_numpy(h).cuda())
    args = (pool.bufs[0].data_ptr(), pool.caps[0], pool.bufs[1].data_ptr(), pool.caps[1])
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_sah_cost_batch(case.ranges, *args)
    assert e.value.code == -4 and (e.value.result.firstBadEntry, e.value.result.errBits) == (1, nt.OPT_ERR_LINK)
    want = ob.sah_costs(case.ranges, h[:pool.caps[0]], case.base[1][:pool.caps[1]])
    for k, (g, w) in enumerate(zip(e.value.entry_results, want)):
        assert _same_float(g.sahCost, w["sahCost"]), k
        assert (g.numNodes, g.numLeaves, g.numTris, g.height) == (w["numNodes"], w["numLeaves"], w["numTris"], w["height"]), k
    # a row range cut short: the leaves behind the cut find no terminator inside their own BLAS's rows, though the pool goes on
    case.restore()
    no, nb, wo, wb = case.ranges[0]
    cut = [(no, nb, wo, wb - 16 * 40)] + case.ranges[1:]
    with pytest.raises(nt.NtrError) as e:
        nt.bvh_sah_cost_batch(cut, *args)
    assert e.value.code == -4 and (e.value.result.firstBadEntry, e.value.result.errBits) == (0, nt.OPT_ERR_ROW)
    one = None
    try:
        nt.bvh_sah_cost(args[0] + no, nb, args[2] + wo, wb - 16 * 40)
    except nt.NtrError as err:
        one = err.code
    assert one == -4
    assert e.value.entry_results[0].numTris < 40 and e.value.entry_results[1].numTris == 129


# ---- 6. what follows an optimised pool ----------------------------------------------------------------------------------------------------------
def test_a_refit_batch_after_optimising_equals_the_spec_on_the_optimised_pool():
    pool = _pool("mixed")
    case = _Case(pool, 0.3)
    case.restore()
    nt.bvh_optimize_batch(case.ranges, pool.bufs[0].data_ptr(), pool.caps[0], 2)
    nodes, woop, idx = pool.download()
    p = rf.moved(pool.pos, 0.02)
    d_boxes = torch.zeros(6 * len(pool.entries), dtype=torch.float32, device="cuda:0")
    res = nt.bvh_refit_batch(*pool.args(pool.bufs, pool.entries, up(p), d_boxes))
    spec = rb.refit(pool.entries, nodes[:pool.caps[0]], woop[:pool.caps[1]], idx[:pool.caps[2]].view(np.int32), pool.tri, p)
    gn, gw, gi = pool.download()
    assert np.array_equal(gn[:pool.caps[0]], spec["nodes"]) and _woop_equal(gw[:pool.caps[1]], spec["woop"]) and np.array_equal(gi, idx)
    assert d_boxes.cpu().numpy().tobytes() == spec["boxes"].tobytes()
    assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == spec["stats"]


def test_trace_over_the_optimised_pool_and_the_unchanged_tlas_equals_the_spec():
    sc = isc.scene("three")
    pool = _Pool(ploc=[isc.blas(name)[:2] for name in sc["names"]])
    case = _Case(pool, 0.1)
    case.restore()
    inst = ni.instances(sc["transforms"], sc["blas"])
    n = inst.shape[0]
    d_inst = up(inst)
    caps = nt.tlas_capacity(n)
    d_tlas, d_rec = (torch.full((c + 64,), 0xAB, dtype=torch.uint8, device="cuda:0") for c in caps)
    tres = nt.tlas_build(n, d_inst.data_ptr(), case.ranges, pool.bufs[0].data_ptr(), pool.caps[0], d_tlas.data_ptr(), caps[0], d_rec.data_ptr(),
                         caps[1])
    torch.cuda.synchronize()
    tlas_before, rec_before = d_tlas.cpu().numpy(), d_rec.cpu().numpy()
    res, _ = nt.bvh_optimize_batch(case.ranges, pool.bufs[0].data_ptr(), pool.caps[0], 2)
    assert res.rewritten[0] > 0
    nodes, woop, idx = pool.download()
    spool = dict(nodes=nodes[:pool.caps[0]], woop=woop[:pool.caps[1]], tri_index=idx[:pool.caps[2]].view(np.int32), ranges=case.ranges)
    # the top-level tree built before is the tree a build over the optimised pool gives: every BLAS's node-0 union kept its bits
    want = ni.tlas_build(spool["nodes"], spool["ranges"], inst, 8)
    tlas = tlas_before[:tres.nodesBytes].view(np.int32).reshape(-1, 16)
    records = rec_before[:tres.recordsBytes].view(np.uint32).reshape(-1, 16)
    assert tres.rootLink == want["root_link"] and np.array_equal(tlas, want["nodes"]) and np.array_equal(records, want["records"])
    rays = isc.scene_rays(primary=(37, 1), random=4096)
    assert rays.shape[0] == 4096 + 37
    d_rays = up(rays)
    hits = 0
    for any_hit in (False, True):
        d_res = torch.full((16 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_ids = torch.full((4 * rays.shape[0],), 0xAB, dtype=torch.uint8, device="cuda:0")
        nt.trace_instanced(rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d_tlas.data_ptr(), tres.nodesBytes,
                           tres.rootLink, d_rec.data_ptr(), n, pool.bufs[0].data_ptr(), pool.caps[0], pool.bufs[1].data_ptr(), pool.caps[1],
                           pool.bufs[2].data_ptr(), timed=False)
        torch.cuda.synchronize()
        assert nt.trace_status() == 0
        gid, gt, gu, gv = isc.result_words(d_res.cpu().numpy().view(nt.RESULT_DTYPE))
        ids = d_ids.cpu().numpy().view(np.int32)
        rid, rt, ru, rv, rinst = ni.trace(tlas, tres.rootLink, records, spool, rays, any_hit)
        for name, g, w in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                           ("instance", ids, rinst)):
            assert np.array_equal(g, w), (name, any_hit)
        hits += int((rid >= 0).sum())
    assert hits > 100
    assert np.array_equal(d_tlas.cpu().numpy(), tlas_before) and np.array_equal(d_rec.cpu().numpy(), rec_before)


# ---- 7. what the calls refuse, and the scratch ----------------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused():
    d_buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        d_buf.fill_(0)   # so that the graph is not empty
        for call in (lambda: nt.bvh_optimize_batch([(0, 128)], d_buf.data_ptr(), 1024, 1, cs),
                     lambda: nt.bvh_sah_cost_batch([(0, 128, 0, 64)], d_buf.data_ptr(), 1024, d_buf.data_ptr() + 2048, 1024, cs)):
            try:
                call()
            except nt.NtrError as e:
                errs.append((e.code, "captured" in str(e)))
    assert errs == [(-1, True), (-1, True)]
    assert not d_buf.cpu().numpy().any()


def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.bvh_optimize_batch_scratch_bytes() == 0
    case = _Case(_pool("mixed"), 0.3)
    runs = []
    for _ in range(2):
        case.restore()
        nt.bvh_optimize_batch(case.ranges, case.pool.bufs[0].data_ptr(), case.pool.caps[0], 8)
        runs.append(case.pool.download()[0])
    assert np.array_equal(runs[0], runs[1])
    slots = sum(r[1] // 64 for r in case.ranges)
    held = nt.bvh_optimize_batch_scratch_bytes()
    assert held >= 40 * slots + 64 * len(case.ranges)
    assert nt.bvh_optimize_scratch_bytes() == 0              # the single-tree calls' pool is another
    nt.bvh_sah_cost_batch(case.ranges, case.pool.bufs[0].data_ptr(), case.pool.caps[0], case.pool.bufs[1].data_ptr(), case.pool.caps[1])
    assert nt.bvh_optimize_batch_scratch_bytes() >= max(held, 56 * slots)
    nt.lbvh_release_workspace()
    assert nt.bvh_optimize_batch_scratch_bytes() == 0
