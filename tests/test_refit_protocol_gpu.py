"""The held-table rule of the five in-place refit entry points (refit_launch.h) on the device, at the smallest shapes where
it can go wrong: ntr_tlas_refit, ntr_tlas_motion_refit, ntr_tlas_wide_refit, ntr_bvh_refit_batch and ntr_pool_wide_refit keep their table
on the device between calls, compare the next call's table with a host copy, and upload only a table that differs -- or whose bytes are
gone, because the scratch pool was released or had to grow.  A mistake there shows as the bytes of another table's refit, so every case
compares every output byte with the numpy rule: nodes, records, motion keys and scene box of a top-level unit; pool nodes, rows and BLAS
boxes of a batch unit.  The helpers and the rules are those of test_tlas_refit_gpu.py, test_instanced_motion_gpu.py,
test_wide_refit_gpu.py and test_refit_batch_gpu.py; the top-level units run over the three BLASes of test_tlas_refit_cpu.pool(), the batch
units over four meshes of 1, 2, 40 and 300 triangles.
The growth case of the top-level units is N = 2, then N = 130 with the same ranges: 129 node slots take 768 bytes each for the climb's
two slices where one slot took 256.  A wide top-level tree of 130 instances has about 62 wide nodes, which still fit 256 bytes, so
the wide unit runs N = 130 all the same and then N = 200 (99 wide nodes), which is where its pool has to grow."""
import copy

import numpy as np
import pytest
import torch

import ntrace_amd as nt

import np_bvh_refit as rf
import test_instanced_motion_gpu as mg
import test_refit_batch_gpu as rbg
import test_tlas_refit_gpu as tg
import test_wide_refit_gpu as wg
from gpu_util import up
from test_tlas_refit_cpu import moved, placed, pool

pytestmark = pytest.mark.gpu

F = np.float32
PREFIX = "ntrace_amd error -1: "
# the refusals of a captured call, as the library worded them before the protocol was stated once
NO_RESULT = "%s: a captured call cannot read a result back (pass result = NULL)"
NO_RANGE_TABLE = ("%s: a captured call uploads and allocates nothing: the device must hold this range table already -- make one uncaptured "
                  "call with the same ranges and instance count first (and none with others, and no ntr_lbvh_release_workspace, between it "
                  "and the capture)")
NO_RANGE_TABLE_WIDE = ("%s: a captured call uploads and allocates nothing: the device must hold this range table already -- make one "
                       "uncaptured call with the same ranges, instance count and extent first (and none with others, and no "
                       "ntr_lbvh_release_workspace, between it and the capture)")
NO_ENTRY_TABLE = ("%s: a captured call uploads and allocates nothing: the device must hold this entry table already -- make one uncaptured "
                  "call with the same entries first (and none with other entries, and no ntr_lbvh_release_workspace, between it and the "
                  "capture)")
MESHES = (1, 2, 40, 300)


def _swapped(ranges):
    """The same BLASes with the ranges of the first and the last exchanged"""
    out = list(ranges)
    out[0], out[-1] = out[-1], out[0]
    return out


# ---- one adapter per entry point: use(table), reset(), run(blocking, stream), check(res, what) -> the rule's bytes ---------------------
class _Binary:
    name, no_table = "ntr_tlas_refit", NO_RANGE_TABLE
    scratch = staticmethod(nt.tlas_refit_scratch_bytes)

    def __init__(self, n=5):
        inst, self.s = tg._three(n)
        self.n, self.new = n, moved(inst, 900 + n)
        self.s.set_instances(self.new)
        self.table_a, self.table_b = list(pool()["ranges"]), _swapped(pool()["ranges"])

    def climbed(self):
        return self.n - 1

    def grow_steps(self):
        return [lambda: type(self)(2), lambda: type(self)(130)]

    def use(self, ranges):
        self.s.ranges = ranges

    def reset(self):
        self.s.set_tree(self.s.built_nodes, self.s.built_records)

    def run(self, blocking=False, stream=0):
        return self.s.refit(blocking=blocking, stream=stream)

    def other_shape(self):
        """-> the call, given a stream, with the same ranges and another instance count (whose scratch is no larger)"""
        other = type(self)(self.n + 1)
        other.use(self.s.ranges)
        return lambda stream: other.run(stream=stream)

    def check(self, res, what):
        want = self.s.spec(pool()["nodes"], self.new)
        assert want["err_bits"] == 0
        self.s.assert_equals(want, res, what)
        return want["nodes"].tobytes() + want["records"].tobytes() + want["scene_box"].tobytes()


class _Motion(_Binary):
    name = "ntr_tlas_motion_refit"
    scratch = staticmethod(nt.tlas_motion_refit_scratch_bytes)

    def __init__(self, n=5):
        inst0 = placed(n, 500 + n)
        inst1 = placed(n, 901 + n, blas=inst0["blas"])
        inst1[::3] = inst0[::3]                  # every third instance stands still
        self.n, self.d = n, mg._Dev(pool(), inst0, inst1)
        self.table_a, self.table_b = list(pool()["ranges"]), _swapped(pool()["ranges"])

    def use(self, ranges):
        self.d.pool = dict(self.d.pool, ranges=ranges)

    def reset(self):
        self.d.reset()

    def run(self, blocking=False, stream=0):
        return self.d.refit(blocking=blocking, stream=stream)

    def other_shape(self):
        other = type(self)(self.n + 1)
        other.use(self.d.pool["ranges"])
        return lambda stream: other.run(stream=stream)

    def check(self, res, what):
        want = self.d.spec()
        assert want["err_bits"] == 0 and want["stats"]["numMoving"] == self.n - (self.n + 2) // 3
        self.d.assert_equals(want, res, what)
        return want["nodes"].tobytes() + want["records"].tobytes() + want["motion_keys"].tobytes() + want["scene_box"].tobytes()


class _Wide(_Binary):
    name, no_table = "ntr_tlas_wide_refit", NO_RANGE_TABLE_WIDE
    scratch = staticmethod(nt.tlas_wide_refit_scratch_bytes)

    def __init__(self, n=5):
        shared = wg._scene_pool()
        shared.reset()
        self.wp = copy.copy(shared)              # its own ranges over the shared buffers
        inst = placed(n, 500 + n)
        self.n, self.s, self.new = n, wg._WideTlas(self.wp, inst), moved(inst, 900 + n)
        self.s.d_inst.copy_(up(self.new))
        self.table_a = (list(shared.ranges), list(shared.wide_ranges))
        self.table_b = (_swapped(shared.ranges), _swapped(shared.wide_ranges))

    def climbed(self):
        return self.s.nodes_bytes // 128

    def grow_steps(self):
        return [lambda: type(self)(2), lambda: type(self)(130), lambda: type(self)(200)]

    def use(self, table):
        self.wp.ranges, self.wp.wide_ranges = table

    def reset(self):
        s = self.s
        s.d_wt[:s.nodes_bytes] = up(s.built_nodes)
        s.d_rec[:s.rec_bytes] = up(s.built_records)
        s.d_scene.fill_(0xAB)

    def other_shape(self):
        """-> the call with the same ranges and instance count and another wideTlasNodesBytes (one node more: the scratch is no larger)"""
        s, wp = self.s, self.wp
        return lambda stream: nt.tlas_wide_refit(s.n, s.d_inst.data_ptr(), wp.ranges, wp.wide_ranges, wp.d_wide.data_ptr(), wp.wide_bytes,
                                                 s.d_wt.data_ptr(), s.nodes_bytes + 128, s.root, s.d_rec.data_ptr(), s.rec_bytes,
                                                 s.d_scene.data_ptr(), stream=stream, blocking=False)

    def check(self, res, what):
        want = self.s.spec(self.wp.wide_host, self.new)
        assert want["err_bits"] == 0
        self.s.assert_equals(want, res, what)
        return want["nodes"].tobytes() + want["records"].tobytes() + want["scene_box"].tobytes()


class _Batch:
    name, no_table = "ntr_bvh_refit_batch", NO_ENTRY_TABLE
    scratch = staticmethod(nt.bvh_refit_batch_scratch_bytes)

    def other_shape(self):
        return None                              # a batch unit's shape is its table

    def __init__(self):
        self.p = rbg._Pool(ploc=rbg._soups(MESHES, 31))
        self.pos = rf.moved(self.p.pos, 0.3)
        self.d_pos = up(self.pos)
        self.table_a = list(self.p.entries)
        self.table_b = [self.table_a[k] for k in (2, 0, 3, 1)]
        self.use(self.table_a)

    def climbed(self):
        return sum(e[0][1] // 64 for e in self.entries)

    def grow_steps(self):
        return [lambda: self.use(self.table_a[:1]) or self, lambda: self.use(self.table_a) or self]

    def use(self, entries):
        self.entries = entries

    def reset(self):
        self.p.reset()
        self.d_boxes = wg._filled(24 * len(self.entries))

    def run(self, blocking=False, stream=0):
        return nt.bvh_refit_batch(*self.p.args(self.p.bufs, self.entries, self.d_pos, self.d_boxes), stream=stream, blocking=blocking)

    def boxes(self):
        torch.cuda.synchronize()
        hb, n = self.d_boxes.cpu().numpy(), 24 * len(self.entries)
        assert (hb[n:] == 0xAB).all(), "bytes beyond the boxes were written"
        return hb[:n].view(F).reshape(-1, 6)

    def check(self, res, what):
        spec = self.p.assert_pool(self.entries, self.pos, self.d_pos, self.boxes(), what, loop=False)
        if res is not None:
            assert (res.numEntries, res.firstBadEntry, res.errBits) == (len(self.entries), -1, 0), what
            assert dict(numNodes=res.numNodes, numLeaves=res.numLeaves, numRows=res.numRows) == spec["stats"], what
        return spec["boxes"].tobytes()


class _WideBatch(_Batch):
    name = "ntr_pool_wide_refit"
    scratch = staticmethod(nt.pool_wide_refit_scratch_bytes)

    def __init__(self):
        self.wp = wg._WidePool(ploc=rbg._soups(MESHES, 31))
        self.pos = rf.moved(self.wp.pool.pos, 0.3)
        self.d_pos = up(self.pos)
        self.table_a, self.table_b = [0, 1, 2, 3], [2, 0, 3, 1]      # (selections of the pool's entries)
        self.use(self.table_a)

    def climbed(self):
        return sum(self.wp.wide_ranges[k][2] for k in self.entries)

    def reset(self):
        self.wp.reset()
        self.d_boxes = wg._filled(24 * len(self.entries))

    def run(self, blocking=False, stream=0):
        return self.wp.call(self.entries, self.d_pos, 1, self.d_boxes, stream=stream, blocking=blocking)

    def check(self, res, what):
        spec = self.wp.spec(self.entries, self.pos, 1)
        self.wp.assert_equals(self.entries, spec, 1, self.boxes(), what)
        if res is not None:
            assert (res.numEntries, res.firstBadEntry, res.errBits) == (len(self.entries), -1, 0), what
            assert dict(numNodes=res.numNodes, numLeafLinks=res.numLeafLinks, numRows=res.numRows) == spec["stats"], what
        return spec["boxes"].tobytes()


UNITS = dict(tlas=_Binary, motion=_Motion, wide_tlas=_Wide, batch=_Batch, wide_batch=_WideBatch)
TLAS_UNITS = ("tlas", "motion", "wide_tlas")
_made = {}


def _unit(key):
    """The entry point's adapter (five instances, or the four meshes), made once, with table A"""
    if key not in _made:
        _made[key] = UNITS[key]()
    u = _made[key]
    u.use(u.table_a)
    return u


def _asynchronous(u, stream, what):
    """One asynchronous call on `stream` over outputs as they were before any refit -> the rule's bytes, which the device's equal"""
    u.reset()
    torch.cuda.synchronize()
    assert u.run(blocking=False, stream=stream.cuda_stream) is None
    return u.check(None, what)


def _captured(stream, fn):
    """fn(the capturing stream) under a capture that is ended and discarded -> the refusal as str(NtrError), or None if fn returned"""
    refusal = None
    dummy = torch.zeros(16, device="cuda:0")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        dummy.zero_()                            # so that the graph is not empty
        try:
            fn(torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            assert e.code == -1
            refusal = str(e)
    torch.cuda.synchronize()
    del g
    return refusal


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(UNITS))
def test_table_a_then_b_then_a_asynchronous_on_one_stream(key):
    """B: the same instance count with the ranges of two BLASes exchanged, or the same entries in another order.  A compare that wrongly
    says "same" leaves B's outputs computed with A's table."""
    u = _unit(key)
    st = torch.cuda.Stream()
    rule = []
    for label, table in (("A", u.table_a), ("B", u.table_b), ("A again", u.table_a)):
        u.use(table)
        rule.append(_asynchronous(u, st, (key, label)))
    assert rule[0] == rule[2] and rule[0] != rule[1]               # B's bytes are not A's: the comparison can tell them apart
    assert nt.trace_status() == 0


@pytest.mark.parametrize("key", list(UNITS))
def test_a_grown_scratch_gets_the_table_again(key):
    """A growing scratch gives a fresh block whose table bytes are undefined, and an unchanged table on the host must not vouch for them
    (the top-level units: the same ranges at every size; the batch units: one entry, then all four)."""
    nt.lbvh_release_workspace()
    st = torch.cuda.Stream()
    steps = _unit(key).grow_steps()
    held, climbed = [], []
    for k, step in enumerate(steps):
        u = step()
        assert UNITS[key].scratch() == (held[-1] if held else 0)   # (making the step's trees does not touch this pool)
        _asynchronous(u, st, (key, "growth step", k))
        held.append(UNITS[key].scratch())
        climbed.append(u.climbed())
    print("%s: %s slots or nodes, scratch %s B" % (key, climbed, held))
    assert climbed[0] <= 64 < climbed[-1] and 0 < held[0] <= held[-2] < held[-1], (climbed, held)
    if key == "wide_tlas":
        assert climbed[1] <= 64 and held[1] == held[0]             # 130 instances: the wide tree's slices still fit
    _unit(key)
    assert nt.trace_status() == 0


@pytest.mark.parametrize("key", list(UNITS))
def test_after_a_release_the_table_is_uploaded_again(key):
    nt.lbvh_release_workspace()                                    # (an earlier case may have left the pool larger than this one needs)
    u = _unit(key)
    st = torch.cuda.Stream()
    first = _asynchronous(u, st, (key, "before the release"))
    held = u.scratch()
    assert held > 0
    nt.lbvh_release_workspace()
    assert u.scratch() == 0
    assert _asynchronous(u, st, (key, "after the release")) == first
    assert u.scratch() == held
    assert nt.trace_status() == 0


@pytest.mark.parametrize("key", list(UNITS))
def test_refused_captures_say_what_they_said_and_allocate_nothing(key):
    nt.lbvh_release_workspace()
    u = _unit(key)
    st = torch.cuda.Stream()
    _asynchronous(u, st, (key, "the uncaptured call"))
    held = u.scratch()
    want = [PREFIX + NO_RESULT % u.name, PREFIX + u.no_table % u.name]
    got = [_captured(st, lambda cs: u.run(blocking=True, stream=cs))]
    u.use(u.table_b)
    got.append(_captured(st, lambda cs: u.run(stream=cs)))
    u.use(u.table_a)
    other = u.other_shape()                                        # (made outside the capture)
    if other is not None:
        got.append(_captured(st, other))
        want.append(PREFIX + u.no_table % u.name)
    assert got == want
    assert u.scratch() == held                                     # no refusal allocated or released anything
    nt.lbvh_release_workspace()
    assert u.scratch() == 0
    assert _captured(st, lambda cs: u.run(stream=cs)) == PREFIX + u.no_table % u.name
    assert u.scratch() == 0
    # the library works afterwards, and holds what it held
    u.reset()
    res = u.run(blocking=True)
    u.check(res, (key, "after the refusals"))
    assert u.scratch() == held
    assert nt.trace_status() == 0


@pytest.mark.parametrize("key", list(UNITS))
def test_the_blocking_form_after_the_asynchronous_one_gives_the_same_bytes_and_the_rules_counts(key):
    u = _unit(key)
    st = torch.cuda.Stream()
    rule = _asynchronous(u, st, (key, "asynchronous"))
    u.reset()
    torch.cuda.synchronize()
    res = u.run(blocking=True, stream=st.cuda_stream)
    assert (res.refit if key == "motion" else res).errBits == 0 and (res.refit if key == "motion" else res).seconds > 0
    assert u.check(res, (key, "blocking")) == rule                 # (check compares the counters, the scene box and numMoving too)
    assert nt.trace_status() == 0


@pytest.mark.parametrize("key", TLAS_UNITS)
def test_one_instance_in_both_forms(key):
    """N == 1: the *_single kernel and its scene-box write"""
    u = UNITS[key](1)
    st = torch.cuda.Stream()
    rule = _asynchronous(u, st, (key, "N = 1, asynchronous"))
    u.reset()
    torch.cuda.synchronize()
    res = u.run(blocking=True, stream=st.cuda_stream)
    r = res.refit if key == "motion" else res
    assert (r.numNodes, r.numLeaves, r.errBits) == (0, 1, 0)
    assert u.check(res, (key, "N = 1, blocking")) == rule
    assert nt.trace_status() == 0
