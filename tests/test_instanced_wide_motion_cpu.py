"""Motion blur over the 4-wide trees without a device: the numpy rule (tests/np_instanced_wide_motion.py) against the specs it joins --
at the shutter's two ends it is the wide spec over the same wide nodes with key 0's or key 1's wide records; with nothing moving it is
the wide spec; its refit's boxes are the binary motion refit's at each slot's source and its key buffer the binary one's; inside the
shutter its closest-hit t is the binary motion spec's on every ray; the corner times; and the C-ABI: symbols, every refusal in its
words, the shared refusals in the recorded order, zero rays, no device."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import _capi

import instanced_motion_cases as mc
import instanced_wide_motion_cases as wc
import np_bvh_wide as bw
import np_instanced_motion as mo
import np_instanced_wide as niw
import np_instanced_wide_motion as wm
import np_wide_refit as wr
import test_instanced_wide_fast_capi_cpu as wide
import test_two_level_refusals_cpu as rec

F = np.float32
FAKE = wide.FAKE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, words=5):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a[:words], b[:words]))


# ---- 1. ends of the shutter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_at_the_shutters_ends_the_rule_is_the_wide_spec_with_that_keys_records(name):
    s, rays = wc.named(name), mc.cpu_rays()
    assert s.refit["stats"]["numMoving"] == s.n - s.n // 3 and s.refit["err_bits"] == 0
    for any_hit in (False, True):
        for t, inst in ((0.0, s.inst0), (1.0, s.inst1)):
            got = s.trace(rays, any_hit, times=np.full(rays.shape[0], t, F))
            # the same wide nodes on both sides: another tree has other boxes, another order of the candidates and another any-hit answer
            want = niw.trace(s.refit["nodes"], s.root, s.records_of(inst), s.pool, s.wp, rays, any_hit)
            assert _same(got, want), (name, any_hit, t)
            assert {k: got[5][k] for k in niw.COUNTERS} == want[5], (name, any_hit, t)
            assert got[5]["numSingular"] == 0 and 0 < got[5]["numMovingEntries"] <= got[5]["numInstanceEntries"]


# ---- 2. nothing moving --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_with_nothing_moving_every_byte_and_counter_is_the_wide_specs(name):
    s, rays = wc.named(name), mc.cpu_rays()
    still = s.refit_of(s.inst0, s.inst0)
    plain = wr.refit_wide_tlas(s.wt["nodes"], s.root, s.wt["records"], s.wp["nodes"], s.pool["ranges"], s.wp["ranges"], s.inst0)
    assert still["nodes"].tobytes() == plain["nodes"].tobytes() and still["records"].tobytes() == plain["records"].tobytes()
    assert still["scene_box"].tobytes() == plain["scene_box"].tobytes()
    assert not still["records"][:, 15].any() and still["stats"]["numMoving"] == 0
    assert still["motion_keys"].tobytes() == mo.motion_keys(s.inst0, s.inst0).tobytes()
    times = np.linspace(0.0, 1.0, rays.shape[0]).astype(F)
    for any_hit in (False, True):
        got = wm.trace(still["nodes"], s.root, still["records"], still["motion_keys"], s.pool, s.wp, rays, any_hit, times=times)
        want = niw.trace(plain["nodes"], s.root, plain["records"], s.pool, s.wp, rays, any_hit)
        assert _same(got, want), (name, any_hit)
        assert got[5] == dict(want[5], numMovingEntries=0, numSingular=0), (name, any_hit)


# ---- 3. the refit's boxes and key buffer ---------------------------------------------------------------------------------------------------
def _binary_sources(nodes, n):
    """The binary tree's child slots by the set of instances below them -> {frozenset: the slot's six box words as bytes}."""
    nf = nodes.view(F)
    out = {}

    def below(slot, k):
        c = int(nodes[slot, 12 + k])
        leaves = frozenset([~c]) if c < 0 else below(c // 64, 0) | below(c // 64, 1)
        out[leaves] = nf[slot, mo.BOX_WORDS[k]].tobytes()
        return leaves
    if n > 1:
        assert len(below(0, 0) | below(0, 1)) == n
    return out


def _wide_slots(wi):
    """The wide tree's slots k < count by the set of instances below them -> [(node, k, frozenset, the slot's six box words as bytes)]."""
    wf = wi.view(F)
    out = []

    def below(node, k):
        link = int(wi[node, bw.WLINK + k])
        assert link != 0
        if link < 0:
            leaves = frozenset([~link])
        else:
            ch = link // bw.WIDE_BYTES
            leaves = frozenset().union(*[below(ch, kk) for kk in range(int(wi[ch, bw.WCOUNT]))])
        out.append((node, k, leaves, wf[node, wr.WBOX[k]].tobytes()))
        return leaves
    if wi.shape[0]:
        for k in range(int(wi[0, bw.WCOUNT])):
            below(0, k)
    return out


@pytest.mark.parametrize("name", mc.SCENES + ["big"])
def test_refit_boxes_are_the_binary_motion_refits_at_each_slots_source(name):
    s = wc.big() if name == "big" else wc.named(name)
    r, b = s.refit, s.ms.refit
    assert r["motion_keys"].tobytes() == b["motion_keys"].tobytes()                     # the key buffer, byte for byte
    mv = mo.moving(s.inst0, s.inst1)
    assert np.array_equal(r["records"][:, 15], mv.astype(np.uint32)) and np.array_equal(r["records"][:, :15], s.wt["records"][:, :15])
    assert r["stats"]["numMoving"] == b["stats"]["numMoving"] == int(mv.sum()) > 0
    assert np.array_equal(r["nodes"][:, bw.WLINK:bw.WLINK + 4], s.wt["nodes"][:, bw.WLINK:bw.WLINK + 4])   # topology stays
    src = _binary_sources(b["nodes"], s.n)
    slots = _wide_slots(r["nodes"])
    assert len(slots) >= s.n
    for node, k, leaves, box in slots:
        assert box == src[leaves], (name, node, k, sorted(leaves)[:4])
    wf = r["nodes"].view(F)
    for node in range(r["nodes"].shape[0]):
        for k in range(int(r["nodes"][node, bw.WCOUNT]), 4):                            # padding: a copy of slot 0
            assert wf[node, wr.WBOX[k]].tobytes() == wf[node, wr.WBOX[0]].tobytes()
    assert r["scene_box"].tobytes() == b["scene_box"].tobytes()


# ---- 4. interior times --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_inside_the_shutter_the_closest_hit_is_the_binary_motion_specs(name):
    """Observed on three, grid and mirror at 0.25, 0.5 and 0.8125: 0 rays whose t differs, 0 ties."""
    s, rays = wc.named(name), mc.cpu_rays()
    n = rays.shape[0]
    for tau in mc.INTERIOR:
        got = s.trace(rays, False, time=tau)
        want = s.ms.trace(rays, False, time=tau)
        bad_t = np.flatnonzero(got[1].view(np.uint32) != want[1].view(np.uint32))
        other = (got[0] != want[0]) | (got[4] != want[4])
        print("%s tau=%r: %d of %d rays differ in t, %d in (id, instance) at the same t (ties)" % (name, tau, bad_t.size, n, int(other.sum())))
        assert bad_t.size == 0, (name, tau, bad_t.size, int(bad_t[0]))
        assert int(other.sum()) <= n // 100, (name, tau, int(other.sum()))
        same_uv = ~other
        assert np.array_equal(got[2].view(np.uint32)[same_uv], want[2].view(np.uint32)[same_uv])
        assert np.array_equal(got[3].view(np.uint32)[same_uv], want[3].view(np.uint32)[same_uv])
        assert (got[0] != -1).any() and got[5]["numMovingEntries"] > 0 and got[5]["numSingular"] == 0


# ---- 5. corner times ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_corner_times_as_a_scalar_and_per_ray(name):
    s, rays = wc.named(name), mc.cpu_rays()[:1024]
    n = rays.shape[0]
    at = lambda t: s.trace(rays, False, time=t)                                         # noqa: E731
    t0, t1 = at(0.0), at(1.0)
    for t, like in ((-1.0, t0), (float("nan"), t0), (2.0, t1)):
        got = at(t)
        assert _same(got, like) and got[5] == like[5], (name, t)
    scalar = {}
    for t in mc.CORNER_TIMES:
        scalar[int(t.view(np.uint32))] = got = at(float(t) if t == t else float("nan"))
        want = s.ms.trace(rays, False, time=float(t) if t == t else float("nan"))
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, t)
    assert not _same(scalar[0x00000001], t0) or not _same(scalar[0x3F7FFFFF], t1)      # next to the ends the lerp is the formula
    times = np.resize(mc.CORNER_TIMES, n).astype(F)
    got = s.trace(rays, False, times=times)
    entries = 0
    for bits, want in scalar.items():
        pick = times.view(np.uint32) == bits
        assert _same([np.asarray(x)[pick] for x in got[:5]], [np.asarray(x)[pick] for x in want[:5]]), (name, hex(bits))
        entries += s.trace(rays[pick], False, time=float(np.array([bits], np.uint32).view(F)[0]))[5]["numMovingEntries"]
    assert got[5]["numMovingEntries"] == entries > 0


def test_masks_singular_poses_and_a_cut_key_buffer():
    """np_instanced_motion's corners over the wide trees: a refused moving instance reads no key and counts as masked only; an exactly
    singular pose is a pop counted in numSingular only; a key entry outside the buffer reads as zeros, and a zero matrix is singular."""
    import instanced_scenes as isc
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    s, rays = wc.two_of_one(a, b.reshape(12)), mc.one_rays()
    r = s.refit
    assert r["records"][:, 15].tolist() == [1, 0] and r["nodes"].shape[0] == 1
    for any_hit in (False, True):
        got = s.trace(rays, any_hit, time=0.5)
        assert got[5]["numSingular"] > 0 and got[5]["numMovingEntries"] == 0 and got[5]["numInstancesMasked"] == 0
        assert (got[4] == 1).any() and not (got[4] == 0).any()
        alone = niw.trace(r["nodes"], s.root, r["records"], s.pool, s.wp, rays, any_hit, inst_masks=np.array([0, 1], np.uint32), ray_mask=1)
        assert _same(got, alone)
    assert s.trace(rays, False, time=0.25)[5]["numSingular"] == 0
    cut = wm.trace(r["nodes"], s.root, r["records"], r["motion_keys"][:0], s.pool, s.wp, rays, False, time=0.25)
    assert cut[5]["numSingular"] > 0 and cut[5]["numMovingEntries"] == 0
    poison = r["motion_keys"].copy()
    poison[0] = 0x7FC00000
    M = np.array([2, 1], np.uint32)
    got = wm.trace(r["nodes"], s.root, r["records"], poison, s.pool, s.wp, rays, False, time=0.25, inst_masks=M, ray_mask=1)
    want = niw.trace(r["nodes"], s.root, r["records"], s.pool, s.wp, rays, False, inst_masks=M, ray_mask=1)
    assert _same(got, want) and {k: got[5][k] for k in niw.COUNTERS} == want[5]
    assert got[5]["numInstancesMasked"] > 0 and got[5]["numMovingEntries"] == got[5]["numSingular"] == 0


# ---- 6. the C-ABI without a device --------------------------------------------------------------------------------------------------------
NAMES = ("ntr_tlas_wide_motion_refit", "ntr_tlas_wide_motion_refit_scratch_bytes", "ntr_trace_instanced_wide_motion",
         "ntr_trace_instanced_wide_motion_stats")
GOOD = {k: v for k, v in wide.GOOD.items() if k != "d_flags"}
MOTION = dict(d_motion_keys=FAKE, motion_keys_bytes=128 * GOOD["num_instances"])


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols():
    with open(os.path.join(ROOT, "include", "ntrace_amd.h")) as f:
        header = f.read()
    bound = {s[0] for s in _capi.SYMBOLS}
    for name in NAMES:
        assert re.search(r"NTR_API int\s+%s\(" % name, header), name
        assert name in bound and getattr(nt.lib(), name) is not None
    assert nt.lib().ntr_tlas_wide_motion_refit_scratch_bytes(None) == -1
    assert b"ntr_tlas_wide_motion_refit_scratch_bytes" in nt.lib().ntr_last_error()


def _refusal(name, kw):
    try:
        getattr(nt, name)(**kw)
    except nt.NtrError as e:
        return [e.code, str(e)]
    return [0, ""]


@pytest.mark.parametrize("name,like", [("trace_instanced_wide_motion", "trace_instanced_wide"),
                                       ("trace_instanced_wide_motion_stats", "trace_instanced_wide_stats")])
def test_trace_refusals_new_and_shared(name, like):
    params = inspect.signature(getattr(nt, name)).parameters
    good = {k: v for k, v in GOOD.items() if k in params}
    motion = lambda **kw: nt.InstanceMotion(**dict(MOTION, **kw))           # noqa: E731
    fn = "ntr_" + name
    short = MOTION["motion_keys_bytes"] - 1
    # the three motion refusals, in ntr_trace_instanced_motion's words under this name, and their order
    new = [(dict(d_ray_times=FAKE + 2), "%s: the ray times must be 4-byte aligned"),
           (dict(d_motion_keys=0), "%s: the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
           (dict(d_motion_keys=FAKE + 8), "%s: the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
           (dict(motion_keys_bytes=short), "%s: motionKeysBytes below 128 * numInstances")]
    for change, text in new:
        assert _refusal(name, dict(good, motion=motion(**change))) == [-1, "ntrace_amd error -1: " + text % fn], change
    for (c1, t1), (c2, _) in zip(new, new[1:]):
        if set(c1) != set(c2):
            assert _refusal(name, dict(good, motion=motion(**dict(c1, **c2)))) == [-1, "ntrace_amd error -1: " + t1 % fn], (c1, c2)
    # the golden of test_two_level_refusals_cpu.py for the wide entry point, replayed under this function's name: a shared check fails
    # before a motion one
    with open(rec.GOLDEN) as f:
        golden = json.load(f)[like]
    bad_motion = motion(d_motion_keys=0)
    checked = 0
    for label, kw in rec.cases(like):
        want = golden[label]
        want = [want[0], want[1].replace("ntr_" + like, fn)]
        assert want[0] == -1
        assert _refusal(name, dict(kw, motion=motion())) == want, label
        assert _refusal(name, dict(kw, motion=bad_motion)) == want, label
        checked += 1
    assert checked >= 26
    # with motion == NULL the call is the wide one
    for label, kw in rec.cases(like)[:3]:
        assert _refusal(name, dict(kw, motion=None)) == golden[label], label


def test_zero_rays_null_stats_and_no_device():
    L = nt.lib()
    st, ms = nt.InstancedTraceStats(), nt.InstancedMotionStats()
    mot = nt.InstanceMotion(**MOTION)
    args = (FAKE, FAKE, FAKE, FAKE, 256, 0, FAKE, 5, FAKE, 1408, FAKE, 1680, FAKE, None)
    for m in (C.byref(mot), None):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(ms), 0xFF, C.sizeof(ms))
        assert L.ntr_trace_instanced_wide_motion_stats(0, 0, *args, m, C.byref(st), C.byref(ms), None) == 0
        assert bytes(st) == bytes(64) and bytes(ms) == bytes(16)
        sec = C.c_float(7.0)
        assert L.ntr_trace_instanced_wide_motion(0, 0, *args, m, C.byref(sec), None) == 0 and sec.value == 0.0
    for a, b in ((None, C.byref(ms)), (C.byref(st), None), (None, None)):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(ms), 0xFF, C.sizeof(ms))
        assert L.ntr_trace_instanced_wide_motion_stats(-1, 0, *args, C.byref(mot), a, b, None) == -1
        assert L.ntr_last_error() == b"ntr_trace_instanced_wide_motion_stats: null stats"
        assert (a is None or bytes(st) == bytes(64)) and (b is None or bytes(ms) == bytes(16))
    if not _has_device():
        for name in ("trace_instanced_wide_motion", "trace_instanced_wide_motion_stats"):
            got = _refusal(name, dict(GOOD, motion=mot))
            assert got[0] in (-2, -3), got                                  # NTR_ERR_NO_DEVICE / NTR_ERR_HIP come after the checks


def test_wide_motion_refit_argument_errors_are_decided_before_device_work():
    fake, fake2 = 0x10000, 0x4000000
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    wranges = [(0, 1280, 10, 5), (1280, 128, 1, 1)]
    good = dict(num_instances=5, d_instances0=fake, d_instances1=fake, ranges=ranges, wide_ranges=wranges, d_wide_pool_nodes=fake,
                wide_pool_nodes_bytes=1408, d_wide_tlas_nodes=fake2, wide_tlas_nodes_bytes=256, root_link=0, d_wide_records=fake2 + 4096,
                records_cap=320, d_motion_keys=fake2 + 8192, motion_keys_cap=640)
    # in the order of the checks: each fault together with the next one's names the first
    bad = [(dict(d_instances1=0), "bad arguments"), (dict(d_motion_keys=0), "bad arguments"), (dict(num_instances=0), "bad arguments"),
           (dict(wide_tlas_nodes_bytes=200), "wideTlasNodesBytes must be the extent ntr_tlas_widen reported"),
           (dict(root_link=-1), "rootLink must be 0"), (dict(records_cap=319), "recordsCapacity below 64 * numInstances"),
           (dict(motion_keys_cap=639), "motionKeysCapacity below 128 * numInstances"),
           (dict(d_instances1=fake + 8), "the buffers must be 16-byte aligned"), (dict(d_motion_keys=fake2 + 4), "the buffers must be 16-byte aligned"),
           (dict(d_instances0=fake + 8), "the buffers must be 16-byte aligned"),
           (dict(wide_pool_nodes_bytes=1400), "widePoolNodesBytes must be a multiple of 128"),
           (dict(ranges=[(0, 640, 8, 1600), ranges[1]]), "BLAS 0: triWoopOffset"),
           (dict(wide_ranges=[wranges[0], (1408, 128, 1, 1)]), "wide BLAS 1")]
    for blocking in (True, False):
        for change, text in bad:
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_wide_motion_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: ntr_tlas_wide_motion_refit: ") and text in str(e.value), \
                (change, str(e.value))
            if blocking:
                assert bytes(e.value.result) == bytes(56)
        for (c1, t1), (c2, _) in zip(bad[2:], bad[3:]):
            if set(c1) != set(c2):
                with pytest.raises(nt.NtrError) as e:
                    nt.tlas_wide_motion_refit(**dict(good, **dict(c2, **c1)), blocking=blocking)
                assert t1 in str(e.value), (c1, c2, str(e.value))
    if not _has_device():
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_wide_motion_refit(**good, blocking=blocking)
            assert e.value.code in (-2, -3)
        assert nt.tlas_wide_motion_refit_scratch_bytes() == 0


def test_the_bindings_algorithmic_bytes_equal_the_specs():
    c = dict(numRays=1000, numTopInnerVisits=2100, numInstanceEntries=1500, numInstancesMasked=40, numInnerVisits=5200, numTriTests=800,
             numLeafVisits=790, numHits=333, numMovingEntries=900, numSingular=7)
    st, ms = nt.InstancedWideTraceStats(), nt.InstancedMotionStats()
    for k, v in c.items():
        setattr(ms if k in ("numMovingEntries", "numSingular") else st, k, v)
    for im in (False, True):
        for rm in (False, True):
            for rt in (False, True):
                assert ms.algorithmic_bytes(st, im, rm, rt) == wm.algorithmic_bytes(c, im, rm, rt)
    assert wm.algorithmic_bytes(c, ray_times=True) == niw.algorithmic_bytes(c) + 128 * 907 + 4000
