"""Motion blur in instanced scenes without a device: the numpy rule (tests/np_instanced_motion.py) against the specs it extends -- at the
shutter's two ends it is the masked spec over the same node buffer with key 0's or key 1's records, inside the shutter the static spec
over the scene posed at that time and the binary64 brute force; the refit rule; the rule's corners on two instances of one triangle;
and the C-ABI: symbols, struct sizes, every refusal in its words, the shared refusals in the recorded order, zero rays, no device."""
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
import instanced_scenes as isc
import np_hlbvh
import np_instanced as ni
import np_instanced_masked as nm
import np_instanced_motion as mo
import np_tlas_refit as tr
import test_instanced_fast_capi_cpu as binary
import test_two_level_refusals_cpu as rec

F = np.float32
FAKE = binary.FAKE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, words=5):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a[:words], b[:words]))


def _records_of(s, inst):
    return np.stack([tr.record_of(inst[i], s.pool["ranges"]) for i in range(s.n)])


# ---- 1. ends ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_at_the_shutters_ends_the_rule_is_the_masked_spec_with_that_keys_records(name):
    s, rays = mc.named(name), mc.cpu_rays()
    assert s.refit["stats"]["numMoving"] == s.n - s.n // 3
    for any_hit in (False, True):
        for t, inst in ((0.0, s.inst0), (1.0, s.inst1)):
            got = s.trace(rays, any_hit, times=np.full(rays.shape[0], t, F))
            # the same node buffer on both sides: another tree has other boxes, another near / far order and another any-hit answer
            want = nm.trace(s.refit["nodes"], s.root, _records_of(s, inst), s.pool, rays, any_hit)
            assert _same(got, want), (name, any_hit, t)
            assert {k: got[5][k] for k in nm.COUNTERS} == want[5], (name, any_hit, t)
            assert got[5]["numSingular"] == 0 and 0 < got[5]["numMovingEntries"] <= got[5]["numInstanceEntries"]


# ---- 2. interior --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_inside_the_shutter_the_rule_is_the_static_spec_over_the_posed_scene(name):
    s, rays, sc = mc.named(name), mc.cpu_rays(), isc.scene(name)
    for tau in mc.INTERIOR:
        got = s.trace(rays, False, time=tau)
        tf = mo.lerp(s.inst0["objectToWorld"], s.inst1["objectToWorld"], F(tau))
        posed = ni.instances(tf, sc["blas"])
        tb = ni.tlas_build(s.pool["nodes"], s.pool["ranges"], posed)            # its own freshly built TLAS
        want = ni.trace(tb["nodes"], tb["root_link"], tb["records"], s.pool, rays, False)
        for k, what in ((0, "id"), (1, "t"), (4, "instance")):
            bad = np.flatnonzero(np.asarray(got[k]).view(np.uint32) != np.asarray(want[k]).view(np.uint32))
            assert bad.size == 0, (name, tau, what, bad.size, int(bad[0]))
        hit, _ = isc.brute_force(isc.flatten(dict(sc, transforms=tf))[0], rays)
        assert int(((got[0] != -1) != hit).sum()) == 0, (name, tau)
        assert (got[0] != -1).any()


# ---- 3. the refit rule --------------------------------------------------------------------------------------------------------------------
def _contains(outer_lo, outer_hi, lo, hi):
    f = np_hlbvh.f2i
    return (f(outer_lo) <= f(lo)).all() and (f(outer_hi) >= f(hi)).all()


def _child_box(nf, s, k):
    b = nf[s, tr.BOX_WORDS[k]]
    return b[tr.LO], b[tr.HI]


@pytest.mark.parametrize("name", mc.SCENES + ["big"])
def test_refit_rule(name):
    s = mc.big() if name == "big" else mc.named(name)
    b = s.built
    # key 1 == key 0: np_tlas_refit's bytes, and no word 15
    same = mo.motion_refit(b["nodes"], s.root, b["records"], s.pool["nodes"], s.pool["ranges"], s.inst0, s.inst0)
    plain = tr.refit(b["nodes"], s.root, b["records"], s.pool["nodes"], s.pool["ranges"], s.inst0)
    assert same["nodes"].tobytes() == plain["nodes"].tobytes() and same["records"].tobytes() == plain["records"].tobytes()
    assert not same["records"][:, 15].any() and same["stats"]["numMoving"] == 0
    assert same["scene_box"].tobytes() == plain["scene_box"].tobytes()
    r = s.refit
    mv = mo.moving(s.inst0, s.inst1)
    assert np.array_equal(r["records"][:, 15], mv.astype(np.uint32)) and np.array_equal(r["records"][:, :15], plain["records"][:, :15])
    assert np.array_equal(r["nodes"][:, 12:], b["nodes"][:, 12:])
    nf = r["nodes"].view(F)
    for slot in range(s.n - 1):
        for k in (0, 1):
            lo, hi = _child_box(nf, slot, k)
            c = int(r["nodes"][slot, 12 + k])
            if c < 0:
                i = ~c
                for inst in (s.inst0, s.inst1) if mv[i] else (s.inst0,):
                    klo, khi = ni.instance_box(s.pool["nodes"], s.pool["ranges"][int(s.inst0["blas"][i])], inst["objectToWorld"][i])
                    assert _contains(lo, hi, klo, khi), (name, slot, k)
                if not mv[i]:
                    assert nf[slot, tr.BOX_WORDS[k]].tobytes() == plain["nodes"].view(F)[slot, tr.BOX_WORDS[k]].tobytes()
            else:
                for kk in (0, 1):
                    assert _contains(lo, hi, *_child_box(nf, c // 64, kk)), (name, slot, k)
    keys = r["motion_keys"]
    assert keys.shape == (s.n, 32) and keys.dtype == np.uint32
    assert keys[:, 0:12].tobytes() == np.ascontiguousarray(s.inst0["objectToWorld"]).tobytes()
    assert keys[:, 16:28].tobytes() == np.ascontiguousarray(s.inst1["objectToWorld"]).tobytes()
    assert not keys[:, 12:16].any() and not keys[:, 28:32].any()


# ---- 4. the rule's corners, on two instances of the one-triangle BLAS ---------------------------------------------------------------------
def _identity_and_its_negation():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    return a, b.reshape(12)


def test_an_exactly_singular_pose_is_popped_and_counted():
    a, b = _identity_and_its_negation()
    s, rays = mc.two_of_one(a, b), mc.one_rays()
    m = mo.lerp(a, b, F(0.5))
    assert not m[[0, 1, 2, 4, 5, 6, 8, 9, 10]].any()                        # M is exactly zero in its linear part
    for any_hit in (False, True):
        rid, rt, ru, rv, rinst, c = s.trace(rays, any_hit, time=0.5)
        assert c["numSingular"] > 0 and c["numMovingEntries"] == 0 and c["numInstancesMasked"] == 0
        assert (rinst == 1).any() and not (rinst == 0).any()                # the ray can still hit the other instance
        # nothing else touched: the records are those of the scene without instance 0
        alone = nm.trace(s.refit["nodes"], s.root, s.refit["records"], s.pool, rays, any_hit, inst_masks=np.array([0, 1], np.uint32), ray_mask=1)
        assert _same((rid, rt, ru, rv, rinst), alone)
    assert s.trace(rays, False, time=0.25)[5]["numSingular"] == 0
    # a key entry outside the buffer reads as zeros, and a zero matrix is singular
    cut = mo.trace(s.refit["nodes"], s.root, s.refit["records"], s.refit["motion_keys"][:0], s.pool, rays, False, time=0.25)
    assert cut[5]["numSingular"] > 0 and cut[5]["numMovingEntries"] == 0


def test_a_key_pair_that_differs_only_in_the_sign_of_a_zero_keeps_its_signs():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy()
    b[1] = F(-0.0)
    assert a[1] == 0 and b.view(np.uint32)[1] == 0x80000000
    s, rays = mc.two_of_one(a, b), mc.one_rays()
    assert mo.moving(s.inst0, s.inst1).tolist() == [True, False] and s.refit["records"][:, 15].tolist() == [1, 0]
    assert mo.lerp(a, b, F(0)).tobytes() == a.tobytes() and mo.lerp(a, b, F(1)).tobytes() == b.tobytes()
    mid = mo.lerp(a, b, F(0.5))
    assert mid.view(np.uint32)[1] == 0 and np.delete(mid, 1).tobytes() == np.delete(a, 1).tobytes()   # a component that stays never changes
    inst1 = ni.instances(np.stack([b, s.inst0["objectToWorld"][1]]), [0, 0])
    for t, inst in ((0.0, s.inst0), (1.0, inst1)):
        assert _same(s.trace(rays, False, time=t), nm.trace(s.refit["nodes"], s.root, _records_of(s, inst), s.pool, rays, False))


def _moved_pair():
    a = isc.transform(isc.rotation(np.random.default_rng(5)), (1.0, 0.7, 1.3), (0.1, -0.2, 0.0))
    return a, mc.key1_transforms(a[None], seed=8, every=True)[0]


def test_corner_times():
    a, b = _moved_pair()
    s, rays = mc.two_of_one(a, b), mc.one_rays()
    assert mo.clamp_time(mc.CORNER_TIMES).view(np.uint32).tolist() == [0, 0x3F800000, 0, 1, 0x3F7FFFFF]
    at = lambda t: s.trace(rays, False, time=t)                             # noqa: E731
    assert _same(at(-1.0), at(0.0)) and _same(at(2.0), at(1.0)) and _same(at(float("nan")), at(0.0))
    assert at(-1.0)[5] == at(0.0)[5] and at(float("nan"))[5] == at(0.0)[5]
    # next to the exact ends the lerp is the formula, checked against binary64 (a product of two binary32 is exact there)
    for t in mc.CORNER_TIMES[3:]:
        u = F(1) - t
        want = np.array([F(float(F(float(u) * float(x))) + float(F(float(t) * float(y)))) for x, y in zip(a, b)], F)
        assert mo.lerp(a, b, t).tobytes() == want.tobytes()
        got = at(float(t))
        w2o, ok = mo.invert_many(want)
        assert ok.all() and w2o[0].tobytes() == ni.invert(want).tobytes()
        rec1 = s.refit["records"].copy()
        rec1[0, :12] = w2o[0].view(np.uint32)
        assert _same(got, nm.trace(s.refit["nodes"], s.root, rec1, s.pool, rays, False))
    assert mo.lerp(a, b, mc.CORNER_TIMES[4]).tobytes() != b.tobytes()


def test_per_ray_times_against_the_scalar_time():
    a, b = _moved_pair()
    s, rays = mc.two_of_one(a, b), mc.one_rays()
    n = rays.shape[0]
    for t in (0.0, 0.3, 1.0):
        assert _same(s.trace(rays, False, times=np.full(n, t, F)), s.trace(rays, False, time=t))
    times = np.resize(np.concatenate([mc.CORNER_TIMES, np.array([0.3, 0.5, 0.9], F)]), n).astype(F)
    got = s.trace(rays, False, times=times)
    moving_entries = 0
    for t in np.unique(times.view(np.uint32)).view(F):
        pick = times.view(np.uint32) == t.view(np.uint32)
        want = s.trace(rays[pick], False, time=float(t))
        assert _same([np.asarray(x)[pick] for x in got[:5]], want), t
        moving_entries += want[5]["numMovingEntries"]
    assert got[5]["numMovingEntries"] == moving_entries > 0
    assert mo.algorithmic_bytes(got[5], ray_times=True) == nm.algorithmic_bytes({k: got[5][k] for k in nm.COUNTERS}) + 128 * moving_entries + 4 * n


def test_masks_together_with_motion():
    """A refused moving instance reads no key and counts as masked only."""
    a, b = _moved_pair()
    s, rays = mc.two_of_one(a, b), mc.one_rays()
    M = np.array([2, 1], np.uint32)                                         # the moving instance is hidden from ray mask 1
    poison = s.refit["motion_keys"].copy()
    poison[0] = 0x7FC00000                                                  # NaN keys: were they read, the step would be singular
    got = mo.trace(s.refit["nodes"], s.root, s.refit["records"], poison, s.pool, rays, False, time=0.5, inst_masks=M, ray_mask=1)
    want = nm.trace(s.refit["nodes"], s.root, s.refit["records"], s.pool, rays, False, inst_masks=M, ray_mask=1)
    assert _same(got, want) and {k: got[5][k] for k in nm.COUNTERS} == want[5]
    assert got[5]["numInstancesMasked"] > 0 and got[5]["numMovingEntries"] == got[5]["numSingular"] == 0
    seen = mo.trace(s.refit["nodes"], s.root, s.refit["records"], poison, s.pool, rays, False, time=0.5, inst_masks=M, ray_mask=2)
    assert seen[5]["numSingular"] > 0                                       # visible, the poisoned keys are read


# ---- 5. the C-ABI without a device --------------------------------------------------------------------------------------------------------
NAMES = ("ntr_tlas_motion_refit", "ntr_tlas_motion_refit_scratch_bytes", "ntr_trace_instanced_motion", "ntr_trace_instanced_motion_stats")
GOOD = {k: v for k, v in binary.GOOD.items() if k != "d_flags"}
MOTION = dict(d_motion_keys=FAKE, motion_keys_bytes=640)


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols_and_struct_sizes():
    with open(os.path.join(ROOT, "include", "ntrace_amd.h")) as f:
        header = f.read()
    bound = {s[0] for s in _capi.SYMBOLS}
    for name in NAMES:
        assert re.search(r"NTR_API int\s+%s\(" % name, header), name
        assert name in bound and getattr(nt.lib(), name) is not None
    assert (C.sizeof(nt.InstanceMotion), C.sizeof(nt.InstancedMotionStats), C.sizeof(nt.TlasMotionRefitResult)) == (32, 16, 56)
    assert C.sizeof(nt.TlasMotionRefitResult) == C.sizeof(nt.TlasRefitResult) + 8
    assert [f[0] for f in nt.InstanceMotion._fields_] == ["d_motionKeys", "motionKeysBytes", "d_rayTimes", "time", "pad"]
    assert nt.lib().ntr_tlas_motion_refit_scratch_bytes(None) == -1 and b"ntr_tlas_motion_refit_scratch_bytes" in nt.lib().ntr_last_error()
    if not _has_device():
        assert nt.lib().ntr_lbvh_release_workspace() in (0, -2, -3)


def _refusal(name, kw):
    try:
        getattr(nt, name)(**kw)
    except nt.NtrError as e:
        return [e.code, str(e)]
    return [0, ""]


@pytest.mark.parametrize("name,like", [("trace_instanced_motion", "trace_instanced_masked"), ("trace_instanced_motion_stats", "trace_instanced_stats")])
def test_trace_refusals_new_and_shared(name, like):
    params = inspect.signature(getattr(nt, name)).parameters
    good = {k: v for k, v in GOOD.items() if k in params}
    motion = lambda **kw: nt.InstanceMotion(**dict(MOTION, **kw))           # noqa: E731
    fn = "ntr_" + name
    # the new refusals, in their words and their order
    new = [(dict(d_ray_times=FAKE + 2), "%s: the ray times must be 4-byte aligned"),
           (dict(d_motion_keys=0), "%s: the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
           (dict(d_motion_keys=FAKE + 8), "%s: the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned"),
           (dict(motion_keys_bytes=639), "%s: motionKeysBytes below 128 * numInstances")]
    for change, text in new:
        assert _refusal(name, dict(good, motion=motion(**change))) == [-1, "ntrace_amd error -1: " + text % fn], change
    for (c1, t1), (c2, _) in zip(new, new[1:]):
        if set(c1) != set(c2):
            assert _refusal(name, dict(good, motion=motion(**dict(c1, **c2)))) == [-1, "ntrace_amd error -1: " + t1 % fn], (c1, c2)
    # a shared check fails before a new one, and the shared ones come in the recorded words and order (the golden of
    # test_two_level_refusals_cpu.py for the masked entry point, under this function's name)
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
    # with motion == NULL the call is the masked one
    for label, kw in rec.cases(like)[:3]:
        assert _refusal(name, dict(kw, motion=None)) == golden[label], label


def test_zero_rays_null_stats_and_no_device():
    L = nt.lib()
    st, ms = nt.InstancedTraceStats(), nt.InstancedMotionStats()
    mot = nt.InstanceMotion(**MOTION)
    args = (FAKE, FAKE, FAKE, FAKE, 256, 0, FAKE, 5, FAKE, 704, FAKE, 1680, FAKE, None)
    for m in (C.byref(mot), None):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(ms), 0xFF, C.sizeof(ms))
        assert L.ntr_trace_instanced_motion_stats(0, 0, *args, m, C.byref(st), C.byref(ms), None) == 0
        assert bytes(st) == bytes(64) and bytes(ms) == bytes(16)
        sec = C.c_float(7.0)
        assert L.ntr_trace_instanced_motion(0, 0, *args, m, C.byref(sec), None) == 0 and sec.value == 0.0
    for a, b in ((None, C.byref(ms)), (C.byref(st), None), (None, None)):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(ms), 0xFF, C.sizeof(ms))
        assert L.ntr_trace_instanced_motion_stats(-1, 0, *args, C.byref(mot), a, b, None) == -1
        assert L.ntr_last_error() == b"ntr_trace_instanced_motion_stats: null stats"
        assert (a is None or bytes(st) == bytes(64)) and (b is None or bytes(ms) == bytes(16))
    if not _has_device():
        good = {k: v for k, v in GOOD.items()}
        for name in ("trace_instanced_motion", "trace_instanced_motion_stats"):
            got = _refusal(name, dict(good, motion=mot))
            assert got[0] in (-2, -3), got


def test_motion_refit_argument_errors_are_decided_before_device_work():
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    good = dict(num_instances=5, d_instances0=FAKE, d_instances1=FAKE, ranges=ranges, d_pool_nodes=FAKE, pool_nodes_bytes=704, d_tlas_nodes=FAKE,
                tlas_nodes_bytes=256, root_link=0, d_records=FAKE, records_cap=320, d_motion_keys=FAKE, motion_keys_cap=640)
    bad = [(dict(d_instances1=0), "bad arguments"), (dict(d_motion_keys=0), "bad arguments"), (dict(num_instances=0), "bad arguments"),
           (dict(tlas_nodes_bytes=320), "tlasNodesBytes must be 64 * (numInstances - 1)"), (dict(root_link=-1), "rootLink must be 0"),
           (dict(records_cap=319), "recordsCapacity below 64 * numInstances"), (dict(motion_keys_cap=639), "motionKeysCapacity below 128 * numInstances"),
           (dict(d_instances1=FAKE + 8), "the buffers must be 16-byte aligned"), (dict(d_motion_keys=FAKE + 4), "the buffers must be 16-byte aligned"),
           (dict(d_instances0=FAKE + 8), "the buffers must be 16-byte aligned"), (dict(pool_nodes_bytes=700), "poolNodesBytes must be a multiple of 64"),
           (dict(ranges=[(0, 640, 0, 1600), (640, 128, 1600, 80)]), "BLAS 1")]
    for blocking in (True, False):
        for change, text in bad:
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_motion_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: ntr_tlas_motion_refit: ") and text in str(e.value), (change, str(e.value))
            if blocking:
                assert bytes(e.value.result) == bytes(56)
    if not _has_device():
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_motion_refit(**good, blocking=blocking)
            assert e.value.code in (-2, -3)
        assert nt.tlas_motion_refit_scratch_bytes() == 0
