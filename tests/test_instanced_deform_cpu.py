"""Deforming BLASes in the motion-blurred two-level trace without a device: the numpy rule (tests/np_instanced_deform.py) against the
specs it extends -- its consequences a to d; the count that shows why the leaf box unites four boxes and not two; the rule's corners on
two instances of the one-triangle BLAS; and the C-ABI: symbols, struct sizes, every new refusal in its words, the shared refusals in
the recorded order, zero rays, no device."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import _capi

import bvh_motion_cases as bc
import instanced_deform_cases as dc
import instanced_motion_cases as mc
import instanced_scenes as isc
import np_bvh_motion as bm
import np_bvh_refit as rf
import np_hlbvh
import np_instanced as ni
import np_instanced_deform as nd
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


# ---- a. nothing deforming -------------------------------------------------------------------------------------------------------------------
def test_a_with_no_deforming_blas_the_rule_is_the_motion_rule():
    s, rays = dc.named("three_static"), dc.rays_of("cpu")
    want = mo.motion_refit(s.built["nodes"], s.root, s.built["records"], s.pool["nodes"], s.ranges, s.inst0, s.inst1)
    for k in ("nodes", "records", "motion_keys", "scene_box"):
        assert s.refit[k].tobytes() == want[k].tobytes(), k
    assert s.refit["stats"] == dict(want["stats"], numDeforming=0) and s.refit["err_bits"] == want["err_bits"]
    assert (s.pool["nodes1"] == 0xCD).all() and (s.pool["vrows0"] == 0xCD).all()          # never read: any read would show
    n = rays.shape[0]
    for any_hit in (False, True):
        for kw in (dict(time=0.5), dict(times=bc.hashed_times(n))):
            got = s.trace(rays, any_hit, **kw)
            ref = mo.trace(s.refit["nodes"], s.root, s.refit["records"], s.refit["motion_keys"], s.pool, rays, any_hit, **kw)
            assert _same(got, ref) and {k: got[5][k] for k in mo.COUNTERS} == ref[5]
            assert got[5]["numDeformEntries"] == got[5]["numDeformInnerVisits"] == got[5]["numDeformTriTests"] == 0
            assert nd.algorithmic_bytes(got[5], ray_times="times" in kw) == mo.algorithmic_bytes(ref[5], ray_times="times" in kw)


# ---- b. one identity instance ---------------------------------------------------------------------------------------------------------------
def test_b_one_identity_instance_of_a_deforming_blas_is_the_single_level_rule():
    inst = ni.instances(ni.IDENTITY[None], [0])
    s = dc.DeformScene(["soup1000"], inst, inst, {0: 0.3})
    assert s.refit["records"][0, 15] == nd.DEFORMING and s.refit["stats"]["numMoving"] == 0
    rays = np.concatenate([dc.rays_of("cpu")[:2048], isc.finite_edge_rays()])
    times = bc.hashed_times(rays.shape[0])
    m, tidx = s.blas_slices(0)
    for any_hit in (False, True):
        got = s.trace(rays, any_hit, times=times)
        ref = bm.trace(m["nodes0"], m["nodes1"], m["vrows0"], m["vrows1"], tidx, rays, any_hit, times, return_stats=True)
        assert _same(got, ref, words=4), any_hit
        c = got[5]
        assert {k: c[k] for k in bm.COUNTERS} == ref[4]
        assert (c["numDeformInnerVisits"], c["numDeformTriTests"]) == (c["numInnerVisits"], c["numTriTests"])
        assert np.array_equal(got[4], np.where(got[0] != -1, 0, -1))
        # the bytes: 64 per visit and 48 per test on top of the motion formula, np_bvh_motion's 128 and 96 in all
        assert nd.algorithmic_bytes(c, ray_times=True) - mo.algorithmic_bytes(c, ray_times=True) == 64 * c["numInnerVisits"] + 48 * c["numTriTests"]


# ---- c. the shutter's two ends --------------------------------------------------------------------------------------------------------------
def _key_pool(s, key):
    """The pool refitted to one key: key 1's has nodes1's boxes with nodes' links and the Woop rows of np_bvh_refit.refit(pos1)"""
    if key == 0:
        return s.pool
    nodes, woop = s.pool["nodes"].copy(), s.pool["woop"].copy()
    for b, mesh in enumerate(s.meshes):
        if mesh is None:
            continue
        n_off, n_bytes, w_off, w_bytes = s.ranges[b]
        m, tidx = s.blas_slices(b)
        assert np.array_equal(m["nodes1"][:, 12:], m["nodes0"][:, 12:])
        nodes[n_off:n_off + n_bytes] = m["nodes1"].view(np.uint8).reshape(-1)
        woop[w_off:w_off + w_bytes] = rf.refit(m["nodes0"], m["woop"], tidx, mesh[0], mesh[2], 0.0)["woop"]
    return dict(nodes=nodes, woop=woop, tri_index=s.pool["tri_index"], ranges=s.ranges)


@pytest.mark.parametrize("name", dc.SCENES + ["collapse"])
def test_c_at_the_shutters_ends_the_rule_is_the_masked_spec_over_that_keys_pool_and_records(name):
    s, rays = dc.named(name), dc.rays_of("cpu")
    for any_hit in (False, True):
        for t, inst in ((0.0, s.inst0), (1.0, s.inst1)):
            got = s.trace(rays, any_hit, times=np.full(rays.shape[0], t, F))
            records = np.stack([tr.record_of(inst[i], s.ranges) for i in range(s.n)])
            want = nm.trace(s.refit["nodes"], s.root, records, _key_pool(s, int(t)), rays, any_hit)
            assert _same(got, want), (name, any_hit, t)
            assert {k: got[5][k] for k in nm.COUNTERS} == want[5], (name, any_hit, t)
            assert got[5]["numDeformInnerVisits"] > 0 and (got[5]["numDeformTriTests"] > 0 or (name, t) == ("collapse", 1.0))   # (a point)


# ---- d. inside the shutter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SCENES)
def test_d_inside_the_shutter_the_rule_is_the_static_spec_over_the_posed_scene(name):
    s, rays = dc.named(name), dc.rays_of("cpu")
    for tau in dc.INTERIOR:
        got = s.trace(rays, False, time=tau)
        pool, posed, meshes = dc.posed_scene(s, tau)
        tb = ni.tlas_build(pool["nodes"], pool["ranges"], posed)                 # its own freshly built TLAS
        want = ni.trace(tb["nodes"], tb["root_link"], tb["records"], pool, rays, False)
        for k, what in ((0, "id"), (1, "t"), (4, "instance")):
            bad = np.flatnonzero(np.asarray(got[k]).view(np.uint32) != np.asarray(want[k]).view(np.uint32))
            assert bad.size == 0, (name, tau, what, bad.size, int(bad[0]))
        hit, _ = isc.brute_force(dc.world_triangles(posed, meshes), rays)
        assert int(((got[0] != -1) != hit).sum()) == 0, (name, tau)
        assert (got[0] != -1).any() and got[5]["numDeformTriTests"] > 0


# ---- the leaf box: four boxes, not two ------------------------------------------------------------------------------------------------------
def _outside(name, how, pairs):
    """Posed instance boxes that are not inside the swept leaf box, over every instance of the scene (all moving, every BLAS deformed by
    `how`) and five times.  pairs: None for the rule's K x J, or the two-box union {(0, 0), (1, 1)}."""
    sc = isc.scene(name)
    s = dc.scene_of(name, {b: how for b in range(len(sc["names"]))}, every=True)
    f = np_hlbvh.f2i
    out = total = 0
    for tau in (0.03, 0.25, 0.5, 0.8125, 0.97):
        t = F(tau)
        posed_nodes = s.pool["nodes"].copy()
        for n_off, _, _, _ in s.ranges:
            w0, w1 = s.pool["nodes"][n_off:n_off + 48].view(F), s.pool["nodes1"][n_off:n_off + 48].view(F)
            posed_nodes[n_off:n_off + 48] = bm.deform_lerp(w0, w1, t).view(np.uint8)
        tf = mo.lerp(s.inst0["objectToWorld"], s.inst1["objectToWorld"], t)
        for i in range(s.n):
            r = s.ranges[int(s.inst0["blas"][i])]
            box = nd.sweep_box(s.pool["nodes"], s.pool["nodes1"], r, s.inst0["objectToWorld"][i], s.inst1["objectToWorld"][i], True, True, pairs)
            lo, hi = ni.instance_box(posed_nodes, r, tf[i])
            total += 1
            out += not ((f(box[rf.LO]) <= f(lo)).all() and (f(box[rf.HI]) >= f(hi)).all())
    return out, total


def test_the_swept_leaf_box_needs_all_four_boxes():
    four = [_outside(name, how, None) for name in ("three", "mirror", "grid") for how in (0.02, 0.3)]
    assert sum(o for o, _ in four) == 0 and sum(t for _, t in four) == 690
    two = {how: _outside("grid", how, {(0, 0), (1, 1)}) for how in (0.02, 0.3)}
    print("two-box union, posed instance boxes outside: %r" % two)
    assert all(total == 320 and out > 0 for out, total in two.values())


def test_refit_rule_bits_and_counts():
    for name in dc.SCENES + ["big"]:
        s = dc.big() if name == "big" else dc.named(name)
        r = s.refit
        mv = mo.moving(s.inst0, s.inst1)
        df = s.pool["deforming"][s.inst0["blas"]] != 0
        assert np.array_equal(r["records"][:, 15], mv.astype(np.uint32) | (df.astype(np.uint32) << 1)) and r["records"][:, 15].max() <= 3
        assert r["stats"]["numMoving"] == int(mv.sum()) and r["stats"]["numDeforming"] == int(df.sum()) > 0
        plain = mo.motion_refit(s.built["nodes"], s.root, s.built["records"], s.pool["nodes"], s.ranges, s.inst0, s.inst1)
        assert r["motion_keys"].tobytes() == plain["motion_keys"].tobytes() and np.array_equal(r["records"][:, :15], plain["records"][:, :15])
        # a leaf box of a static BLAS's instance is the motion refit's; every box contains the motion refit's
        f = np_hlbvh.f2i
        nf, pf = r["nodes"].view(F), plain["nodes"].view(F)
        for slot in range(s.n - 1):
            for k in (0, 1):
                a, b = nf[slot, tr.BOX_WORDS[k]], pf[slot, tr.BOX_WORDS[k]]
                assert (f(a[rf.LO]) <= f(b[rf.LO])).all() and (f(a[rf.HI]) >= f(b[rf.HI])).all()
                c = int(r["nodes"][slot, 12 + k])
                if c < 0 and not df[~c]:
                    assert a.tobytes() == b.tobytes()


# ---- the rule's corners, on two instances of the one-triangle BLAS --------------------------------------------------------------------------
def _moved_pair():
    a = isc.transform(isc.rotation(np.random.default_rng(5)), (1.0, 0.7, 1.3), (0.1, -0.2, 0.0))
    return a, mc.key1_transforms(a[None], seed=8, every=True)[0]


def _one_keys(x0=0.0):
    """The one-triangle mesh with vertex 0's x given, and a key 1 that moves every vertex a little"""
    pos0 = np.array([(x0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], F)
    pos1 = (pos0 + np.array([(0.0, 0.05, 0.1), (0.1, 0.0, -0.05), (-0.05, 0.1, 0.0)], F)).astype(F)
    pos1[0, 0] = pos0[0, 0]
    return pos0, pos1


def test_a_vertex_x_of_minus_zero_is_not_a_terminator():
    ident = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    rays = mc.one_rays()
    minus, plus = dc.two_of_one(ident, ident, _one_keys(F(-0.0))), dc.two_of_one(ident, ident, _one_keys(F(0.0)))
    row = minus.pool["vrows0"].view(np.uint32).reshape(-1, 4)
    at = np.flatnonzero(row[:, 0] == 0x80000000)                                # the one row whose x word is the terminator's word
    assert at.size == 1 and row[at[0], 3] == 0 and row[at[0] + 3].tolist() == [0, 0, 0, 0x80000000]
    for t in (0.0, 0.5, 1.0):
        a, b = minus.trace(rays, False, time=t), plus.trace(rays, False, time=t)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])
        assert a[5] == b[5] and a[5]["numDeformTriTests"] > 0 and (a[0] != -1).any() and (a[4] == 0).any()


def test_corner_times_and_per_ray_times():
    a, b = _moved_pair()
    s, rays = dc.two_of_one(a, b), mc.one_rays()
    n = rays.shape[0]
    at = lambda t: s.trace(rays, False, time=t)                                # noqa: E731
    assert _same(at(-1.0), at(0.0)) and _same(at(2.0), at(1.0)) and _same(at(float("nan")), at(0.0))
    assert at(-1.0)[5] == at(0.0)[5] and at(float("nan"))[5] == at(0.0)[5] and at(2.0)[5] == at(1.0)[5]
    for t in (0.0, 0.3, 1.0):
        assert _same(s.trace(rays, False, times=np.full(n, t, F)), s.trace(rays, False, time=t))
    times = np.resize(np.concatenate([dc.CORNER_TIMES, np.array([0.3, 0.5, 0.9], F)]), n).astype(F)
    got = s.trace(rays, False, times=times)
    tests = 0
    for t in np.unique(times.view(np.uint32)).view(F):
        pick = times.view(np.uint32) == t.view(np.uint32)
        want = s.trace(rays[pick], False, time=float(t))
        assert _same([np.asarray(x)[pick] for x in got[:5]], want), t
        tests += want[5]["numDeformTriTests"]
    assert got[5]["numDeformTriTests"] == tests > 0


def test_masks_together_with_deform():
    """A refused instance of a deforming BLAS reads no key and nothing of the pool's key 1, and counts as masked only."""
    a, b = _moved_pair()
    s, rays = dc.two_of_one(a, b), mc.one_rays()
    M = np.array([2, 2], np.uint32)                                            # both hidden from ray mask 1
    got = s.trace(rays, False, time=0.5, inst_masks=M, ray_mask=1)
    c = got[5]
    assert c["numInstancesMasked"] > 0 and c["numInstanceEntries"] == c["numDeformEntries"] == c["numDeformInnerVisits"] == 0
    assert (got[0] == -1).all()
    M = np.array([2, 1], np.uint32)                                            # the moving instance is hidden
    got = s.trace(rays, False, time=0.5, inst_masks=M, ray_mask=1)
    assert got[5]["numMovingEntries"] == 0 and got[5]["numDeformEntries"] == got[5]["numInstanceEntries"] > 0 and not (got[4] == 0).any()


def test_a_singular_pose_is_popped_before_any_deform_read():
    a = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    b = a.copy().reshape(3, 4)
    b[:, :3] = -b[:, :3]
    s, rays = dc.two_of_one(a, b.reshape(12)), mc.one_rays()
    for any_hit in (False, True):
        got = s.trace(rays, any_hit, time=0.5)
        assert got[5]["numSingular"] > 0 and got[5]["numMovingEntries"] == 0 and not (got[4] == 0).any() and (got[4] == 1).any()
        # nothing else touched: the records and every counter but the singular steps are those of the scene without instance 0
        alone = s.trace(rays, any_hit, time=0.5, inst_masks=np.array([0, 1], np.uint32), ray_mask=1)
        assert _same(got, alone)
        for k in ("numInstanceEntries", "numDeformEntries", "numDeformInnerVisits", "numDeformTriTests", "numInnerVisits", "numTriTests"):
            assert got[5][k] == alone[5][k], k
        assert alone[5]["numInstancesMasked"] == got[5]["numSingular"]


def test_deform_lerps_ends_and_the_ulp_inside_the_shutter():
    """deform_lerp has no same-word shortcut: a vertex of a deforming BLAS that does not move may wobble by an ulp inside the shutter;
    at the two ends it is the key's word, and a static BLAS's vertex never changes."""
    x = np.random.default_rng(3).normal(size=4096).astype(F)
    assert bm.deform_lerp(x, x, F(0)).tobytes() == x.tobytes() and bm.deform_lerp(x, x, F(1)).tobytes() == x.tobytes()
    assert (bm.deform_lerp(x, x, F(0.37)).view(np.uint32) != x.view(np.uint32)).any()
    ident = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 0.0))
    rays = mc.one_rays()
    pos = isc.blas("one")[1]
    still, static = dc.two_of_one(ident, ident, (pos, pos)), dc.two_of_one(ident, ident, None)
    assert still.refit["records"][:, 15].tolist() == [2, 2] and static.refit["records"][:, 15].tolist() == [0, 0]
    for t in (0.0, 1.0):
        assert _same(still.trace(rays, False, time=t), static.trace(rays, False, time=t))
    assert _same(static.trace(rays, False, time=0.37), static.trace(rays, False, time=0.0))
    a, b = still.trace(rays, False, time=0.37), static.trace(rays, False, time=0.37)
    assert np.array_equal(a[0], b[0]) and np.allclose(a[1], b[1], rtol=1e-5)    # the same hits, t within the wobble


# ---- the C-ABI without a device -------------------------------------------------------------------------------------------------------------
NAMES = ("ntr_tlas_deform_refit", "ntr_tlas_deform_refit_scratch_bytes", "ntr_trace_instanced_deform", "ntr_trace_instanced_deform_stats")
GOOD = {k: v for k, v in binary.GOOD.items() if k != "d_flags"}
MOTION = dict(d_motion_keys=FAKE, motion_keys_bytes=640)
D1, D2, D3 = 0x100000, 0x200000, 0x300000                                      # apart from every other buffer of GOOD
DEFORM = dict(d_pool_nodes1=D1, d_pool_vert_rows0=D2, d_pool_vert_rows1=D3)


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
    assert (C.sizeof(nt.InstanceDeform), C.sizeof(nt.InstancedDeformStats), C.sizeof(nt.TlasDeformRefitResult)) == (24, 24, 64)
    assert C.sizeof(nt.TlasDeformRefitResult) == C.sizeof(nt.TlasMotionRefitResult) + 8
    assert [f[0] for f in nt.InstanceDeform._fields_] == ["d_poolNodes1", "d_poolVertRows0", "d_poolVertRows1"]
    assert nt.lib().ntr_tlas_deform_refit_scratch_bytes(None) == -1 and b"ntr_tlas_deform_refit_scratch_bytes" in nt.lib().ntr_last_error()


def _refusal(name, kw):
    try:
        getattr(nt, name)(**kw)
    except nt.NtrError as e:
        return [e.code, str(e)]
    return [0, ""]


@pytest.mark.parametrize("name,like", [("trace_instanced_deform", "trace_instanced_masked"), ("trace_instanced_deform_stats", "trace_instanced_stats")])
def test_trace_refusals_new_and_shared(name, like):
    params = inspect.signature(getattr(nt, name)).parameters
    good = {k: v for k, v in GOOD.items() if k in params}
    motion = lambda **kw: nt.InstanceMotion(**dict(MOTION, **kw))              # noqa: E731
    deform = lambda **kw: nt.InstanceDeform(**dict(DEFORM, **kw))              # noqa: E731
    fn = "ntr_" + name
    head = "ntrace_amd error -1: " + fn + ": "
    # the new refusals, in their words and their order
    new = [(dict(d_pool_nodes1=0), "null d_poolNodes1"), (dict(d_pool_vert_rows0=0), "null d_poolVertRows0"),
           (dict(d_pool_vert_rows1=0), "null d_poolVertRows1"),
           (dict(d_pool_nodes1=D1 + 8), "d_poolNodes1, d_poolVertRows0 and d_poolVertRows1 must be 16-byte aligned"),
           (dict(d_pool_vert_rows1=D3 + 4), "d_poolNodes1, d_poolVertRows0 and d_poolVertRows1 must be 16-byte aligned"),
           (dict(d_pool_nodes1=FAKE), "d_poolNodes1 overlaps d_rays"), (dict(d_pool_vert_rows0=FAKE + 1024), "d_poolVertRows0 overlaps d_rays"),
           (dict(d_pool_nodes1=D2 - 688), "d_poolNodes1 overlaps d_poolVertRows0"),
           (dict(d_pool_vert_rows1=D2 + 1664), "d_poolVertRows0 overlaps d_poolVertRows1")]
    for change, text in new:
        assert _refusal(name, dict(good, motion=motion(), deform=deform(**change))) == [-1, head + text], change
    for (c1, t1), (c2, _) in zip(new, new[1:]):
        if set(c1) != set(c2):
            assert _refusal(name, dict(good, motion=motion(), deform=deform(**dict(c2, **c1)))) == [-1, head + t1], (c1, c2)
    # a null motion with a deform, and motion's refusals before deform's
    assert _refusal(name, dict(good, motion=None, deform=deform())) == [-1, head + "null motion"]
    assert _refusal(name, dict(good, motion=motion(d_motion_keys=0), deform=deform(d_pool_nodes1=0)))[1].endswith("must be given and 16-byte aligned")
    # buffers that touch but do not overlap are taken
    if not _has_device():
        assert _refusal(name, dict(good, motion=motion(), deform=deform(d_pool_vert_rows1=D2 + 1680)))[0] in (-2, -3)
    # a shared check fails before a new one, and the shared ones come in the recorded words and order
    with open(rec.GOLDEN) as f:
        golden = json.load(f)[like]
    checked = 0
    for label, kw in rec.cases(like):
        want = golden[label]
        want = [want[0], want[1].replace("ntr_" + like, fn)]
        assert want[0] == -1
        assert _refusal(name, dict(kw, motion=motion(), deform=deform())) == want, label
        assert _refusal(name, dict(kw, motion=motion(d_motion_keys=0), deform=deform(d_pool_nodes1=0))) == want, label
        assert _refusal(name, dict(kw, motion=None, deform=deform())) == want, label
        checked += 1
    assert checked >= 26
    # with deform == NULL the call is the motion one
    mname = name.replace("deform", "motion")
    for label, kw in rec.cases(like)[:3]:
        assert _refusal(name, dict(kw, motion=motion(), deform=None)) == [-1, golden[label][1].replace("ntr_" + like, "ntr_" + mname)], label
    assert _refusal(name, dict(good, motion=motion(motion_keys_bytes=639), deform=None)) == [-1, "ntrace_amd error -1: ntr_%s: motionKeysBytes below 128 * numInstances" % mname]


def test_zero_rays_null_stats_and_no_device():
    L = nt.lib()
    st, ms, ds = nt.InstancedTraceStats(), nt.InstancedMotionStats(), nt.InstancedDeformStats()
    mot, dfm = nt.InstanceMotion(**MOTION), nt.InstanceDeform(**DEFORM)
    args = (FAKE, FAKE, FAKE, FAKE, 256, 0, FAKE, 5, FAKE, 704, FAKE, 1680, FAKE, None)
    outs = (st, ms, ds)
    for m, d in ((C.byref(mot), C.byref(dfm)), (C.byref(mot), None), (None, None), (None, C.byref(dfm))):
        for o in outs:
            C.memset(C.byref(o), 0xFF, C.sizeof(o))
        assert L.ntr_trace_instanced_deform_stats(0, 0, *args, m, d, C.byref(st), C.byref(ms), C.byref(ds), None) == 0
        assert bytes(st) == bytes(64) and bytes(ms) == bytes(16) and bytes(ds) == bytes(24)
        sec = C.c_float(7.0)
        assert L.ntr_trace_instanced_deform(0, 0, *args, m, d, C.byref(sec), None) == 0 and sec.value == 0.0
    for null in range(1, 8):
        ptrs = [None if null >> k & 1 else C.byref(o) for k, o in enumerate(outs)]
        for o in outs:
            C.memset(C.byref(o), 0xFF, C.sizeof(o))
        assert L.ntr_trace_instanced_deform_stats(-1, 0, *args, C.byref(mot), C.byref(dfm), *ptrs, None) == -1
        assert L.ntr_last_error() == b"ntr_trace_instanced_deform_stats: null stats"
        assert all(p is None or bytes(o) == bytes(C.sizeof(o)) for p, o in zip(ptrs, outs))
    if not _has_device():
        for name in ("trace_instanced_deform", "trace_instanced_deform_stats"):
            got = _refusal(name, dict(GOOD, motion=mot, deform=dfm))
            assert got[0] in (-2, -3), got


def test_deform_refit_argument_errors_are_decided_before_device_work():
    ranges = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
    good = dict(num_instances=5, d_instances0=FAKE, d_instances1=FAKE, ranges=ranges, d_pool_nodes=FAKE, d_pool_nodes1=D1, pool_nodes_bytes=704,
                d_blas_deforming=D2, d_tlas_nodes=FAKE, tlas_nodes_bytes=256, root_link=0, d_records=FAKE, records_cap=320, d_motion_keys=FAKE,
                motion_keys_cap=640)
    bad = [(dict(d_instances1=0), "bad arguments"), (dict(d_motion_keys=0), "bad arguments"), (dict(d_pool_nodes1=0), "bad arguments"),
           (dict(d_blas_deforming=0), "bad arguments"), (dict(num_instances=0), "bad arguments"),
           (dict(tlas_nodes_bytes=320), "tlasNodesBytes must be 64 * (numInstances - 1)"), (dict(root_link=-1), "rootLink must be 0"),
           (dict(records_cap=319), "recordsCapacity below 64 * numInstances"), (dict(motion_keys_cap=639), "motionKeysCapacity below 128 * numInstances"),
           (dict(d_blas_deforming=D2 + 2), "d_blasDeforming must be 4-byte aligned"), (dict(d_pool_nodes1=D1 + 8), "the buffers must be 16-byte aligned"),
           (dict(d_instances1=FAKE + 8), "the buffers must be 16-byte aligned"), (dict(pool_nodes_bytes=700), "poolNodesBytes must be a multiple of 64"),
           (dict(ranges=[(0, 640, 0, 1600), (640, 128, 1600, 80)]), "BLAS 1")]
    for blocking in (True, False):
        for change, text in bad:
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_deform_refit(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and str(e.value).startswith("ntrace_amd error -1: ntr_tlas_deform_refit: ") and text in str(e.value), (change, str(e.value))
            if blocking:
                assert bytes(e.value.result) == bytes(64)
    if not _has_device():
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.tlas_deform_refit(**good, blocking=blocking)
            assert e.value.code in (-2, -3)
        assert nt.tlas_deform_refit_scratch_bytes() == 0
