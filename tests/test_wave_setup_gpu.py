"""A per-ray wave's set-up and its triangle step on the GPU: the votes decide which loop a wave runs, never a record.

* ntr_selftest_ray_class: the integer form of the FAST path's admission test (ray_class, trace_lane.h) against the rule's float ranges, on
  every exponent of every component with the mantissas 0, 1 and 0x7FFFFF and both signs, and on random bit patterns, with and without
  NTR_BVH_NOTINY.  The same comparison is restated in numpy (no GPU), so the formula is checked apart from its compilation.
* Records against the oracle for waves built to take every branch of the set-up: all-nice waves, one lane at each end of the nice ranges
  and one just outside, one wave per octant, the same with one live lane of the opposite signs, and with only dead lanes of the opposite
  signs (tmin >= tmax; the lanes past numRays of a ragged last wave).
* The reference's missed test recorded at t = FLT_MAX (tmax = +inf), beside the values next to it, through the binary and the wide trace.
  Every record is compared in all four words: id and t against the oracle, u and v against the two sums restated here (expected_uv).
* Buffers placed where the set-up's preconditions fail: a node buffer 16 but not 64 bytes aligned (no scalar prologue), an empty leaf in
  the last bytes of triWoop (the descriptor fallback), as separate allocations and as one."""
import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

F = np.float32
U = np.uint32
FLT_MAX = np.finfo(F).max
gpu = pytest.mark.gpu

BODIES = (("fermi_speculative_while_while", {}),
          ("fermi_speculative_while_while", {"NTR_TRACE_MINIPOOL": "1"}),      # the mini kernel's own per-ray path, closest hit included
          ("fermi_speculative_while_while", {"NTR_TRACE_MINIPOOL": "2"}),
          ("fermi_speculative_while_while", {"NTR_TRACE_MINIPOOL": "4"}),
          ("kepler_dynamic_fetch", {}))


def f32(bits):
    return np.asarray(bits, dtype=U).view(F)


def below(x):
    return np.nextafter(F(x), F(0))


def above(x):
    return np.nextafter(F(x), F(np.inf) if x > 0 else F(-np.inf))


# ---- the class of a ray ---------------------------------------------------------------------------------------------------------------
NICE = np.array([(1.5, -2.5, 3.25, 0.0, 0.3, -0.4, 0.5, 1e30)], dtype=nt.RAY_DTYPE)
COMPONENTS = ("ox", "oy", "oz", "dx", "dy", "dz")


def class_rays():
    """each component through all 256 exponents x mantissa {0, 1, 0x7FFFFF} x both signs, the other five nice; then 2^16 random patterns"""
    e, m, s = np.meshgrid(np.arange(256, dtype=U), np.array([0, 1, 0x7FFFFF], dtype=U), np.array([0, 1], dtype=U), indexing="ij")
    words = f32(((s << U(31)) | (e << U(23)) | m).reshape(-1))
    parts = []
    for c in COMPONENTS:
        r = np.repeat(NICE, words.shape[0])
        r[c] = words
        parts.append(r)
    rnd = np.zeros(1 << 16, dtype=nt.RAY_DTYPE)
    rng = np.random.default_rng(2)
    for c in COMPONENTS:
        rnd[c] = f32(rng.integers(0, 1 << 32, rnd.shape[0], dtype=np.uint64).astype(U))
    return np.concatenate(parts + [rnd])


def rule(rays, zero_ok):
    """the ranges as trace_lane.h states them, in float compares (NaN fails every compare)"""
    with np.errstate(invalid="ignore"):
        ok = np.ones(rays.shape[0], dtype=bool)
        for c in ("dx", "dy", "dz"):
            a = np.abs(rays[c])
            ok &= (a >= F(2.0 ** -40)) & (a <= F(2.0 ** 20))
        for c in ("ox", "oy", "oz"):
            a = np.abs(rays[c])
            ok &= ((a >= F(2.0 ** -36)) & (a < F(2.0 ** 55))) | (zero_ok & (rays[c] == 0))
    return ok


def integer_class(rays, zero_ok):
    """ray_class of trace_lane.h, word for word, in 64-bit arithmetic reduced mod 2^32"""
    M = np.uint64(0xFFFFFFFF)
    w = lambda c, lo2: ((rays[c].view(U).astype(np.uint64) << np.uint64(1)) - np.uint64(lo2)) & M
    zero_word = np.uint64(0xA5000000 if zero_ok else 0xA5000001)
    d = np.maximum(np.maximum(w("dx", 0x57000000), w("dy", 0x57000000)), w("dz", 0x57000000))
    p = [np.where(x == zero_word, np.uint64(0), x) for x in (w("ox", 0x5B000000), w("oy", 0x5B000000), w("oz", 0x5B000000))]
    return np.maximum(np.maximum(np.maximum(p[0], p[1]), p[2]), np.minimum(d + np.uint64(0x5AFFFFFE - 0x3C000000), M))


@pytest.mark.parametrize("zero_ok", (False, True))
def test_integer_class_restated_in_numpy_equals_the_rule(zero_ok):
    rays = class_rays()
    want = rule(rays, zero_ok)
    assert 1000 < want.sum() < rays.shape[0] - 1000, "both classes must occur"
    got = integer_class(rays, zero_ok) <= 0x5AFFFFFE
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "ray %d: %r" % (bad[0], rays[bad[0]])


@gpu
@pytest.mark.parametrize("flags", (0, nt.BVH_NOTINY))
def test_selftest_ray_class_counts_no_difference(flags):
    from gpu_util import up
    rays = class_rays()
    assert rays.shape[0] == 6 * 256 * 3 * 2 + (1 << 16)
    zero = rays[(rays["ox"] == 0) | (rays["oy"] == 0) | (rays["oz"] == 0)]
    assert zero.shape[0] >= 6 and rule(zero, True).sum() > rule(zero, False).sum(), "the flag must matter on these rays"
    d_rays = up(rays)
    assert nt.selftest_ray_class(d_rays.data_ptr(), rays.shape[0], flags | nt.BVH_FASTDIV) == 0


# ---- records ---------------------------------------------------------------------------------------------------------------------------
_cache = {}


def soup():
    if "soup" not in _cache:
        tri, pos, cam = scenes.random_soup(1000, seed=11, walls=False)
        _cache["soup"] = (nt.sah_build(tri, pos), pos.min(0).astype(F), pos.max(0).astype(F))
    return _cache["soup"]


def aimed(rng, n, signs, lo, hi, tmax=1e30):
    """n rays with the direction signs given ((n, 3) or (3,) of +-1) that cross the scene's box: origin = a point of the box - 40 % .. 90 % of
    the box's diagonal along the direction"""
    r = np.zeros(n, dtype=nt.RAY_DTYPE)
    d = rng.uniform(0.2, 1.0, (n, 3)) * np.broadcast_to(np.asarray(signs, dtype=np.float64), (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    target = rng.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (n, 3))
    o = target - d * (rng.uniform(0.4, 0.9, n) * np.linalg.norm(hi - lo))[:, None]
    r["ox"], r["oy"], r["oz"] = o[:, 0].astype(F), o[:, 1].astype(F), o[:, 2].astype(F)
    r["dx"], r["dy"], r["dz"] = d[:, 0].astype(F), d[:, 1].astype(F), d[:, 2].astype(F)
    r["tmin"], r["tmax"] = 0.0, tmax
    return r


def setup_rays():
    """64 waves and one ray: what each wave is for stands beside it"""
    host, lo, hi = soup()
    rng = np.random.default_rng(5)
    octants = [np.array([1 - 2 * (o & 1), 1 - 2 * ((o >> 1) & 1), 1 - 2 * ((o >> 2) & 1)]) for o in range(8)]
    waves = []
    for i in range(10):                                    # all nice, signs mixed (wave 0: + + +, the ray the ragged wave's dead lanes load)
        waves.append(aimed(rng, 64, octants[0] if i == 0 else rng.choice((-1, 1), (64, 3)), lo, hi))
    edge_dir = (F(2.0 ** -40), F(2.0 ** 20), below(2.0 ** -40), above(2.0 ** 20))          # in, in, out, out
    edge_pos = (F(2.0 ** -36), below(2.0 ** 55), below(2.0 ** -36), F(2.0 ** 55), F(0.0), F(-0.0))
    for comps, values in ((("dx", "dy", "dz"), edge_dir), (("ox", "oy", "oz"), edge_pos)):
        for c in comps:
            for k, v in enumerate(values):                 # one lane at the value, the other 63 nice
                w = aimed(rng, 64, octants[len(waves) % 8], lo, hi)
                lane = int(rng.integers(0, 64))
                w[c][lane] = v if (k & 1) == 0 else -v
                waves.append(w)
    for o in range(8):                                     # uniform in sign: the octant's own loop
        waves.append(aimed(rng, 64, octants[o], lo, hi))
    for o in range(8):                                     # one live lane of the opposite signs: the general loop
        w = aimed(rng, 64, octants[o], lo, hi)
        w[int(rng.integers(0, 64))] = aimed(rng, 1, octants[7 - o], lo, hi)[0]
        waves.append(w)
    for o in range(8):                                     # only dead lanes of the opposite signs: still the octant's loop
        w = aimed(rng, 64, octants[o], lo, hi)
        for lane in rng.choice(64, 5, replace=False):
            w[lane] = aimed(rng, 1, octants[7 - o], lo, hi)[0]
            w["tmin"][lane], w["tmax"][lane] = (1.0, 1.0) if lane & 1 else (2.0, -1.0)
        waves.append(w)
    assert len(waves) == 64
    last = aimed(rng, 1, octants[7], lo, hi)               # the ragged wave: one live lane, - - -; its other lanes load ray 0 (+ + +) and are dead
    return np.concatenate(waves + [last])


class Placed:
    """A host BVH on the device: separate allocations or one, the node buffer 64-byte aligned or 16 bytes past that"""

    def __init__(self, host, one_allocation=False, node_skew=0):
        import torch
        from gpu_util import up
        self.host = host
        nb, wb, ib = host.nodes.nbytes, host.woop.nbytes, host.tri_index.nbytes
        rnd = lambda x: (x + 255) // 256 * 256   # (keeps every part on the 64-byte grid)

        def put(buf, at, a):
            buf[at:at + a.nbytes] = up(a)

        if one_allocation:
            self.buf = torch.zeros(512 + rnd(nb) + rnd(wb) + rnd(ib), dtype=torch.uint8, device="cuda:0")
            at_nodes = (-self.buf.data_ptr()) % 64 + node_skew
            at_woop = at_nodes - node_skew + 64 + rnd(nb)
            offs = (at_nodes, at_woop, at_woop + rnd(wb))
            bufs = (self.buf, self.buf, self.buf)
        else:
            bufs = tuple(torch.zeros(n + 128, dtype=torch.uint8, device="cuda:0") for n in (nb, wb, ib))
            offs = ((-bufs[0].data_ptr()) % 64 + node_skew, (-bufs[1].data_ptr()) % 64, (-bufs[2].data_ptr()) % 64)
            self.bufs = bufs
        for b, at, a in zip(bufs, offs, (host.nodes, host.woop, host.tri_index)):
            put(b, at, a)
        ptr = [b.data_ptr() + at for b, at in zip(bufs, offs)]
        assert ptr[0] % 64 == node_skew and ptr[1] % 16 == 0 and ptr[2] % 4 == 0
        self.view = nt.BvhView(ptr[0], nb, ptr[1], wb, ptr[2])
        self.flags = self.view.validate()


def expected_uv(host, rays, ref):
    """The u and v words of a record whose id and t the oracle gave: Intersect::RayTriangleWoop's two sums on the hit triangle's rows (the
    kernels' own operation order: tests/np_bvh_wide.py _dot4), 0 for a miss and for the missed test recorded at t = FLT_MAX."""
    from np_bvh_wide import _dot4
    woop = np.frombuffer(host.woop.tobytes(), dtype=F).reshape(-1, 4)
    woop_u = woop.view(U)
    tri_index = np.asarray(host.tri_index, dtype=np.int32)
    row_of = np.full(int(tri_index.max()) + 1, -1, dtype=np.int64)
    r = 0
    while r < woop.shape[0]:
        if woop_u[r, 0] == 0x80000000:
            r += 1
        else:
            row_of[tri_index[r]] = r
            r += 3
    real = (ref["id"] >= 0) & ~((ref["t"] == FLT_MAX) & np.isinf(rays["tmax"]))
    rows = row_of[np.where(real, ref["id"], 0)]
    assert (rows[real] >= 0).all()
    out = []
    with np.errstate(all="ignore"):
        for k in (1, 2):
            a = woop[rows + k]
            w = _dot4(a, rays["ox"], rays["oy"], rays["oz"], np.ones(rays.shape[0], dtype=F)) + ref["t"] * _dot4(
                a, rays["dx"], rays["dy"], rays["dz"], np.zeros(rays.shape[0], dtype=F))
            out.append(np.where(real, w.astype(F).view(np.int32), 0).astype(np.int32))
    return out


def check(monkeypatch, dbvh, rays, counts, what, ref_trace=None):
    """every body on rays[:n], closest hit and any hit, against the oracle; the overflow bit stays clear"""
    from gpu_util import gpu_trace
    from oracle import oracle
    host = dbvh.host
    refs = {ah: oracle.trace(host.nodes, host.woop, host.tri_index, rays, any_hit=ah)[0] for ah in (False, True)}
    uvs = {ah: expected_uv(host, rays, refs[ah]) for ah in (False, True)}
    nt.trace_status()
    monkeypatch.setenv("NTR_TRACE_ROUTE", "0")
    try:
        for kernel, env in BODIES:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            nt.set_tunables()
            for any_hit in (False, True):
                ref = refs[any_hit]
                for n in counts:
                    got, _ = gpu_trace(kernel, dbvh, rays[:n], any_hit)
                    bad = np.nonzero((got["id"] != ref["id"][:n]) | (got["t"].view(U) != ref["t"][:n].view(U)) |
                                     (got["padA"] != uvs[any_hit][0][:n]) | (got["padB"] != uvs[any_hit][1][:n]))[0]
                    assert bad.size == 0, "%s: %s %s any_hit=%s n=%d: %d records differ, first at ray %d: got %r want (%d, %r, %d, %d)" % (
                        what, kernel, env, any_hit, n, bad.size, bad[0], got[bad[0]], ref["id"][bad[0]], ref["t"][bad[0]],
                        uvs[any_hit][0][bad[0]], uvs[any_hit][1][bad[0]])
            for k in env:
                monkeypatch.delenv(k, raising=False)
        assert nt.trace_status() == 0, what + ": the stack-overflow bit must stay clear"
    finally:
        for k in ("NTR_TRACE_ROUTE", "NTR_TRACE_MINIPOOL"):
            monkeypatch.delenv(k, raising=False)
        nt.set_tunables()
    return refs


@gpu
def test_waves_that_take_every_branch_of_the_setup_against_the_oracle(monkeypatch):
    host, lo, hi = soup()
    rays = setup_rays()
    assert rays.shape[0] == 4097
    dbvh = Placed(host)
    assert dbvh.flags & nt.BVH_FASTDIV and dbvh.flags & nt.BVH_ORDERED, "the soup must select the FAST path and the octant vote"
    nice = rule(rays, bool(dbvh.flags & nt.BVH_NOTINY))
    per_wave = nice[:4096].reshape(64, 64).sum(1)
    assert (per_wave == 64).sum() >= 46 and (per_wave == 63).sum() >= 12, "FAST waves and waves kept off it by one lane"
    refs = check(monkeypatch, dbvh, rays, (4097, 4096, 4033), "set-up waves")
    hits = int((refs[False]["id"] >= 0).sum())
    assert 200 < hits < 3900, "the rays must hit and miss (%d hit)" % hits


# ---- the missed test that is recorded --------------------------------------------------------------------------------------------------
def quirk_rays():
    host, lo, hi = soup()
    rng = np.random.default_rng(8)
    rays = aimed(rng, 2048, rng.choice((-1, 1), (2048, 3)), lo, hi)
    tmax = np.array([np.inf, np.nan, FLT_MAX, below(FLT_MAX)], dtype=F)
    tmin = np.array([0.0, FLT_MAX], dtype=F)
    combo = np.arange(2048) % 8                      # the first half lane by lane: every wave holds all eight
    combo[1024:] = (np.arange(1024) // 128) % 8      # the second half in blocks of two waves: waves with and without +inf
    rays["tmax"], rays["tmin"] = tmax[combo % 4], tmin[combo // 4]
    return rays


@gpu
def test_a_missed_test_is_recorded_at_flt_max_only_under_an_infinite_tmax(monkeypatch):
    host, lo, hi = soup()
    rays = quirk_rays()
    dbvh = Placed(host)
    refs = check(monkeypatch, dbvh, rays, (2048, 2047), "miss quirk")
    ref = refs[False]
    inf_rays = np.isinf(rays["tmax"]) & (rays["tmin"] == 0)
    quirk = (ref["id"] >= 0) & (ref["t"] == FLT_MAX)
    assert quirk[inf_rays].sum() > 20 and not quirk[~inf_rays].any(), "recorded misses: under tmax = +inf and tmin = 0, and nowhere else"
    assert ((ref["id"] >= 0) & (ref["t"] < FLT_MAX))[inf_rays].sum() > 20, "and real hits beside them"


@gpu
def test_the_wide_trace_keeps_the_recorded_miss():
    from test_bvh_wide_gpu import _Tree, _assert_trace_equals_spec
    host, lo, hi = soup()
    rays = quirk_rays()[::2]
    t = _Tree(host.nodes, host.woop, host.tri_index)
    rid = _assert_trace_equals_spec(t, t.wide, rays, "miss quirk")     # tests/np_bvh_wide.py on the device's own wide tree
    assert (np.isinf(rays["tmax"]) & (rays["tmin"] == 0) & (rid >= 0)).sum() > 20


# ---- buffer placement ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("one_allocation", (False, True))
def test_a_node_buffer_off_the_64_byte_grid_runs_without_the_scalar_prologue(monkeypatch, one_allocation):
    host, lo, hi = soup()
    rays = setup_rays()[: 40 * 64 + 1]
    check(monkeypatch, Placed(host, one_allocation, node_skew=16), rays, (rays.shape[0],), "nodes at 16 mod 64, one allocation: %s" % one_allocation)


@gpu
@pytest.mark.parametrize("one_allocation", (False, True))
def test_an_empty_leaf_in_the_last_bytes_of_triwoop(monkeypatch, one_allocation):
    from test_unified_loop_gpu import end_leaf_tree
    host, cam = end_leaf_tree()
    rays = np.concatenate([scenes.primary_rays(cam, 24, 16)[0], scenes.random_rays(641, seed=4)])
    check(monkeypatch, Placed(host, one_allocation), rays, (rays.shape[0], 64), "end leaf, one allocation: %s" % one_allocation)
