"""The carried certain descent of the per-ray kernels' prologue (NTR_TRACE_CERTAIN_DESCENT) on the GPU: records equal the oracle's bit for
bit, and the records of the same launch with the knob at 0, any hit (certain steps at their default) and closest hit
(NTR_TRACE_CERTAIN_STEPS=2), for batches of 64, 65 and 64 x 8 rays.  The trees are hand-built chains: inner node k holds the one-triangle
leaf k and the rest of the chain, clusters ten units apart, 1 to 6 inner levels -- a wave of short rays that starts in cluster j is
carried for j steps (one fewer in the last two clusters) and then handed a leaf, so the run of carried steps has every length from 0 to 5;
the rest of the chain is child 0 or child 1 in turn, with either parity.  The waves are the ones on which the loop, not the rule, can go
wrong: see `cases`."""
import numpy as np
import pytest

import ntrace_amd as nt
from oracle import oracle

pytestmark = pytest.mark.gpu

F = np.float32
GROUP = 8          # waves per batch: 64 x 8 rays
SPACING = 10.0


def chain_tree(xs, flip):
    """Inner node k: leaf k (a one-triangle cluster, box x in [xs[k], xs[k] + 1], y and z in [1, 2]) and the rest of the chain, which is
    child (k + flip) & 1; the last inner node holds the last two leaves and is the last record of the node buffer."""
    from np_hlbvh import woop_rows
    n = len(xs)
    levels = n - 1
    pos = np.concatenate([[[x, 1, 1], [x + 1, 1, 1.25], [x, 2, 2]] for x in xs]).astype(F)
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    rows = woop_rows(tri, pos).reshape(n, 3, 4)
    term = np.full((1, 4), 0x80000000, dtype=np.uint32).view(F)
    woop = np.concatenate([np.concatenate([rows[i], term]) for i in range(n)]).astype(F)      # leaf i at float4 index 4 i
    tri_index = np.zeros(4 * n, dtype=np.int32)
    tri_index[0::4] = np.arange(n)
    lo, hi = pos.reshape(n, 3, 3).min(1), pos.reshape(n, 3, 3).max(1)

    def node(lo0, hi0, c0, lo1, hi1, c1):
        r = np.zeros(16, dtype=F)
        r[0:4] = (lo0[0], hi0[0], lo0[1], hi0[1])
        r[4:8] = (lo1[0], hi1[0], lo1[1], hi1[1])
        r[8:12] = (lo0[2], hi0[2], lo1[2], hi1[2])
        r.view(np.int32)[12:14] = (c0, c1)
        return r
    leaf = lambda i: ~(4 * i)
    recs = []
    for k in range(levels):
        rest = (lo[k + 1:].min(0), hi[k + 1:].max(0), 64 * (k + 1) if k + 1 < levels else leaf(k + 1))
        own = (lo[k], hi[k], leaf(k))
        recs.append(node(*rest, *own) if (k + flip) & 1 == 0 else node(*own, *rest))
    nodes = np.concatenate(recs)
    return nt.HostBvh(nodes.view(np.uint8).copy(), woop.reshape(-1).view(np.uint8).copy(), tri_index)


def unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.where(np.abs(d) < 1e-4, 1e-4, d)


def cases(xs, seed):
    """The waves of one tree, 64 rays each."""
    rng = np.random.default_rng(seed)
    n = len(xs)
    levels = n - 1
    waves = []

    def wave(o, d, tmin, tmax):
        r = np.zeros(64, dtype=nt.RAY_DTYPE)
        o, d = np.broadcast_to(o, (64, 3)), np.broadcast_to(d, (64, 3))
        r["ox"], r["oy"], r["oz"], r["dx"], r["dy"], r["dz"] = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
        r["tmin"], r["tmax"] = tmin, tmax
        waves.append(r)
        return r

    def inside(j, count):
        """origins inside cluster j's box, a tenth off its faces, half of them 1e-4 off its triangle"""
        p = rng.random((count, 3)) * 0.8 + 0.1
        w = rng.dirichlet((2, 2, 2), count)
        on = w @ np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 1]]) + rng.choice((-1e-4, 1e-4), (count, 1)) * np.array([-0.25, -1, 1]) / 1.4361
        p[::2] = np.clip(on[::2], 1e-3, 1 - 1e-3)
        return p + np.array([xs[j], 1, 1])

    def bundle(j, length):
        """8 origins x 8 directions in cluster j (mixed direction signs: the wave runs the general slab test's instance)"""
        return wave(np.repeat(inside(j, 8), 8, axis=0), unit_dirs(rng, 64), 0.0, length)

    def octant_bundle(j, length, signs):
        """... with the direction signs the same in every lane (the octant's own instance of the prologue)"""
        return wave(np.repeat(inside(j, 8), 8, axis=0), np.abs(unit_dirs(rng, 64)) * np.array(signs), 0.0, length)

    # 8 origins x 8 directions with length 5, 1e-3 and 1e4 from every cluster: j carried steps, then a leaf (for the last two clusters
    # the carried run ends on the last record of the node buffer, whose children are both leaves)
    for j in range(n):
        for length in (5.0, 1e-3, 1e4):
            bundle(j, length)
        octant_bundle(j, 5.0, (1, -1, 1) if j & 1 else (-1, -1, -1))
    # the lanes part at step k: half of them in cluster k, the others at the end of the chain; the leading lanes on either side
    for k in range(levels):
        for lead in (0, 1):
            o = np.where(((np.arange(64) // 8 + lead) % 2 == 0)[:, None], np.repeat(inside(k, 8), 8, axis=0), np.repeat(inside(n - 1, 8), 8, axis=0))
            wave(o, unit_dirs(rng, 64), 0.0, 5.0)
    # one lane uncertain at step k after k carried steps: from the near face of the rest of the chain (a child plane of node k) straight
    # at leaf k, ending on the leaf's plane and 3 ulp either side of it
    for k in range(levels):
        for ulp in (-3, 0, 3):
            r = bundle(n - 1, 5.0)
            lane = int(rng.integers(0, 64))
            d = np.array([-1.0, 2.0 ** -7, -(2.0 ** -8)], dtype=F)
            ox, plane = F(xs[k + 1]), F(xs[k] + 1)
            t = F(F(plane - ox) / d[0])
            r["ox"][lane], r["oy"][lane], r["oz"][lane] = ox, 1.5, 1.5
            r["dx"][lane], r["dy"][lane], r["dz"][lane] = d
            r["tmax"][lane] = (np.array([t], dtype=F).view(np.int32) + ulp).view(F)[0]
    # dead leading lanes, degenerate lanes in between, a wave without a live lane, tmin = -0
    r = bundle(n - 1, 5.0); r["tmax"][0:37] = -1.0
    r = bundle(n - 1, 5.0); r["tmax"][5::2] = -1.0; r["tmin"][8] = 6.0
    r = bundle(n - 1, 5.0); r["tmax"][:] = -1.0
    r = bundle(n - 1, 5.0); r["tmin"][40] = -0.0
    # one lane with tmin > 0: the wave must not enter; a wave that is not FAST
    r = bundle(n - 1, 5.0); r["tmin"][13] = 1e-3
    r = bundle(n - 1, 5.0); r["tmax"][3] = np.inf; r["dx"][5] = 0.0
    # one lane far-reaching from the start (two uncertain steps in a row: the wave gives up, and the nodes below would have been certain)
    r = bundle(n - 1, 5.0); r["tmax"][17] = 1e4
    # every lane towards the start of the chain with reach 7 (the close-set chain: uncertain at nodes 0 and 1, certain from node 2 on)
    wave(np.repeat(inside(min(2, n - 1), 8), 8, axis=0), np.array([-1.0, 2.0 ** -6, 2.0 ** -7]), 0.0, 7.0)
    while len(waves) % GROUP:
        bundle(int(rng.integers(0, n)), 5.0)
    return np.concatenate(waves)


class OffsetBvh:
    """The same tree with its node buffer 16 bytes off a 64-byte boundary: the scalar prologue is off, records are the same."""

    def __init__(self, host):
        import torch
        from gpu_util import up
        self.host = host
        raw = torch.zeros(host.nodes.nbytes + 64, dtype=torch.uint8, device="cuda:0")
        raw[16:16 + host.nodes.nbytes] = up(host.nodes)
        self.raw, self.woop, self.idx = raw, up(host.woop), up(host.tri_index)
        assert raw.data_ptr() % 64 == 0
        self.view = nt.BvhView(raw.data_ptr() + 16, host.nodes.nbytes, self.woop.data_ptr(), host.woop.nbytes, self.idx.data_ptr())
        self.flags = self.view.validate()


def chain(levels, close=False):
    xs = [1.0 + SPACING * i for i in range(levels + 1)]
    if close:                       # the first three clusters three units apart: within reach 7 of each other
        xs = [1.0, 4.0, 7.0] + [7.0 + SPACING * i for i in range(1, levels - 1)]
    return xs


TREES = [(levels, flip, False) for levels in range(1, 7) for flip in (0, 1)] + [(4, 0, True), (4, 1, True)]


@pytest.mark.parametrize("levels,flip,close", TREES)
def test_carried_descent_changes_no_record(monkeypatch, levels, flip, close):
    from gpu_util import DeviceBvh, assert_parity, gpu_trace
    xs = chain(levels, close)
    host = chain_tree(xs, flip)
    assert host.nodes.nbytes == 64 * levels and len(xs) <= 64
    rays = cases(xs, 100 * levels + 10 * flip + close)
    refs = {ah: oracle.trace(host.nodes, host.woop, host.tri_index, rays, any_hit=ah, threads=8)[0] for ah in (False, True)}
    hits = int((refs[True]["id"] >= 0).sum())
    assert 0 < hits < rays.shape[0], "the rays must hit and miss"
    dbvh = DeviceBvh(host)
    assert dbvh.flags & nt.BVH_ORDERED and dbvh.flags & nt.BVH_FASTDIV, "the tree must qualify for the FAST path and certain steps"
    off = OffsetBvh(host)
    assert off.flags == dbvh.flags
    groups = range(0, rays.shape[0], 64 * GROUP)
    got = {}
    try:
        for any_hit, steps in ((True, None), (False, "2")):
            for descent in ("1", "0"):
                monkeypatch.setenv("NTR_TRACE_CERTAIN_DESCENT", descent)
                if steps is None:
                    monkeypatch.delenv("NTR_TRACE_CERTAIN_STEPS", raising=False)
                else:
                    monkeypatch.setenv("NTR_TRACE_CERTAIN_STEPS", steps)
                nt.set_tunables()
                assert nt.trace_plan_certain(any_hit) == dict(certainSteps=True, certainDescent=descent == "1")
                for g in groups:
                    for n in (64, 65, 64 * GROUP):
                        what = "levels=%d flip=%d close=%d any_hit=%s descent=%s group=%d n=%d" % (levels, flip, close, any_hit, descent, g, n)
                        res, _ = gpu_trace("fermi_speculative_while_while", dbvh, rays[g:g + n], any_hit)
                        assert_parity(res, refs[any_hit][g:g + n], what)
                        got[(any_hit, descent, g, n)] = res
                        if descent == "0":      # the same launch with the knob at 0
                            assert got[(any_hit, "1", g, n)].tobytes() == res.tobytes(), what
                    res, _ = gpu_trace("fermi_speculative_while_while", off, rays[g:g + 64 * GROUP], any_hit)
                    assert_parity(res, refs[any_hit][g:g + 64 * GROUP], "node buffer 16 bytes off: " + what)
    finally:
        monkeypatch.delenv("NTR_TRACE_CERTAIN_DESCENT", raising=False)
        monkeypatch.delenv("NTR_TRACE_CERTAIN_STEPS", raising=False)
        nt.set_tunables()
