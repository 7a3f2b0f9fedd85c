"""Certain steps of the per-ray kernels' prologue (NTR_TRACE_CERTAIN_STEPS) on the GPU: records equal the oracle's bit for bit with the
knob at 0, at 1 (the default: any-hit launches take certain steps) and at 2 (closest-hit launches too), any hit and closest hit, on
a hand-built three-level tree and on the atrium SAH tree, for batches of 64, 65 and 64 x 200 rays.  The rays are the ones the rule is about: AO-style bundles (8 origins x 8 directions a wave, 1e-4 off a surface, tmin 0)
of length 5, 1e-3 and 1e4, origins copied from top-level node planes, rays that end on (and a few ulp either side of) a sibling's
plane, and waves that must fall back to the exact prologue or mix with it: one lane with tmin > 0, dead and degenerate lanes, one lane
pointing away."""
import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
from oracle import oracle

pytestmark = pytest.mark.gpu

F = np.float32
TOTAL = 64 * 200


def hand_tree():
    """Root -> two inner nodes -> four one-triangle leaves, in four clusters along x ([0, 1], [2, 3], [10, 11], [12, 13]): the root's child
    boxes stand 7 units apart, each inner node's 1 unit.  Cluster B's triangle lies in the plane z = 0.5 (a zero-thickness box) and
    cluster C's in the plane x = 10 (the sibling plane of the root IS a flat box's)."""
    pos = np.array([[0, 0, 0], [1, 0, 0.2], [0, 1, 1],            # A
                    [2, 0, 0.5], [3, 0, 0.5], [2, 1, 0.5],        # B: flat in z
                    [10, 0, 0], [10, 1, 0], [10, 0, 1],           # C: flat in x
                    [12, 0, 0], [13, 1, 0.3], [12.5, 1, 1]], dtype=F)
    tri = np.arange(12, dtype=np.int32).reshape(4, 3)
    from np_hlbvh import woop_rows
    rows = woop_rows(tri, pos).reshape(4, 3, 4)
    term = np.full((1, 4), 0x80000000, dtype=np.uint32).view(F)
    woop = np.concatenate([np.concatenate([rows[i], term]) for i in range(4)]).astype(F)      # leaf i at float4 index 4 i
    tri_index = np.zeros(16, dtype=np.int32)
    tri_index[0::4] = np.arange(4)
    lo = pos.reshape(4, 3, 3).min(1)
    hi = pos.reshape(4, 3, 3).max(1)

    def node(lo0, hi0, c0, lo1, hi1, c1):
        n = np.zeros(16, dtype=F)
        n[0:4] = (lo0[0], hi0[0], lo0[1], hi0[1])
        n[4:8] = (lo1[0], hi1[0], lo1[1], hi1[1])
        n[8:12] = (lo0[2], hi0[2], lo1[2], hi1[2])
        n.view(np.int32)[12:14] = (c0, c1)
        return n
    leaf = lambda i: ~(4 * i)
    nodes = np.concatenate([
        node(np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1]), 64, np.minimum(lo[2], lo[3]), np.maximum(hi[2], hi[3]), 128),
        node(lo[0], hi[0], leaf(0), lo[1], hi[1], leaf(1)),
        node(lo[2], hi[2], leaf(2), lo[3], hi[3], leaf(3))])
    return nt.HostBvh(nodes.view(np.uint8).copy(), woop.reshape(-1).view(np.uint8).copy(), tri_index), tri, pos


def top_nodes(nodes_u8, count):
    """the first `count` inner nodes breadth first: (12 planes, child words)"""
    f = nodes_u8.view(F)
    i = nodes_u8.view(np.int32)
    out, queue = [], [0]
    while queue and len(out) < count:
        b = queue.pop(0) // 4
        out.append(f[b:b + 12].copy())
        queue += [int(c) for c in i[b + 12:b + 14] if c >= 0]
    return out


def unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.where(np.abs(d) < 1e-4, 1e-4, d)


def ray_set(host, tri, pos, seed):
    rng = np.random.default_rng(seed)
    waves = []

    def wave(o, d, tmin, tmax):
        r = np.zeros(64, dtype=nt.RAY_DTYPE)
        o, d = np.broadcast_to(o, (64, 3)), np.broadcast_to(d, (64, 3))
        r["ox"], r["oy"], r["oz"], r["dx"], r["dy"], r["dz"] = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
        r["tmin"], r["tmax"] = tmin, tmax
        waves.append(r)
        return r

    v = pos[tri].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)

    def bundle(length):
        """8 origins 1e-4 off neighbouring triangles x 8 directions of their hemispheres"""
        t0 = int(rng.integers(0, tri.shape[0]))
        ts = (t0 + np.arange(8)) % tri.shape[0]
        w = rng.dirichlet((1, 1, 1), 8)
        side = rng.choice((-1.0, 1.0), 8)[:, None]
        o = (v[ts] * w[:, :, None]).sum(1) + side * nrm[ts] * 1e-4
        d = unit_dirs(rng, 64).reshape(8, 8, 3)
        flip = ((d * (side * nrm[ts])[:, None, :]).sum(2) < 0)[:, :, None]
        d = np.where(flip, -d, d)
        return wave(np.repeat(o, 8, axis=0), d.reshape(64, 3), 0.0, length)

    bundle(5.0)                                                   # the batch of 64 is one AO wave
    # the second wave (the batch of 65 ends one ray into it) and the next ones: waves that must not, or only partly, take certain steps
    r = bundle(5.0); r["tmin"][13] = 1e-3                         # one lane with tmin > 0: the whole wave runs the exact prologue
    r = bundle(5.0); r["tmax"][0:37] = -1.0                       # the first 37 lanes dead
    r = bundle(5.0); r["tmax"][5::2] = -1.0; r["tmin"][8] = 6.0   # dead and degenerate lanes among live ones
    r = bundle(5.0)
    for k in ("dx", "dy", "dz"):
        r[k][21] = -r[k][21]                                      # one lane pointing away (into the surface)
    r = bundle(5.0); r["tmax"][:] = -1.0                          # a wave with no live lane
    r = bundle(5.0); r["tmin"][40] = -0.0                         # tmin = -0 counts as 0
    r = bundle(5.0); r["tmax"][3] = np.inf; r["tmax"][4] = np.nan; r["dx"][5] = 0.0   # a wave that is not FAST
    for length in (1e-3, 1e4):
        for _ in range(6):
            bundle(length)
    # origins copied from top-level node planes (corners and faces of the child boxes), eight directions each
    tops = top_nodes(host.nodes, 7)
    for p in tops:
        for c in (0, 1):
            bx = (p[0 + 4 * c], p[1 + 4 * c]), (p[2 + 4 * c], p[3 + 4 * c]), (p[8 + 2 * c], p[9 + 2 * c])
            o = np.array([[bx[0][(i >> 0) & 1], bx[1][(i >> 1) & 1], bx[2][(i >> 2) & 1]] for i in range(8)], dtype=np.float64)
            mid = np.array([0.5 * (b[0] + b[1]) for b in bx])
            face = o.copy()
            face[:, 1:] = mid[1:]                                 # on an x plane only / corner: 4 origins of each
            o = np.concatenate([o[:4], face[:4]])
            wave(np.repeat(o, 8, axis=0), unit_dirs(rng, 64), 0.0, 5.0)
    # endpoints on sibling planes: from inside one child of a top node towards the other along each axis, tmax = the quotient of the
    # sibling's near plane and up to 4 ulp either side of it, at steep and shallow angles
    for p in tops:
        for c in (0, 1):
            s = 1 - c
            lo = np.array([p[0 + 4 * c], p[2 + 4 * c], p[8 + 2 * c]], dtype=np.float64)
            hi = np.array([p[1 + 4 * c], p[3 + 4 * c], p[9 + 2 * c]], dtype=np.float64)
            slo = np.array([p[0 + 4 * s], p[2 + 4 * s], p[8 + 2 * s]], dtype=F)
            shi = np.array([p[1 + 4 * s], p[3 + 4 * s], p[9 + 2 * s]], dtype=F)
            o = (lo + rng.random((64, 3)) * (hi - lo)).astype(F)
            o = np.where(o == 0, F(2.0 ** -20), o)
            d = unit_dirs(rng, 64).astype(F)
            k = rng.integers(0, 3, 64)
            rows = np.arange(64)
            ahead = d[rows, k] > 0
            plane = np.where(ahead, slo[k], shi[k])                # the sibling's near plane on axis k
            with np.errstate(all="ignore"):
                t = ((plane - o[rows, k]).astype(F) / d[rows, k]).astype(F)
            t = np.where(np.isfinite(t) & (t > 0), t, F(5.0)).astype(F)
            steps = rng.integers(-4, 5, 64)
            t = (t.view(np.int32) + steps).astype(np.int32).view(F)
            wave(o, d, 0.0, t)
    special = np.concatenate(waves)
    assert special.shape[0] < TOTAL - 64 * 40, special.shape
    while sum(w.shape[0] for w in waves) < TOTAL:                 # the rest: AO bundles of length 5
        bundle(5.0)
    rays = np.concatenate(waves)[:TOTAL]
    assert rays.shape[0] == TOTAL
    return rays


def build_case(tree):
    if tree == "hand-built":
        host, tri, pos = hand_tree()
    else:
        tri, pos, _ = scenes.atrium()
        host = nt.sah_build(tri, pos, 1, 1)
    rays = ray_set(host, tri, pos, 7 if tree == "hand-built" else 8)
    refs = {ah: oracle.trace(host.nodes, host.woop, host.tri_index, rays, any_hit=ah, threads=8)[0] for ah in (False, True)}
    return host, rays, refs


@pytest.mark.parametrize("tree", ["hand-built", "atrium sah"])
def test_certain_steps_change_no_record(monkeypatch, tree):
    from gpu_util import DeviceBvh, assert_parity, gpu_trace
    host, rays, refs = build_case(tree)
    dbvh = DeviceBvh(host)
    assert dbvh.flags & nt.BVH_ORDERED and dbvh.flags & nt.BVH_FASTDIV, "the tree must qualify for the FAST path and certain steps"
    hits = int((refs[True]["id"] >= 0).sum())
    assert 0 < hits < rays.shape[0], "the AO rays must hit and miss"
    try:
        for knob in ("1", "0", "2"):
            monkeypatch.setenv("NTR_TRACE_CERTAIN_STEPS", knob)
            nt.set_tunables()
            for any_hit in (True, False):
                for n in (64, 65, TOTAL):
                    got, _ = gpu_trace("fermi_speculative_while_while", dbvh, rays[:n], any_hit)
                    assert_parity(got, refs[any_hit][:n], "%s certain=%s any_hit=%s n=%d" % (tree, knob, any_hit, n))
    finally:
        monkeypatch.delenv("NTR_TRACE_CERTAIN_STEPS", raising=False)
        nt.set_tunables()
