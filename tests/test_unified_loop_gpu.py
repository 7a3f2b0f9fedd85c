"""The unified-step loop's stack and fetch on the GPU, records word for word against tests/np_tracer.py.

The loop's bookkeeping (trace_lane.h: push, the pop of the per-ray bodies with its clamped LDS read and the scratch entry fetched over
it, the pop of the persistent kernels, the scratch levels; trace_fetch.h: the flat fetch's range check and its descriptor fallback)
changes no record, so what can go wrong is the loop, not a ray's arithmetic.  The trees are the ones on which it can:

* a "comb" of 40 inner levels whose two children are both hit at every level (comb_tree): a ray that enters at its open end pushes one
  leaf per level, so its stack passes LDS_DEPTH - 1, LDS_DEPTH and LDS_DEPTH + 1 on the way down and again on the way back, and a ray
  that starts at tooth j turns round at depth j -- a wave of rays with mixed j pops from scratch in some lanes, from LDS in others and
  pushes in the rest, in the same step.  Every closest-hit ray ends with the pop of the sentinel right after its last leaf; the comb's
  last leaf is empty and its terminator is the last row of triWoop (the descriptor fallback);
* a 300-triangle SAH tree under a new root whose second child is an empty leaf at the very end of triWoop, traced with ragged counts.

Each case runs the three bodies (NTR_TRACE_ROUTE=0: the body the selector names) and the per-ray body as mini-pools of two chunks, whose
refill restarts a lane's stack right after the pop that ended its ray."""
import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

pytestmark = pytest.mark.gpu

F = np.float32
LEVELS = 40
PITCH = 2.0            # distance between two teeth of the comb
TERM = 0x80000000

BODIES = (("fermi_speculative_while_while", {}),
          ("kepler_dynamic_fetch", {}),
          ("tesla_persistent_while_while", {}),
          ("fermi_speculative_while_while", {"NTR_TRACE_MINIPOOL": "2"}))


def node_record(lo0, hi0, c0, lo1, hi1, c1):
    r = np.zeros(16, dtype=F)
    r[0:4] = (lo0[0], hi0[0], lo0[1], hi0[1])
    r[4:8] = (lo1[0], hi1[0], lo1[1], hi1[1])
    r[8:12] = (lo0[2], hi0[2], lo1[2], hi1[2])
    r.view(np.int32)[12:14] = (c0, c1)
    return r


def tooth_x(k):
    """tooth k stands at x = tooth_x(k): the deeper the level, the nearer to the comb's open end at x = 0"""
    return PITCH * (LEVELS + 1 - k)


def comb_tree(flip):
    """Inner node k: tooth k (a one-triangle leaf in the box [x, x + 0.5] x [0, 1] x [0, 1], the triangle covering y + z < 1 of it) and the
    rest of the comb, which lies nearer to x = 0 and is child (k + flip) & 1.  The last inner node holds tooth LEVELS - 1 and an EMPTY leaf:
    a lone terminator, the last row of triWoop."""
    from np_hlbvh import woop_rows
    n = LEVELS
    xs = [tooth_x(k) for k in range(n)]
    pos = np.concatenate([[[x, 0, 0], [x + 0.5, 1, 0], [x, 0, 1]] for x in xs]).astype(F)
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    rows = woop_rows(tri, pos).reshape(n, 3, 4)
    term = np.full((1, 4), TERM, dtype=np.uint32).view(F)
    woop = np.concatenate([np.concatenate([rows[i], term]) for i in range(n)] + [term]).astype(F)   # tooth i at row 4 i, the empty leaf at row 4 n
    tri_index = np.zeros(4 * n + 1, dtype=np.int32)
    tri_index[0:4 * n:4] = np.arange(n)
    lo, hi = pos.reshape(n, 3, 3).min(1), pos.reshape(n, 3, 3).max(1)
    empty_lo, empty_hi = np.array([tooth_x(n), 0, 0], dtype=F), np.array([tooth_x(n) + 0.5, 1, 1], dtype=F)
    recs = []
    for k in range(n):
        own = (lo[k], hi[k], ~(4 * k))
        if k + 1 < n:
            rest = (np.minimum(lo[k + 1:].min(0), empty_lo), hi[k + 1:].max(0), 64 * (k + 1))
        else:
            rest = (empty_lo, empty_hi, ~(4 * n))
        recs.append(node_record(*rest, *own) if (k + flip) & 1 == 0 else node_record(*own, *rest))
    nodes = np.concatenate(recs)
    return nt.HostBvh(nodes.view(np.uint8).copy(), woop.reshape(-1).view(np.uint8).copy(), tri_index)


def comb_rays(seed):
    """Waves of 64 rays along +x through the comb.  A ray that starts in front of tooth j (j = LEVELS: in front of the open end) pushes
    j leaves and pops them again; y + z < 1 hits the teeth (an any-hit ray ends at its deepest tooth), y + z > 1 passes through every box and
    misses every triangle (an any-hit ray comes all the way back, too)."""
    rng = np.random.default_rng(seed)
    waves = []

    def wave(j, hit, tilt=1e-4, tmax=1e30):
        r = np.zeros(64, dtype=nt.RAY_DTYPE)
        j = np.broadcast_to(np.asarray(j), (64,))
        hit = np.broadcast_to(np.asarray(hit), (64,))
        y = rng.uniform(0.15, 0.35, 64)
        z = rng.uniform(0.15, 0.35, 64)
        y, z = np.where(hit, y, y + 0.5), np.where(hit, z, z + 0.5)
        r["ox"] = np.where(j >= LEVELS, 0.5, PITCH * (LEVELS + 1 - np.minimum(j, LEVELS - 1)) - 0.25).astype(F)
        r["oy"], r["oz"] = y.astype(F), z.astype(F)
        s = rng.choice((-1.0, 1.0), (64, 2))
        r["dx"], r["dy"], r["dz"] = 1.0, (tilt * s[:, 0]).astype(F), (tilt * s[:, 1]).astype(F)
        r["tmin"], r["tmax"] = 0.0, tmax
        waves.append(r)
        return r

    lanes = np.arange(64)
    wave(LEVELS, True)                                  # every lane down all 40 levels and back
    wave(LEVELS, False)
    wave(LEVELS, lanes % 2 == 0)
    # the mixed wave: lane l turns round at depth j(l), so while the deep lanes still push, the middle ones pop from scratch (sp >= 16)
    # and the shallow ones from LDS
    wave(rng.permutation(np.concatenate([np.arange(0, 41), np.arange(13, 21), np.arange(25, 40)]))[:64], lanes % 3 != 0)
    wave(np.where(lanes < 32, 14 + lanes % 6, LEVELS), False)   # around the LDS boundary: depths 14 .. 19
    wave(np.where(lanes < 48, 15 + lanes % 4, 1), True)
    wave(0, lanes % 2 == 0)                             # tooth 0 only: no push, the leaf, the pop of the sentinel
    r = wave(LEVELS, lanes % 4 != 1)                    # degenerate and dead lanes among deep ones
    r["tmax"][3::7] = -1.0
    r["tmin"][5::11] = 1e31
    r = wave(rng.integers(0, 41, 64), lanes % 2 == 1)   # not FAST: a zero direction component, an infinite tmax
    r["dy"][0:64:9] = 0.0
    r["tmax"][4] = np.inf
    wave(LEVELS, lanes % 5 != 0, tilt=2.0 ** -20, tmax=3.0 * PITCH)   # short rays: only the last teeth are within reach
    return np.concatenate(waves)


def end_leaf_tree():
    """A 300-triangle SAH tree under a new root: child 0 is the old root (moved to the end of the node buffer), child 1 an empty leaf
    appended to triWoop -- a lone terminator in the buffer's last 16 bytes -- in the scene's box, so every ray that meets the scene reads
    it: a 64-byte fetch that would cross the end of triWoop."""
    tri, pos, cam = scenes.random_soup(300, seed=5, walls=False)
    host = nt.sah_build(tri, pos)
    nodes = np.frombuffer(host.nodes.tobytes(), dtype=F).reshape(-1, 16).copy()
    woop = np.frombuffer(host.woop.tobytes(), dtype=np.uint32).reshape(-1, 4)
    lo, hi = pos.min(0) - F(1), pos.max(0) + F(1)
    old_root = nodes[0].copy()
    nodes = np.concatenate([nodes, old_root[None]])
    nodes[0] = node_record(lo, hi, 64 * (nodes.shape[0] - 1), lo, hi, ~woop.shape[0])
    woop = np.concatenate([woop, np.full((1, 4), TERM, dtype=np.uint32)])
    tri_index = np.concatenate([host.tri_index, np.zeros(1, dtype=np.int32)])
    return nt.HostBvh(nodes.reshape(-1).view(np.uint8).copy(), woop.reshape(-1).view(np.uint8).copy(), tri_index), cam


def check(monkeypatch, host, rays, counts, what):
    """Every body on rays[:n] for n in counts, closest hit and any hit, against np_tracer; the overflow bit stays clear."""
    import np_tracer
    from gpu_util import DeviceBvh, gpu_trace
    refs = {ah: np_tracer.trace(host.nodes, host.woop, host.tri_index, rays, any_hit=ah) for ah in (False, True)}
    hits = int((refs[False][0] >= 0).sum())
    assert 0 < hits < rays.shape[0], "the rays must hit and miss"
    dbvh = DeviceBvh(host)
    nt.trace_status()
    monkeypatch.setenv("NTR_TRACE_ROUTE", "0")
    try:
        for kernel, env in BODIES:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            nt.set_tunables()
            for any_hit in (False, True):
                ref_id, ref_t = refs[any_hit]
                for n in counts:
                    got, _ = gpu_trace(kernel, dbvh, rays[:n], any_hit)
                    where = "%s: %s %s any_hit=%s n=%d" % (what, kernel, env, any_hit, n)
                    bad = np.nonzero((got["id"] != ref_id[:n]) | (got["t"].view(np.uint32) != ref_t[:n].view(np.uint32)))[0]
                    assert bad.size == 0, "%s: %d records differ, first at ray %d: got (%d, %r) want (%d, %r)" % (
                        where, bad.size, bad[0], got["id"][bad[0]], got["t"][bad[0]], ref_id[bad[0]], ref_t[bad[0]])
            for k in env:
                monkeypatch.delenv(k, raising=False)
        assert nt.trace_status() == 0, what + ": the stack-overflow bit must stay clear"
    finally:
        for k in ("NTR_TRACE_ROUTE", "NTR_TRACE_MINIPOOL"):
            monkeypatch.delenv(k, raising=False)
        nt.set_tunables()


@pytest.mark.parametrize("flip", (0, 1))
def test_comb_drives_the_stack_across_the_lds_boundary_and_back(monkeypatch, flip):
    host = comb_tree(flip)
    assert host.nodes.nbytes == 64 * LEVELS and host.woop.nbytes == 16 * (4 * LEVELS + 1)
    rays = comb_rays(17 + flip)
    # (the depth the comb is built for, counted by the restatement itself: a full-length ray visits all 40 inner nodes)
    import np_tracer
    _, _, stats = np_tracer.trace(host.nodes, host.woop, host.tri_index, rays[64:65], any_hit=True, return_stats=True)
    assert stats["numInnerVisits"] == LEVELS and stats["numLeafVisits"] == LEVELS + 1 and stats["numHits"] == 0
    check(monkeypatch, host, rays, (64, 65, rays.shape[0]), "comb flip=%d" % flip)


def test_ragged_counts_with_a_leaf_at_the_end_of_triwoop(monkeypatch):
    from ray_sets import edge_rays
    host, cam = end_leaf_tree()
    edge = edge_rays()
    rays = np.concatenate([scenes.primary_rays(cam, 24, 16)[0], edge[:: max(1, edge.shape[0] // 300)][:300], scenes.random_rays(400, seed=3)])
    rays = rays[np.random.default_rng(9).permutation(rays.shape[0])][:1025]     # degenerate and edge rays in some lanes of every wave
    assert rays.shape[0] == 1025
    check(monkeypatch, host, rays, (1, 63, 64, 65, 255, 257, 1025), "end leaf")
