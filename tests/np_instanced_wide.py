"""numpy spec of the two-level trace over 4-wide trees: ntr_pool_widen, ntr_tlas_widen, ntr_trace_instanced_wide and
ntr_trace_instanced_wide_stats (test helper; this docstring is the normative text).

EXTENSION: the reference has neither instancing nor wide trees.  The spec joins tests/np_instanced_masked.py (the two-level rule with
visibility masks and counters) and tests/np_bvh_wide.py (the 4-wide node, its widening and its step); the device
(csrc/instanced_widen_kernels.hip, csrc/trace_instanced_wide_kernels.hip) equals widen_pool() and widen_tlas() byte for byte and trace()
in all four result words, the instance id and every counter.  Arithmetic is binary32 without contraction, GENERIC only.

Data.
  wide pool    ONE more node buffer beside the pool (np_instanced.make_pool); the pool's triWoop and triIndex are used unchanged.  Wide
               BLAS k is np_bvh_wide.widen applied to the bytes [nodesOffset_k, +nodesBytes_k) of the pool's nodes, and lies at the sum
               of the exact wide extents (128 * numNodes) of the BLASes before it: every offset is a multiple of 128, there are no gaps,
               and links stay relative to the BLAS's own start.  The buffer is at most 0xFFFFFF00 bytes.
  wide TLAS    np_bvh_wide.widen applied to the top-level node buffer of np_instanced.tlas_build.  Leaf links ~i are negative and pass
               through verbatim, as a Compact leaf link does.  N == 1: there is no node and the root link stays ~0.
  wide record  16 words: 0..11 worldToObject, 12 the wide BLAS's offset in the wide pool, 13 triWoopOffset / 16 (as the binary
               record), 14 the wide BLAS's extent, 15 zero.  An instance whose blas index lies outside [0, numBlas) gets words 12..14
               zero: with extent 0 nothing of it is ever read (see "bottom level, wide node").
  stackBound   of a widened scene: the wide TLAS's stackBound (0 for N == 1) + 1 (the exit marker) + the largest stackBound of any
               wide BLAS of the pool.  A bound of at most 104 guarantees that no ray's stack overflows.

trace(wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit, inst_masks, ray_masks, ray_mask)
  is np_instanced_masked.trace with its two inner steps replaced by np_bvh_wide's wide-node step.
  top level, wide node     the 32 words at byte `node` of the wide TLAS (words beyond its extent read as zero), with the world ray W
  bottom level, wide node  the 32 words at byte offset + node of the wide pool, with the current ray R -- read only if node < extent
                           (unsigned) and offset + node < 0xFFFFFF00; otherwise, and beyond the pool's end, the words read as zero
  the wide-node step       all four (mn_k, mx_k) as ray_box2's GENERIC path has them (true division, select-form min / max, folded
                           x, y, z); child k is a candidate iff its link is non-zero and mn_k <= mx_k and mx_k >= tmin and
                           mn_k <= tmax; candidates are visited in ascending (mn_k, k), mn compared as floats: the nearest becomes
                           the node, the others are pushed farthest first; with no candidate -- a node of zeros among them -- the
                           traversal pops
  unchanged                entering an instance (push the exit marker, R = xform(worldToObject, W), node 0 of the instance; the record's
                           words 12, 13, 14 become offset, row offset and extent), the mask rule, a link ~i with i outside
                           [0, numInstances) (popped), popping the exit marker (R = W, pop again), triangles and updateHit, any hit,
                           the miss record (id -1, t = ray.tmax, u = v = 0, instance -1), degenerate rays (!(tmin < tmax): a miss
                           without traversal), the stack of 104 entries (the device's 16 + 88; the spec raises beyond).
Counters: np_instanced_masked's eight, where numTopInnerVisits and numInnerVisits count wide-node steps.
Algorithmic bytes: 52 numRays + 112 (numTopInnerVisits + numInnerVisits) + 64 numInstanceEntries + 32 numInstanceEntries
  + 48 numTriTests + 16 numLeafVisits + 4 numHits, plus 4 (numInstanceEntries + numInstancesMasked) with instance masks and 4 numRays
  with per-ray masks (112: the seven rows a wide node's step fetches; row 7, the child count, is for the host).
KNOWN LIMIT, np_bvh_wide's: the records may differ from the binary two-level trace's (np_instanced.trace) on the same scene.  A rounded
box test is not conservative, so a triangle within rounding of a box surface can be reached through one tree and culled in the other,
and among hits of equal t the visiting order decides.  This spec is the definition, not the binary trace.
"""
import numpy as np

import np_bvh_wide as bw
from np_instanced import EXIT_MARKER, F, FLT_MAX, MAX_STACK, SENTINEL, _dot4, _smax, _smin, xform
from np_instanced_masked import COUNTERS, is_terminator, visible

WIDE_BYTES = bw.WIDE_BYTES
POOL_MAX_BYTES = 0xFFFFFF00
NO_NODE = 0xFFFFFF00


def algorithmic_bytes(c, instance_masks=False, ray_masks=False):
    n = (52 * c["numRays"] + 112 * (c["numTopInnerVisits"] + c["numInnerVisits"]) + 64 * c["numInstanceEntries"] + 32 * c["numInstanceEntries"]
         + 48 * c["numTriTests"] + 16 * c["numLeafVisits"] + 4 * c["numHits"])
    return n + (4 * (c["numInstanceEntries"] + c["numInstancesMasked"]) if instance_masks else 0) + (4 * c["numRays"] if ray_masks else 0)


# ---- widening -------------------------------------------------------------------------------------------------------------------------
def widen_pool(pool):
    """pool: np_instanced.make_pool's dict -> dict(nodes uint8 (the wide pool), ranges: a list of (offset, bytes, numNodes, stackBound)
    per BLAS, stats: nodesBytes, numNodes, counts, numLeafLinks (sums), height, stackBound (the largest of any BLAS))."""
    nodes = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1)
    parts, ranges = [], []
    stats = dict(nodesBytes=0, numNodes=0, counts=[0, 0, 0], numLeafLinks=0, height=0, stackBound=0)
    off = 0
    for n_off, n_bytes, _, _ in pool["ranges"]:
        w = bw.widen(nodes[n_off:n_off + n_bytes])
        s = w["stats"]
        ext = WIDE_BYTES * s["numNodes"]
        parts.append(w["nodes"].view(np.uint8).reshape(-1))
        ranges.append((off, ext, s["numNodes"], s["stackBound"]))
        off += ext
        stats["numNodes"] += s["numNodes"]
        stats["counts"] = [a + b for a, b in zip(stats["counts"], s["counts"])]
        stats["numLeafLinks"] += s["numLeafLinks"]
        stats["height"] = max(stats["height"], s["height"])
        stats["stackBound"] = max(stats["stackBound"], s["stackBound"])
    assert off <= POOL_MAX_BYTES
    stats["nodesBytes"] = off
    return dict(nodes=np.concatenate(parts), ranges=ranges, stats=stats)


def widen_tlas(tlas_nodes, root_link, inst, blas_ranges, wide_ranges):
    """tlas_nodes, root_link: np_instanced.tlas_build's; inst: the INSTANCE_DTYPE array; blas_ranges: the pool's; wide_ranges:
    widen_pool's.  -> dict(nodes int32 (M, 32), root_link, records uint32 (N, 16), stats: np_bvh_wide's of the top level plus
    tlasStackBound and stackBound (the scene's))."""
    n = inst.shape[0]
    if int(root_link) < 0:
        nodes = np.zeros((0, bw.WIDE_WORDS), np.int32)
        stats = dict(numNodes=0, counts=[0, 0, 0], numLeafLinks=0, height=0, stackBound=0)
    else:
        w = bw.widen(tlas_nodes)
        nodes, stats = w["nodes"], dict(w["stats"])
    records = np.zeros((n, 16), np.uint32)
    records[:, :12] = inst["worldToObject"].view(np.uint32)
    for i, b in enumerate(inst["blas"]):
        if 0 <= int(b) < len(wide_ranges):
            records[i, 12], records[i, 13], records[i, 14] = wide_ranges[int(b)][0], blas_ranges[int(b)][2] // 16, wide_ranges[int(b)][1]
    stats["tlasStackBound"] = stats["stackBound"]
    stats["stackBound"] = stats["tlasStackBound"] + 1 + max(r[3] for r in wide_ranges)
    return dict(nodes=nodes, root_link=int(root_link), records=records, stats=stats)


# ---- the two-level trace over wide nodes ------------------------------------------------------------------------------------------------
def trace(wide_tlas, root_link, wide_records, pool, wide_pool, rays, any_hit=False, inst_masks=None, ray_masks=None, ray_mask=0xFFFFFFFF,
          probe=None):
    """wide_pool: widen_pool's dict, or the wide pool's bytes.  -> (id int32, t float32, u float32, v float32, instance int32, counters
    dict).  probe: a dict that receives maxStack, the most entries any ray's stack held."""
    def padded(buf):                                   # a zero node behind the extent: what a read beyond it gives
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        return np.concatenate([b, np.zeros(2 * WIDE_BYTES, np.uint8)]).view(F), b.size
    tl, tl_bytes = padded(wide_tlas)
    wp, wp_bytes = padded(wide_pool["nodes"] if isinstance(wide_pool, dict) else wide_pool)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(wide_records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
    num_inst = rec.shape[0]
    M = np.full(num_inst, 0xFFFFFFFF, np.uint32) if inst_masks is None else np.ascontiguousarray(inst_masks).view(np.uint32).reshape(-1)
    m = np.full(n, int(ray_mask) & 0xFFFFFFFF, np.uint32) if ray_masks is None else np.ascontiguousarray(ray_masks).view(np.uint32).reshape(-1)
    assert M.shape[0] == num_inst and m.shape[0] == n
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["numRays"] = n
    W = [rays[k].astype(F) for k in ("ox", "oy", "oz", "dx", "dy", "dz")]
    R = [w.copy() for w in W]
    tmin = rays["tmin"].astype(F)
    tmax = rays["tmax"].astype(F).copy()
    res_id = np.full(n, -1, np.int32)
    res_inst = np.full(n, -1, np.int32)
    res_t = tmax.copy()
    res_u = np.zeros(n, F)
    res_v = np.zeros(n, F)
    node = np.full(n, int(root_link), np.int64)
    inst = np.full(n, -1, np.int64)
    w_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    w_ext = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced_wide: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1
        if probe is not None and idx.size:
            probe["maxStack"] = max(probe.get("maxStack", 0), int(sp[idx].max()))

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

    def wide(idx, buf, byte):
        """np_bvh_wide's wide-node step for rays idx on the nodes at `byte` of buf."""
        b = byte // 4
        bi = buf.view(np.int32)
        rx, ry, rz, ex, ey, ez = (a[idx] for a in R)
        k_n = idx.size
        key = np.full((k_n, 4), np.inf, F)
        cand = np.zeros((k_n, 4), bool)
        links = np.zeros((k_n, 4), np.int64)
        for k in range(4):
            g = [buf[b + w] for w in bw.WBOX[k]]
            t0x, t1x = (g[0] - rx) / ex, (g[1] - rx) / ex
            t0y, t1y = (g[2] - ry) / ey, (g[3] - ry) / ey
            t0z, t1z = (g[4] - rz) / ez, (g[5] - rz) / ez
            mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
            mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
            links[:, k] = bi[b + bw.WLINK + k]
            cand[:, k] = (links[:, k] != 0) & (mn <= mx) & (mx >= tmin[idx]) & (mn <= tmax[idx])
            key[:, k] = mn
        # candidates first, by ascending mn (a candidate's mn is no NaN; -0 + 0 == +0: floats compare, not words), ties by k
        order = np.lexsort((np.where(cand, np.arange(4), np.arange(4) + 4), np.where(cand, key + F(0), F(np.inf))), axis=1)
        c = cand.sum(axis=1)
        rows = np.arange(k_n)
        for pos in (3, 2, 1):                       # farthest first
            sel = c > pos
            push(idx[sel], links[rows[sel], order[sel, pos]])
        sel = c > 0
        node[idx[sel]] = links[rows[sel], order[sel, 0]]
        pop(idx[~sel])

    with np.errstate(all="ignore"):
        while True:
            act = node != SENTINEL
            if not act.any():
                break
            is_exit = act & (node == EXIT_MARKER)
            is_inner = act & (node >= 0) & (node < SENTINEL)
            top = inst < 0
            k_top_inner = np.flatnonzero(is_inner & top)
            k_enter = np.flatnonzero(act & (node < 0) & top)
            k_bot_inner = np.flatnonzero(is_inner & ~top)
            k_tri = np.flatnonzero(act & (node < 0) & ~top)
            k_exit = np.flatnonzero(is_exit)
            k_other = np.flatnonzero(act & (node > SENTINEL) & ~is_exit)      # a positive word that is no link: dropped
            assert k_top_inner.size + k_enter.size + k_bot_inner.size + k_tri.size + k_exit.size + k_other.size == int(act.sum())
            cnt["numTopInnerVisits"] += k_top_inner.size
            cnt["numInnerVisits"] += k_bot_inner.size
            if k_top_inner.size:
                wide(k_top_inner, tl, np.minimum(node[k_top_inner], tl_bytes))
            if k_bot_inner.size:
                nd = node[k_bot_inner]
                o = w_off[k_bot_inner] + nd
                readable = (nd < w_ext[k_bot_inner]) & (o < NO_NODE)
                wide(k_bot_inner, wp, np.where(readable, np.minimum(o, wp_bytes), wp_bytes))
            if k_other.size:
                pop(k_other)
            if k_enter.size:
                i = ~node[k_enter]
                in_range = (i >= 0) & (i < num_inst)
                pop(k_enter[~in_range])                       # no instance: popped, counted as nothing, its mask never read
                k_enter, i = k_enter[in_range], i[in_range]
                seen = visible(M, m, i, k_enter)
                cnt["numInstancesMasked"] += int((~seen).sum())
                pop(k_enter[~seen])                           # refused: no marker, no transform; tmax, hit and instance untouched
                k_enter, i = k_enter[seen], i[seen]
                cnt["numInstanceEntries"] += k_enter.size
            if k_enter.size:
                push(k_enter, EXIT_MARKER)
                m_i = rec_f[i, :12]
                o = xform(m_i, W[0][k_enter], W[1][k_enter], W[2][k_enter], 1)
                d = xform(m_i, W[3][k_enter], W[4][k_enter], W[5][k_enter], 0)
                for a in range(3):
                    R[a][k_enter] = o[a]
                    R[3 + a][k_enter] = d[a]
                inst[k_enter] = i
                w_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                w_ext[k_enter] = rec[i, 14]
                node[k_enter] = 0
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                pop(k_exit)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = is_terminator(pw_u, row)
                cnt["numLeafVisits"] += int(term.sum())
                cnt["numTriTests"] += int((~term).sum())
                pop(k_tri[term])
                ti, a = k_tri[~term], row[~term]
                if ti.size:
                    z, u4, v4 = pw[a], pw[a + 1], pw[a + 2]
                    rx, ry, rz, ex, ey, ez = (q[ti] for q in R)
                    one, zero = np.full_like(rx, F(1)), np.zeros_like(rx)
                    Oz = z[:, 3] - rx * z[:, 0] - ry * z[:, 1] - rz * z[:, 2]
                    ooDz = F(1) / _dot4(z, ex, ey, ez, zero)
                    t = Oz * ooDz
                    ok = (t > tmin[ti]) & (t < tmax[ti])
                    u = _dot4(u4, rx, ry, rz, one) + t * _dot4(u4, ex, ey, ez, zero)
                    ok &= u >= 0
                    v = _dot4(v4, rx, ry, rz, one) + t * _dot4(v4, ex, ey, ez, zero)
                    ok &= (v >= 0) & ((u + v) <= F(1))
                    tt = np.where(ok, t, FLT_MAX)
                    acc = (tt > tmin[ti]) & (tt < tmax[ti])
                    # (a missed test that updateHit accepts at t = FLT_MAX -- tmax = +inf -- records u = v = 0, as np_tracer's t)
                    h = ti[acc]
                    tmax[h] = tt[acc]
                    res_t[h] = tt[acc]
                    res_u[h] = np.where(ok[acc], u[acc], F(0))
                    res_v[h] = np.where(ok[acc], v[acc], F(0))
                    res_id[h] = tri_index[a[acc]]
                    res_inst[h] = inst[h]
                    node[ti] -= 3                              # (the row after a triangle is read by the next step: a terminator pops)
                    if any_hit:
                        node[h] = SENTINEL
    cnt["numHits"] = int((res_id != -1).sum())
    return res_id, res_t, res_u, res_v, res_inst, cnt
