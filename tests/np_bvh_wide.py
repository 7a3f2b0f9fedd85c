"""The 4-wide BVH: the numpy spec of ntr_bvh_widen and ntr_trace_wide (test helper; this docstring is the normative text).

An extension without a reference counterpart.  A wide tree is a second node buffer over the leaves of a BVHLayout_Compact tree: the
Woop rows and triIndex are shared with the binary tree unchanged.

THE WIDE NODE is 32 words, 128 bytes, eight 16-byte rows:
  rows 0..2 (words 0..11)    the boxes of children 0 and 1, in Compact's box words: component j (lo.x hi.x lo.y hi.y lo.z hi.z) of
                             child k is word 4k + j for j < 4 and word 8 + 2k + (j - 4) otherwise
  row 3     (words 12..15)   the links of children 0..3
  rows 4..6 (words 16..27)   the boxes of children 2 and 3: 16 + Compact's box word for k - 2
  row 7     (words 28..31)   word 28 the child count (2..4), words 29..31 zero
A link < 0 is a leaf, ~link its first Woop row, copied verbatim from the binary tree; a link > 0 is 128 * index of a wide node; 0 is
an empty slot.  Slot k >= count has link 0 and a copy of slot 0's box, so every box word of the wide tree is a box word of the binary
tree.  The stack sentinel stays 0x76543210: a wide node buffer is a multiple of 128 bytes in [128, 0x76543200].

widen(nodes).  An *entry* is a link of the binary tree and the box stored beside it.  An entry is *inner* when its link names a node
slot: link > 0, a multiple of 64, link / 64 < numSlots (compact_bvh.h is_inner_link).
  1  The wide node of a kept binary slot b starts from the entry list E = [child 0 of b, child 1 of b].  Slot 0 is kept.
  2  While len(E) < 4 and some entry is inner: take the inner entry of largest area -- np_bvh_optimize.area's binary32 expression
     fl(fl(fl(dx*dy) + fl(dy*dz)) + fl(dz*dx)) over d = fl(hi - lo); areas are compared as floats (-0 == +0), a NaN area loses to
     every number, ties go to the lowest position in E -- and replace it, in place, by its node's child 0 followed by its child 1.
  3  The inner entries left in E are kept slots.
  4  The wide index of a kept slot is its rank among the kept slots in ascending binary slot index: the root is 0, the wide tree
     inherits the binary tree's node order, and the numbering does not depend on the order in which slots were processed.
  5  Slot k < len(E) of the wide node gets the box of E[k] and a link: a leaf link verbatim, a child word 0 as 0, an inner link as
     128 * wideIndex.  count = len(E).
  6  Malformed input.  A link > 0 that names no slot is written as 0 and the call reports a layout error after the work.  A slot named
     by several links is kept once.  The pass ends on any input: an expansion takes at most two steps and a slot is kept once.
A tree with more than 0x76543200 / 128 kept slots cannot be addressed: an overflow error, nothing written.

Statistics: numNodes; counts[3], the wide nodes with 2, 3 and 4 children; numLeafLinks, the negative links written; height, the wide
nodes on the longest root-to-leaf path; stackBound, the maximum over root-to-leaf paths of the sum of (count - 1), which is the most
entries a traversal can hold.  For a malformed input in which a slot is named by several links both are defined by levels: the slot
belongs to the first level (distance from the root in wide nodes) that names it, and carries the largest sum among that level's namers.

trace(wide, woop, tri_index, rays, any_hit) is np_tracer.trace with the inner step replaced.
  All four (mn_k, mx_k) are computed as ray_box2's GENERIC path has them (true division, select-form min / max, folded x, y, z).
  Child k is a candidate iff its link is non-zero and mn_k <= mx_k and mx_k >= tmin and mn_k <= tmax.
  Candidates are visited in ascending mn_k (compared as floats), ties by ascending k: the nearest becomes the node, the others are
  pushed farthest first; with no candidate the traversal pops.  A 2-child wide node therefore steps exactly as the binary rule does.
  Triangles, updateHit, any-hit termination, degenerate rays (tmin >= tmax: a miss without traversal) and the miss record
  (-1, ray.tmax, 0, 0) are np_tracer's and the device's, unchanged.  The stack holds 104 entries (16 in LDS + 88 in scratch).
  Stats: wide nodes visited, triangle tests, leaf terminators read and hits, in NtrTraceStats's fields.
KNOWN LIMIT: records may differ from the binary tracer's on the same tree.  A rounded box test is not conservative, so a triangle
within rounding of a box surface can be reached through one tree and culled in the other, and among hits of equal t the visiting order
decides.  This spec is the definition, not the binary tracer.
"""
import numpy as np

import np_bvh_optimize as opt

F = np.float32
FLT_MAX = np.float32(3.4028234663852886e38)
WIDE_WORDS, WIDE_BYTES = 32, 128
SENTINEL = 0x76543210
MAX_WIDE_BYTES = 0x76543200
MAX_STACK = 104
TERM = 0x80000000


class LayoutError(Exception):
    """widen's result is attached: the tree is written, with the offending links as empty slots."""

    def __init__(self, msg, result):
        Exception.__init__(self, msg)
        self.result = result


def box_word(k, j):
    """Compact's word of component j of child k (k < 2)."""
    return 4 * k + j if j < 4 else 8 + 2 * k + (j - 4)


def wide_box_word(k, j):
    return (16 if k >= 2 else 0) + box_word(k & 1, j)


BOX = [[box_word(k, j) for j in range(6)] for k in range(2)]
WBOX = [[wide_box_word(k, j) for j in range(6)] for k in range(4)]
LINK, WLINK, WCOUNT = 12, 12, 28


def _is_inner(c, S):
    return c > 0 and c % 64 == 0 and c // 64 < S


def _as_nodes(nodes):
    return np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16)


def expand(ni, areas, b):
    """Rules 1 and 2 for slot b -> the entry list [(link, source slot, source child)]."""
    S = ni.shape[0]
    E = [(int(ni[b, LINK + k]), b, k) for k in (0, 1)]
    while len(E) < 4:
        best = -1
        for p, (c, s, k) in enumerate(E):
            if not _is_inner(c, S):
                continue
            a = areas[s, k]
            if best < 0 or a > areas[E[best][1], E[best][2]] or (np.isnan(areas[E[best][1], E[best][2]]) and not np.isnan(a)):
                best = p
        if best < 0:
            break
        n = E[best][0] // 64
        E[best:best + 1] = [(int(ni[n, LINK]), n, 0), (int(ni[n, LINK + 1]), n, 1)]
    return E


def widen(nodes, strict=True):
    """-> dict(nodes int32[numNodes, 32], kept int64[numNodes] (the binary slot of each wide node), stats dict, bad_links).  With
    strict a malformed tree raises LayoutError (its .result is this dict)."""
    ni = _as_nodes(nodes)
    S = ni.shape[0]
    nf = ni.view(F)
    areas = np.stack([opt.area(nf[:, BOX[0]]), opt.area(nf[:, BOX[1]])], axis=1)
    level_of = np.zeros(S, np.int64)          # 1 + level of a kept slot, 0: not kept
    bound_in = np.zeros(S, np.int64)          # the sum of (count - 1) over the slot's ancestors
    entries = {}
    level_of[0] = 1
    frontier, level = [0], 1
    while frontier:
        nxt = []
        for b in frontier:
            E = expand(ni, areas, b)
            entries[b] = E
            for c, _, _ in E:
                if not _is_inner(c, S):
                    continue
                n = c // 64
                if level_of[n] == 0:
                    level_of[n] = level + 1
                    nxt.append(n)
                if level_of[n] == level + 1:
                    bound_in[n] = max(bound_in[n], bound_in[b] + len(E) - 1)
        frontier, level = sorted(nxt), level + 1
    kept = np.flatnonzero(level_of)
    if kept.size * WIDE_BYTES > MAX_WIDE_BYTES:
        raise OverflowError("np_bvh_wide: %d wide nodes cannot be addressed" % kept.size)
    rank = np.cumsum(level_of != 0) - 1
    out = np.zeros((kept.size, WIDE_WORDS), np.int32)
    counts, leaf_links, bad = [0, 0, 0], 0, 0
    stack_bound = 0
    for w, b in enumerate(kept):
        E = entries[int(b)]
        counts[len(E) - 2] += 1
        stack_bound = max(stack_bound, int(bound_in[b]) + len(E) - 1)
        for k in range(4):
            c, s, ck = E[k] if k < len(E) else (0, E[0][1], E[0][2])
            out[w, WBOX[k]] = ni[s, BOX[ck]]
            if c < 0:
                link = c
                leaf_links += 1
            elif _is_inner(c, S):
                link = WIDE_BYTES * int(rank[c // 64])
            else:
                link = 0
                bad += c != 0
            out[w, WLINK + k] = link
        out[w, WCOUNT] = len(E)
    stats = dict(numNodes=int(kept.size), counts=counts, numLeafLinks=leaf_links, height=int(level_of.max()), stackBound=stack_bound)
    res = dict(nodes=out, kept=kept, stats=stats, bad_links=int(bad))
    if bad and strict:
        raise LayoutError("np_bvh_wide: %d links name no slot" % bad, res)
    return res


def binary_height(nodes):
    """Inner nodes on the longest root-to-leaf path of the binary tree (reached slots only)."""
    return len(opt.levels_of(_as_nodes(nodes))) - 1


# ---- the trace ---------------------------------------------------------------------------------------------------------------------
def _smin(a, b):
    return np.where(a < b, a, b)


def _smax(a, b):
    return np.where(a > b, a, b)


def _dot4(a, bx, by, bz, bw):
    r = np.zeros_like(bx, dtype=F)
    r = r + a[:, 0] * bx
    r = r + a[:, 1] * by
    r = r + a[:, 2] * bz
    r = r + a[:, 3] * bw
    return r


def trace(wide, woop, tri_index, rays, any_hit=False, return_stats=False, probe=None):
    """-> (id, t, u, v) [, stats]: the four result words per ray.  probe: a dict that receives maxStack, the most entries any ray's
    stack held."""
    n_inner = n_tri = n_leaf = 0
    wf = np.frombuffer(np.ascontiguousarray(wide).tobytes(), dtype=F)
    wi = wf.view(np.int32)
    woop_f = np.frombuffer(np.ascontiguousarray(woop).tobytes(), dtype=F).reshape(-1, 4)
    woop_u = woop_f.view(np.uint32)
    tri_index = np.asarray(tri_index, dtype=np.int32)
    n = rays.shape[0]
    ox, oy, oz = rays["ox"].astype(F), rays["oy"].astype(F), rays["oz"].astype(F)
    dx, dy, dz = rays["dx"].astype(F), rays["dy"].astype(F), rays["dz"].astype(F)
    tmin = rays["tmin"].astype(F)
    tmax = rays["tmax"].astype(F).copy()
    res_id = np.full(n, -1, dtype=np.int32)
    res_u, res_v = np.zeros(n, F), np.zeros(n, F)
    node = np.zeros(n, dtype=np.int64)
    stack = np.zeros((n, MAX_STACK + 1), dtype=np.int64)
    stack[:, 0] = SENTINEL
    sp = np.ones(n, dtype=np.int64)
    done = ~(tmin < tmax)                                 # a degenerate ray is a miss without traversal
    one, zero = F(1.0), F(0.0)

    def pop(idx):
        sp[idx] -= 1
        node[idx] = stack[idx, sp[idx]]
        done[idx[node[idx] == SENTINEL]] = True

    def push(idx, v):
        if (sp[idx] > MAX_STACK).any():
            raise RuntimeError("np_bvh_wide: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1
        if probe is not None and idx.size:
            probe["maxStack"] = max(probe.get("maxStack", 0), int(sp[idx].max()) - 1)

    with np.errstate(all="ignore"):
        while not done.all():
            act = ~done
            # ---- one triangle (the cursor is the link: ~row, three rows further each step) ---------------------------------
            ti = np.nonzero(act & (node < 0))[0]
            inner = np.nonzero(act & (node >= 0))[0]
            if ti.size:
                a = ~node[ti]
                term = woop_u[a, 0] == TERM
                n_leaf += int(term.sum())
                pop(ti[term])
                ti, a = ti[~term], a[~term]
            if ti.size:
                n_tri += int(ti.size)
                z, u4, v4 = woop_f[a], woop_f[a + 1], woop_f[a + 2]
                rx, ry, rz = ox[ti], oy[ti], oz[ti]
                ex, ey, ez = dx[ti], dy[ti], dz[ti]
                Oz = z[:, 3] - rx * z[:, 0] - ry * z[:, 1] - rz * z[:, 2]
                ooDz = one / _dot4(z, ex, ey, ez, np.zeros_like(ex))
                t = Oz * ooDz
                ok = (t > tmin[ti]) & (t < tmax[ti])
                u = _dot4(u4, rx, ry, rz, np.full_like(rx, one)) + t * _dot4(u4, ex, ey, ez, np.full_like(rx, zero))
                ok &= (u >= 0)
                v = _dot4(v4, rx, ry, rz, np.full_like(rx, one)) + t * _dot4(v4, ex, ey, ez, np.full_like(rx, zero))
                ok &= (v >= 0) & ((u + v) <= one)
                tt = np.where(ok, t, FLT_MAX)
                acc = (tt > tmin[ti]) & (tt < tmax[ti])    # updateHit re-tests the returned t
                hi = ti[acc]
                tmax[hi] = tt[acc]
                res_id[hi] = tri_index[a[acc]]
                res_u[hi] = np.where(ok[acc], u[acc], zero)
                res_v[hi] = np.where(ok[acc], v[acc], zero)
                if any_hit:
                    done[hi] = True
                    ti, a = ti[~acc], a[~acc]
                nxt = woop_u[a + 3, 0] == TERM             # the terminator comes with the triangle
                n_leaf += int(nxt.sum())
                node[ti[~nxt]] -= 3
                pop(ti[nxt])
            # ---- one wide node ---------------------------------------------------------------------------------------------
            if inner.size:
                n_inner += int(inner.size)
                b = node[inner] // 4
                rx, ry, rz = ox[inner], oy[inner], oz[inner]
                ex, ey, ez = dx[inner], dy[inner], dz[inner]
                m = inner.size
                key = np.full((m, 4), np.inf, F)
                cand = np.zeros((m, 4), bool)
                links = np.zeros((m, 4), np.int64)
                for k in range(4):
                    g = [wf[b + w] for w in WBOX[k]]
                    t0x, t1x = (g[0] - rx) / ex, (g[1] - rx) / ex
                    t0y, t1y = (g[2] - ry) / ey, (g[3] - ry) / ey
                    t0z, t1z = (g[4] - rz) / ez, (g[5] - rz) / ez
                    mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
                    mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
                    links[:, k] = wi[b + WLINK + k]
                    cand[:, k] = (links[:, k] != 0) & (mn <= mx) & (mx >= tmin[inner]) & (mn <= tmax[inner])
                    key[:, k] = mn
                # candidates first, by ascending mn (a candidate's mn is no NaN; -0 + 0 == +0: floats compare, not words), ties by k
                order = np.lexsort((np.where(cand, np.arange(4), np.arange(4) + 4), np.where(cand, key + zero, F(np.inf))), axis=1)
                cnt = cand.sum(axis=1)
                rows = np.arange(m)
                for pos in (3, 2, 1):                       # farthest first
                    sel = cnt > pos
                    push(inner[sel], links[rows[sel], order[sel, pos]])
                sel = cnt > 0
                node[inner[sel]] = links[rows[sel], order[sel, 0]]
                pop(inner[~sel])
    out = (res_id, tmax, res_u, res_v)                    # t: the working tmax, which only an accepted hit changes
    if return_stats:
        return out + (dict(numRays=n, numInnerVisits=n_inner, numTriTests=n_tri, numLeafVisits=n_leaf, numHits=int((res_id >= 0).sum())),)
    return out
