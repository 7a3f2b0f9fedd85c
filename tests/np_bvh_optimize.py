"""The rules of ntr_bvh_optimize and ntr_bvh_sah_cost (csrc/bvh_optimize_kernels.hip) in vectorised numpy binary32.

optimize() is an EXTENSION: the reference has no treelet restructuring, so this docstring, not a reference line, is the normative
text (the algorithm is the treelet part of Karras and Aila, "Fast parallel construction of high-quality bounding volume hierarchies",
HPG 2013).  The device's node buffer equals this module's byte for byte.  sah_cost() restates the reference's calcSAHNode
(emitTreeKernel.cu:1361-1391) in strict binary32; see its own docstring.

Input of optimize: the node buffer of a BVHLayout_Compact tree (16 words per 64-byte slot -- c0 lo.x hi.x lo.y hi.y, c1 lo.x hi.x lo.y
hi.y, c0 lo.z hi.z, c1 lo.z hi.z, child 0, child 1, split word, a fourth word; an inner child is the byte offset 64 * index, a leaf
child ~row) and the number of passes (1..8).  Triangles are not looked at: leaves stay as they are, leaf links move between parents.
Treelet size n = 7.  Per pass:

1. Reached slots as in np_bvh_refit rule 1: the root (slot 0) and every slot named by an inner link of a reached slot.  An inner
   link is a positive child word that is a multiple of 64 and names a slot inside the buffer; every other child word (negative, 0,
   or pointing outside: the last is reported as bad_links) is a leaf link: it is never followed and cannot be expanded.
   height(slot) = 1 + the largest height of its inner children (0 for a leaf link); leafLinks(slot) = the leaf links in its subtree.
   Both are taken from the pass's input tree, once per pass.  Unreached slots are never written.
2. Every reached slot with leafLinks >= 7 roots a treelet; the roots are taken in ascending height.  A treelet only permutes slots
   and links inside its root's subtree, so two roots of equal height work on disjoint bytes: a height is one parallel step.
3. Formation at root R: the list starts as (child 0 of R, child 1 of R) with the boxes stored in R.  Until it has 7 entries: among
   the entries that are inner links the first one in list order is the candidate, and a later one replaces the candidate iff its area
   is greater (so ties go to the lowest list position and a NaN area never replaces); the candidate's child 0 takes its place, its
   child 1 is appended, with the boxes stored in the candidate's node; its slot joins the treelet's internal slots.
4. Area of a box, binary32, no FMA contraction: d = fl(hi - lo) per axis, a = fl(fl(fl(dx*dy) + fl(dy*dz)) + fl(dz*dx)).  The box
   of a subset of entries is the per-axis min (lo) / max (hi) in the float-order integer encoding (np_hlbvh.f2i, the device's
   ord_enc; -0 < +0), so it does not depend on operand order.
5. Dynamic programme over the 127 non-empty subsets s of the 7 entries (entry i is bit i): c[s] = 0 for one entry, else
   c[s] = fl(a[s] + best), where p ranges in ascending numerical order over the proper subsets of s that hold s's lowest entry,
   best starts as +inf with the first p as the choice, and a later p replaces it iff fl(c[p] + c[s ^ p]) < best (ties stay with
   the lowest mask; a comparison with a NaN is false, a NaN never wins).
6. Only strict improvements.  c_orig is the same recurrence along the treelet's existing topology (each internal node: fl(a[its
   entries] + fl(c_orig[child 0's entries] + c_orig[child 1's entries])), 0 for one entry).  It is one of the programme's candidates,
   so c[full] <= c_orig in binary32.  The treelet is rewritten iff c[full] < c_orig; otherwise none of its bytes change.
7. Emission.  R stays the root (its parent's link and box are not written).  The other five internal slots are handed out in
   ascending slot index to the new inner nodes in preorder, child 0's subtree first.  Child 0 of a node over s is the chosen part p
   (the one with s's lowest entry), child 1 is s ^ p.  A rewritten record gets the two parts' boxes (rule 4; an entry's own box words
   for a single entry), the two links (the entry's original link word for a single entry, 64 * slot otherwise), split word 0, and
   keeps its fourth word.  All six records of a rewritten treelet are written.

Returns the nodes and per pass: treelets formed and rewritten, the tree's height before and after.
"""
import numpy as np

import np_bvh_refit as rf

np_hlbvh = rf.np_hlbvh
F = np.float32
TERM = 0x80000000
N = 7                                   # treelet size
FULL = (1 << N) - 1
BOX_WORDS = rf.BOX_WORDS
LO, HI = rf.LO, rf.HI
POPC = np.array([bin(s).count("1") for s in range(FULL + 1)])


def inner_mask(c, num_slots):
    """Which child words are inner links (rule 1)."""
    c = c.astype(np.int64)
    return (c > 0) & (c % 64 == 0) & (c // 64 < num_slots)


def levels_of(ni):
    """Reached node slots by depth (rule 1's notion of an inner link): a list of index arrays, [0] first."""
    S = ni.shape[0]
    seen = np.zeros(S, bool)
    seen[0] = True
    levels = [np.array([0], np.int64)]
    while levels[-1].size:
        c = ni[levels[-1], 12:14].reshape(-1).astype(np.int64)
        nxt = c[inner_mask(c, S)] // 64
        assert not seen[nxt].any() and np.unique(nxt).size == nxt.size, "not a tree"
        seen[nxt] = True
        levels.append(nxt)
    return levels[:-1]


def topology(ni):
    """(levels, height[S], leafLinks[S], bad_links) of the reached slots; height and leafLinks are 0 for unreached slots."""
    S = ni.shape[0]
    levels = levels_of(ni)
    height = np.zeros(S, np.int64)
    leaf_links = np.zeros(S, np.int64)
    bad = 0
    for slots in reversed(levels):
        c = ni[slots, 12:14].astype(np.int64)
        inner = inner_mask(c, S)
        bad += int(((c > 0) & ~inner).sum())
        ch = np.where(inner, c // 64, 0)
        height[slots] = 1 + np.where(inner, height[ch], 0).max(axis=1)
        leaf_links[slots] = np.where(inner, leaf_links[ch], 1).sum(axis=1)
    return levels, height, leaf_links, bad


def area(box):
    """Rule 4 on [..., 6] float32 boxes (lo.x hi.x lo.y hi.y lo.z hi.z)."""
    with np.errstate(all="ignore"):
        d = (box[..., HI] - box[..., LO]).astype(F)
        return (((d[..., 0] * d[..., 1]).astype(F) + (d[..., 1] * d[..., 2]).astype(F)).astype(F) + (d[..., 2] * d[..., 0]).astype(F)).astype(F)


def _child_boxes(nf, slots):
    """[m, 2, 6] boxes stored in the nodes `slots`."""
    return np.stack([nf[slots][:, BOX_WORDS[0]], nf[slots][:, BOX_WORDS[1]]], axis=1)


def _partitions(s):
    low = s & -s
    rest = s ^ low
    return np.array([low | q for q in range(rest) if (q & rest) == q], np.int64)   # ascending; q == rest (p == s) is left out


_PARTS = {s: _partitions(s) for s in range(1, FULL + 1) if POPC[s] > 1}
_BY_SIZE = sorted((s for s in range(1, FULL + 1) if POPC[s] > 1), key=lambda s: (POPC[s], s))


def treelets(ni, roots):
    """Rules 3-6 for the treelet roots `roots` (disjoint subtrees) on the tree ni.  Returns dict(link [m, 7], box_i [m, 7, 6] in the
    f2i encoding, slots [m, 5] the internal slots other than the root in formation order, c [m, 128], choice [m, 128], c_orig [m],
    sub_i [m, 128, 6] the subsets' boxes in the f2i encoding)."""
    S = ni.shape[0]
    nf = ni.view(F)
    m = roots.size
    link = np.zeros((m, N), np.int64)
    box = np.zeros((m, N, 6), F)
    link[:, :2] = ni[roots, 12:14]
    box[:, :2] = _child_boxes(nf, roots)
    slots = np.zeros((m, N - 2), np.int64)
    # entries under child 0 / child 1 of the internal nodes, as bit masks; node 0 is the root
    m0 = np.zeros((m, N - 1), np.int64)
    m1 = np.zeros((m, N - 1), np.int64)
    m0[:, 0], m1[:, 0] = 1, 2
    rows = np.arange(m)
    for n in range(2, N):
        inner = inner_mask(link[:, :n], S)
        assert inner.any(axis=1).all(), "leafLinks >= 7 guarantees an inner entry"
        a = area(box[:, :n])
        cand = np.full(m, -1)
        for e in range(n):
            with np.errstate(invalid="ignore"):
                take = inner[:, e] & ((cand < 0) | (a[:, e] > a[rows, np.maximum(cand, 0)]))
            cand = np.where(take, e, cand)
        x = link[rows, cand] // 64
        slots[:, n - 2] = x
        cb = _child_boxes(nf, x)
        link[rows, cand], link[:, n] = ni[x, 12], ni[x, 13]
        box[rows, cand], box[:, n] = cb[:, 0], cb[:, 1]
        bit, new = 1 << cand, 1 << n
        m0[:, :n - 1] |= np.where(m0[:, :n - 1] & bit[:, None], new, 0)
        m1[:, :n - 1] |= np.where(m1[:, :n - 1] & bit[:, None], new, 0)
        m0[:, n - 1], m1[:, n - 1] = bit, new
    box_i = np_hlbvh.f2i(box).astype(np.int64)
    sub_i = np.zeros((m, FULL + 1, 6), np.int64)
    for s in range(1, FULL + 1):
        e = (s & -s).bit_length() - 1
        r = s & (s - 1)
        if r == 0:
            sub_i[:, s] = box_i[:, e]
        else:
            sub_i[:, s][:, LO] = np.minimum(sub_i[:, r][:, LO], box_i[:, e][:, LO])
            sub_i[:, s][:, HI] = np.maximum(sub_i[:, r][:, HI], box_i[:, e][:, HI])
    a = area(np_hlbvh.i2f(sub_i.astype(np.int32)).astype(F))                      # [m, 128]
    c = np.zeros((m, FULL + 1), F)
    choice = np.zeros((m, FULL + 1), np.int64)
    with np.errstate(all="ignore"):
        for s in _BY_SIZE:
            ps = _PARTS[s]
            v = (c[:, ps] + c[:, s ^ ps]).astype(F)
            v = np.where(np.isnan(v), F(np.inf), v)
            j = np.argmin(v, axis=1)                                               # the first minimum: the lowest mask
            choice[:, s] = ps[j]
            c[:, s] = (a[:, s] + v[rows, j]).astype(F)
        co = np.zeros((m, FULL + 1), F)
        for i in range(N - 2, -1, -1):                                             # children are formed after their parents
            s0, s1 = m0[:, i], m1[:, i]
            co[rows, s0 | s1] = (a[rows, s0 | s1] + (co[rows, s0] + co[rows, s1]).astype(F)).astype(F)
    assert (m0[:, 0] | m1[:, 0] == FULL).all()
    return dict(link=link, box_i=box_i, slots=slots, c=c, choice=choice, c_orig=co[:, FULL], sub_i=sub_i)


def emit(ni, roots, t, sel):
    """Rule 7 for the treelets sel (a boolean mask over roots)."""
    roots, link, slots, choice, sub_i = roots[sel], t["link"][sel], t["slots"][sel], t["choice"][sel], t["sub_i"][sel]
    m = roots.size
    if not m:
        return
    rows = np.arange(m)
    order = np.concatenate([roots[:, None], np.sort(slots, axis=1)], axis=1)      # slot of the node with preorder index i
    subset = np.zeros((m, N - 1), np.int64)
    subset[:, 0] = FULL
    sub_f = np_hlbvh.i2f(sub_i.astype(np.int32)).view(np.int32)                    # box words of every subset
    for i in range(N - 1):
        s = subset[:, i]
        assert (POPC[s] > 1).all()
        p = choice[rows, s]
        parts = (p, s ^ p)
        idx = (np.full(m, i + 1), i + 1 + np.maximum(POPC[p] - 1, 0))             # preorder index of an inner child
        slot = order[:, i]
        fourth = ni[slot, 15].copy()
        for k in (0, 1):
            q = parts[k]
            single = POPC[q] == 1
            e = np.array([int(v).bit_length() - 1 for v in (q & -q)])
            j = np.minimum(idx[k], N - 2)
            subset[rows[~single], j[~single]] = q[~single]
            ni[slot[:, None], BOX_WORDS[k][None, :]] = sub_f[rows, q]
            ni[slot, 12 + k] = np.where(single, link[rows, e], 64 * order[rows, j]).astype(np.int32)
        ni[slot, 14] = 0
        ni[slot, 15] = fourth


def optimize(nodes, passes=1, detail=False):
    """Returns dict(nodes int32[slots, 16], passes: a list of dict(formed, rewritten, heightBefore, heightAfter), bad_links); with
    detail=True each pass also carries roots, rewritten_mask, c_full and c_orig over all its treelets."""
    assert 1 <= passes <= 8
    ni = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16).copy()
    out = []
    levels, height, leaf_links, bad = topology(ni)
    for _ in range(passes):
        reached = np.concatenate(levels)
        roots_all = reached[leaf_links[reached] >= N]
        info = dict(formed=int(roots_all.size), rewritten=0, heightBefore=int(height[0]))
        det = dict(roots=[], rewritten_mask=[], c_full=[], c_orig=[])
        for h in np.unique(height[roots_all]):
            roots = np.sort(roots_all[height[roots_all] == h])
            t = treelets(ni, roots)
            with np.errstate(invalid="ignore"):
                sel = t["c"][:, FULL] < t["c_orig"]
            emit(ni, roots, t, sel)
            info["rewritten"] += int(sel.sum())
            det["roots"].append(roots); det["rewritten_mask"].append(sel)
            det["c_full"].append(t["c"][:, FULL]); det["c_orig"].append(t["c_orig"])
        levels, height, leaf_links, _ = topology(ni)
        info["heightAfter"] = int(height[0])
        if detail:
            info.update({k: (np.concatenate(v) if v else np.zeros(0)) for k, v in det.items()})
        out.append(info)
    return dict(nodes=ni, passes=out, bad_links=bad)


# ---- SAH cost -----------------------------------------------------------------------------------------------------------

def _fmin(a, b):
    """fminf: the other operand for a NaN, else the smaller in the f2i order (-0 < +0)."""
    r = np.where(np_hlbvh.f2i(a) <= np_hlbvh.f2i(b), a, b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, r))


def _fmax(a, b):
    r = np.where(np_hlbvh.f2i(a) >= np_hlbvh.f2i(b), a, b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, r))


def sah_cost(nodes, woop, dtype=F):
    """calcSAHNode(0) of the reference (emitTreeKernel.cu:1361-1391; host HLBVHBuilder::calcSAHGPU, HLBVHBuilder.cpp:752-770) in strict
    binary32 in source order (the reference compiles it -use_fast_math and so defines no bits).  Per reached node, on the box words as
    stored: xi = fminf(c0 lo.x, c1 lo.x), xa = fmaxf(c0 hi.x, c1 hi.x), likewise y and z;
    pa = fl(2 * fl(fl(fl(dx*dy) + fl(dy*dz)) + fl(dz*dx))) with dx = fl(xa - xi) ..., pl and pr the same over child 0's and child 1's
    own box; a leaf child's value is its number of triangles (row groups up to the terminator, calcLeafs), an inner child's value is
    that node's; a child word that is neither (0, or a link outside the buffer) has value 0.  The node's value is
    fl(fl(1 + fl(fl(pl / pa) * l)) + fl(fl(pr / pa) * r)) with the correctly rounded divide; zero areas give infinities and NaNs as IEEE
    does.  dtype=np.float64 evaluates the same formula in binary64 on the binary32 box words (for comparisons of tree quality).
    Returns dict(sahCost, numNodes (reached slots), numLeaves (negative child words of reached slots), numTris, height)."""
    ni = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16)
    nf = ni.view(F)
    w = np.ascontiguousarray(woop).reshape(-1).view(np.uint32).reshape(-1, 4)
    S = ni.shape[0]
    levels, height, _, _ = topology(ni)
    T = dtype
    val = np.zeros(S, T)
    tris = 0
    leaves = 0

    def ar(lox, hix, loy, hiy, loz, hiz):
        dx, dy, dz = (hix.astype(T) - lox.astype(T)).astype(T), (hiy.astype(T) - loy.astype(T)).astype(T), (hiz.astype(T) - loz.astype(T)).astype(T)
        return (T(2) * (((dx * dy).astype(T) + (dy * dz).astype(T)).astype(T) + (dz * dx).astype(T)).astype(T)).astype(T)

    with np.errstate(all="ignore"):
        for slots in reversed(levels):
            b = _child_boxes(nf, slots)                                           # [m, 2, 6]
            pa = ar(_fmin(b[:, 0, 0], b[:, 1, 0]), _fmax(b[:, 0, 1], b[:, 1, 1]), _fmin(b[:, 0, 2], b[:, 1, 2]),
                    _fmax(b[:, 0, 3], b[:, 1, 3]), _fmin(b[:, 0, 4], b[:, 1, 4]), _fmax(b[:, 0, 5], b[:, 1, 5]))
            v = []
            for k in (0, 1):
                c = ni[slots, 12 + k].astype(np.int64)
                inner = inner_mask(c, S)
                cnt = np.zeros(slots.size, np.int64)
                leaf = np.flatnonzero(c < 0)
                cur = ~c[leaf]
                while leaf.size:
                    live = w[cur, 0] != TERM
                    leaf, cur = leaf[live], cur[live] + 3
                    cnt[leaf] += 1
                tris += int(cnt.sum())
                leaves += int((c < 0).sum())
                v.append(np.where(inner, val[np.where(inner, c // 64, 0)], cnt.astype(T)).astype(T))
            pl, pr = ar(*[b[:, 0, j] for j in range(6)]), ar(*[b[:, 1, j] for j in range(6)])
            val[slots] = ((T(1) + ((pl / pa).astype(T) * v[0]).astype(T)).astype(T) + ((pr / pa).astype(T) * v[1]).astype(T)).astype(T)
    return dict(sahCost=T(val[0]), numNodes=int(sum(s.size for s in levels)), numLeaves=leaves, numTris=tris, height=int(height[0]))
