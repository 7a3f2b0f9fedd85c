"""The rule of the on-device BVH renumbering (ntr_bvh_reorder, csrc/bvh_reorder_kernels.hip) in numpy.  The pass is an EXTENSION as a
call of its own, but the order it produces is the host builder's: the walk of CudaBVH::createCompact (host/CudaBVH.cpp; reference
CudaBVH.cpp:594-652), restated here over the Compact tree itself.  This docstring is the normative text.  The device's three output
buffers equal this module's byte for byte.

Input: a BVHLayout_Compact tree -- nodes (16 words per 64-byte slot; words 12 and 13 are the links of child 0 and child 1), triWoop
(16-byte rows) and triIndex (a word per row), with their byte extents.  numSlots = nodes bytes / 64, numRows = triWoop bytes / 16.

1. Links are classified as csrc/bvh_climb.h does.  A word c is LINK_NONE if c == 0 (the root's offset names nobody: the one-triangle
   tree's empty child 0), LINK_LEAF if c < 0 (the leaf's first row is ~c), LINK_INNER if c > 0, c % 64 == 0 and c / 64 < numSlots
   (the slot c / 64), and LINK_BAD otherwise.
2. Reached, as in np_bvh_refit.py: slot 0, and every slot an inner link of a reached slot names.  The reached slots must form a tree
   (every reached slot other than 0 named by exactly one inner link of a reached slot, no cycle); anything else is out of contract:
   this module asserts, and the device returns NTR_ERR_LAYOUT having written nothing (it ends on any input).
3. Leaf length.  A leaf's rows are read from row r = ~link in steps of three rows, as the tracer reads them: the leaf ends at the first
   row among r, r + 3, r + 6, ... whose x word is 0x80000000.  That row is the terminator and belongs to the leaf, so a leaf of t
   triangles has 3 t + 1 rows.  Only the first row of each triangle is tested: the second and third Woop rows of an axis-aligned
   triangle legitimately hold -0.0f in x.  A leaf whose scan leaves the triWoop extent (a row >= numRows before a terminator) is
   malformed: its length is 1.
4. Order.  A stack holding slot 0, nextSlot = 1, nextRow = 0.  Pop a slot v (the last pushed); for child 0, then child 1: an inner
   child takes slot nextSlot++ and is pushed; a leaf child takes rows nextRow .. nextRow + len - 1 and nextRow += len.  Slot 0 stays
   slot 0.  So child 1's subtree is laid out before child 0's, a node's two inner children are adjacent, and a node's direct leaves
   precede everything below it.
5. Output.  Node v goes to its new slot: words 0-11, 14 and 15 unchanged (the split word and whatever the fourth link word holds);
   words 12 and 13 become 64 * newSlot(child), ~newRow(child), 0 for LINK_NONE, and the word itself for LINK_BAD.  Every leaf link
   gets its own copy of its rows and of the triIndex words beside them, bit for bit, the terminator row with all its words included;
   a leaf two links name is copied twice.  A malformed leaf is emitted as a lone terminator row: four words 0x80000000, triIndex 0.
   Unreached slots, and rows no reached leaf link names, are dropped.  The new extents are 64 * nextSlot, 16 * nextRow and
   4 * nextRow bytes; nothing beyond them is written.
6. Reported: LINK_BAD words and malformed leaves of reached slots (the device: NTR_ERR_LAYOUT after the work).  What unreached slots
   hold is never looked at.

Closed form (`closed_form`; `reorder` asserts that it equals the walk of rule 4; it is what the device computes).  Bottom-up, I(v) =
the inner nodes in v's subtree, itself included; W(v) = the rows of all leaves below v; d_k(v) = the length of v's direct leaf child
k, 0 if it is none; a(v) = the number of v's inner children; d(v) = d_0(v) + d_1(v).  Let f(v), g(v) be nextSlot, nextRow at the
moment v is popped: f(0) = 1, g(0) = 0, and
   newSlot(c0) = f(v)                        newSlot(c1) = f(v) + [c0 inner]
   newRow(c0)  = g(v)                        newRow(c1)  = g(v) + d_0(v)
   f(c1) = f(v) + a(v)                       g(c1) = g(v) + d(v)
   f(c0) = f(v) + a(v) + (c1 inner ? I(c1) - 1 : 0)          g(c0) = g(v) + d(v) + (c1 inner ? W(c1) : 0)
because everything child 1's subtree allocates below c1 itself is handed out between v's pop and c0's.  So a node's place is a sum
along its parent chain and no level loop is needed.

stats: numNodes (reached slots = nextSlot), numLeaves (leaf links of reached slots), numRows (nextRow), numDroppedSlots.
"""
import numpy as np

TERM = 0x80000000
NONE, LEAF, INNER, BAD = 0, 1, 2, 3


def kind_of(c, num_slots):
    if c == 0:
        return NONE
    if c < 0:
        return LEAF
    return INNER if (c % 64 == 0 and c // 64 < num_slots) else BAD


def _views(nodes, woop, tri_index):
    ni = np.ascontiguousarray(nodes).reshape(-1).view(np.int32).reshape(-1, 16)
    w = np.ascontiguousarray(woop).reshape(-1).view(np.uint32).reshape(-1, 4)
    ti = np.ascontiguousarray(tri_index).reshape(-1).view(np.int32)
    assert ti.size >= w.shape[0], "triIndex must cover one entry per Woop row"
    return ni, w, ti


def leaf_length(wx, link):
    """(rows, malformed) of the leaf at link < 0; wx is the x word of every row (a list or array)."""
    r, n = ~link, len(wx)
    while r < n and wx[r] != TERM:
        r += 3
    return (r - ~link + 1, False) if r < n else (1, True)


def walk(ni, wx):
    """Rule 4, literally.  Returns (src_of: old slot per new slot, new_link [numSlots, 2] (rows of unreached slots are 0),
    leaves: list of (old first row, new first row, length, malformed) in output order, bad_links)."""
    S = ni.shape[0]
    links = ni[:, 12:14].tolist()
    new_link = np.zeros((S, 2), np.int64)
    src_of, leaves, bad = [0], [], 0
    seen = np.zeros(S, bool)
    seen[0] = True
    stack, next_row = [0], 0
    while stack:
        v = stack.pop()
        for k in (0, 1):
            c = links[v][k]
            kd = kind_of(c, S)
            if kd == INNER:
                assert not seen[c // 64], "the links do not form a tree under slot 0"
                seen[c // 64] = True
                new_link[v, k] = 64 * len(src_of)
                src_of.append(c // 64)
                stack.append(c // 64)
            elif kd == LEAF:
                n, mal = leaf_length(wx, c)
                new_link[v, k] = ~next_row
                leaves.append((~c, next_row, n, mal))
                next_row += n
            else:
                new_link[v, k] = c
                bad += kd == BAD
    return np.array(src_of, np.int64), new_link, leaves, bad


def closed_form(ni, wx):
    """The closed form: the same four values as walk(), from I, W bottom-up and f, g as sums along the parent chain."""
    S = ni.shape[0]
    links = ni[:, 12:14].tolist()
    kinds = [[kind_of(c, S) for c in l] for l in links]
    # reached slots in some top-down order, and each one's parent child slot
    order, parent = [0], {0: None}
    for v in order:
        for k in (0, 1):
            if kinds[v][k] == INNER:
                c = links[v][k] // 64
                assert c not in parent, "the links do not form a tree under slot 0"
                parent[c] = (v, k)
                order.append(c)
    I, W, dk = {}, {}, {}
    for v in reversed(order):
        I[v], W[v], dk[v] = 1, 0, [0, 0]
        for k in (0, 1):
            if kinds[v][k] == INNER:
                I[v] += I[links[v][k] // 64]
                W[v] += W[links[v][k] // 64]
            elif kinds[v][k] == LEAF:
                dk[v][k] = leaf_length(wx, links[v][k])[0]
                W[v] += dk[v][k]
    # the two deltas of every child slot
    df, dg = {}, {}
    for v in order:
        a = (kinds[v][0] == INNER) + (kinds[v][1] == INNER)
        d = dk[v][0] + dk[v][1]
        c1 = links[v][1] // 64 if kinds[v][1] == INNER else None
        df[(v, 1)], dg[(v, 1)] = a, d
        df[(v, 0)], dg[(v, 0)] = a + (I[c1] - 1 if c1 is not None else 0), d + (W[c1] if c1 is not None else 0)
    new_link = np.zeros((S, 2), np.int64)
    src_of = np.full(I[0], -1, np.int64)
    src_of[0] = 0
    placed, bad = [], 0
    for v in order:
        f, g, n = 1, 0, v
        while parent[n] is not None:                       # a sum along the parent chain
            f += df[parent[n]]
            g += dg[parent[n]]
            n = parent[n][0]
        for k in (0, 1):
            c, kd = links[v][k], kinds[v][k]
            if kd == INNER:
                s = f + (k == 1 and kinds[v][0] == INNER)
                new_link[v, k] = 64 * s
                src_of[s] = c // 64
            elif kd == LEAF:
                row = g + (dk[v][0] if k == 1 else 0)
                new_link[v, k] = ~row
                placed.append((~c, row, dk[v][k], leaf_length(wx, c)[1]))
            else:
                new_link[v, k] = c
                bad += kd == BAD
    placed.sort(key=lambda t: t[1])
    assert sum(t[2] for t in placed) == W[0]
    return src_of, new_link, placed, bad


def reorder(nodes, woop, tri_index):
    """Returns dict(nodes int32[numNodes, 16], woop uint8[16 * numRows], tri_index int32[numRows], stats, bad_links, bad_leaves)."""
    ni, w, ti = _views(nodes, woop, tri_index)
    wx = w[:, 0].tolist()
    src_of, new_link, leaves, bad = walk(ni, wx)
    c_src, c_link, c_leaves, c_bad = closed_form(ni, wx)
    assert np.array_equal(src_of, c_src) and np.array_equal(new_link, c_link) and leaves == c_leaves and bad == c_bad, \
        "the closed form differs from the walk"
    out = ni[src_of].copy()
    out[:, 12:14] = new_link[src_of].astype(np.int32)
    rows = sum(t[2] for t in leaves)
    ow = np.empty((rows, 4), np.uint32)
    oi = np.empty(rows, np.int32)
    for src, dst, n, mal in leaves:
        if mal:
            ow[dst], oi[dst] = TERM, 0
        else:
            ow[dst:dst + n] = w[src:src + n]
            oi[dst:dst + n] = ti[src:src + n]
    stats = dict(numNodes=int(src_of.size), numLeaves=len(leaves), numRows=int(rows), numDroppedSlots=int(ni.shape[0] - src_of.size))
    return dict(nodes=out, woop=ow.reshape(-1).view(np.uint8).copy(), tri_index=oi, stats=stats, bad_links=int(bad),
                bad_leaves=int(sum(t[3] for t in leaves)))
