"""numpy restatement of HLBVHBuilder::buildHLBVH (src/rt/bvh/HLBVH/HLBVHBuilder.cpp:595-750) -- the spec of ntr_hlbvh_build.

The device build must equal this tree bit for bit in canonical form (oracle.bvh_canonical_hash: node numbering and leaf placement
are free, as for the LBVH).  The per-triangle terms are the LBVH's: Morton codes and Woop rows come from the C oracle
(orc_lbvh_morton, orc_lbvh_woop) and the sort is the same stable sort by code.

  clusters     radixSort.cu:48-58, 74-115: with d = 3 * hlbvhBits, consecutive sorted triangles with equal code >> d form one cluster;
               hlbvhBits = 0 uses predFalse (every triangle is a cluster, no bottom level).  Cluster box = min / max over the raw
               vertices (no epsilon, emitTreeKernel.cu:1090-).
  top level    HLBVHBuilder.cpp:156-317, breadth first over tasks; the root task holds every cluster and its box is sceneMin/Max.
               fillBins (emitTreeKernel.cu:713-777): mid = lo + (hi - lo) / 2, step = (taskHi - taskLo) / 8,
               bin = clamp(int(floorf((mid - taskLo) / step)), 0, 7) per axis in binary32; bin boxes reduced in the f2i order (:78-95).
               findSplit (:779-938): per axis 0..2 a sweep from the right, then from the left over planes 0..6; cost
               cntL * area(boxL) + cntR * area(boxR), area(v) = (x*y + y*z + z*x) * 2 (:119-121); a plane wins only with s < best
               (best starts at FLT_MAX), so the first (axis, plane) wins ties and an empty side (0 * inf = NaN) never wins.  Children
               get the union boxes of their bins.  A child of more than one cluster is a new top node; a child of one cluster is a leaf
               over its triangles (<= leafSize of them) or the root of a bottom-level tree.  Axis word = SAH axis, 0 for an object split.
  bottom level HLBVHBuilder.cpp:319-406 with bOfs = 3 * (10 - hlbvhBits): the LBVH emit (emitTreeKernel.cu:233-381) with the starting
               level 3 * hlbvhBits - 1 at each bottom-level root, so the depth rule (level 0 forces leaves) fires 3 * hlbvhBits levels
               below the cluster root.
  refit        calcAABB (emitTreeKernel.cu:383-562): leaf box = fold of min(a, b, c) - epsilon / max(a, b, c) + epsilon, inner child
               box = union of its two child boxes -- exactly the LBVH's.

CANONICAL choices (where the reference is nondeterministic or broken):
  1. float -> int of the bin index follows CUDA's cvt.rzi.s32.f32 (emitTreeKernel.cu:742, ifloorf): NaN -> 0, +inf -> 7, -inf -> 0.
     A flat task (a floor) gives 0 / 0 = NaN, so its clusters all fall into bin 0 on the flat axis.
  2. Split missed (no cost below FLT_MAX, :852-866): cntR = n // 2, cntL = n - cntR, axis 0; the reference picks the clusters that go
     left by atomic order (distribute, :940-1027, `atomicAdd(g_qsiCnt + old_id, 1<<4)`); here the cntL clusters of lowest index
     (Morton order) go left.
  3. Split missed: the reference leaves the right child's task box unset (`mx_left = mn_right`, :859); here both children get the box
     of the first occupied bin on axis 0.
  4. Fewer than two clusters: the reference writes a self-referencing root (:911-922, r = 0); here the tree is the bottom-level tree of
     the whole range.
  5. numTris <= leafSize, and hlbvhBits == 10 (HLBVHBuilder.cpp:44-47): the tree is ntr_lbvh_build's.
  6. Arithmetic is strict IEEE binary32 in source order (the reference builds with -use_fast_math).  area()'s `* 2.0` is a binary64
     multiply of a binary32 sum narrowed back to binary32, which equals the binary32 product.

The sign of a zero never reaches a decision: a task box has lo == hi on an axis exactly when every mid on it equals lo, and then
(mid - lo) / step is +-0 / +-0 = NaN -> bin 0 whatever the signs; costs compare equal for +0 and -0."""
import ctypes as C

import numpy as np

from oracle import oracle

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
BINS = 8
NAN_BIN = 0            # canonical choice 1; a name of its own so that a test can show which scenes tell it from 7


def missed_cnt_right(m):
    """Canonical choice 2: clusters that go right when a task of m clusters misses its split."""
    return m // 2


def left_of_plane(bins_a, b):
    """Plane b of an axis has bins 0..b on its left (emitTreeKernel.cu:940-1027, `bin <= split`)."""
    return bins_a <= b


def f2i(a):
    """emitTreeKernel.cu:78-81: an int whose signed order is the float order (-0 < +0)."""
    i = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF).astype(np.int32)


def i2f(a):
    i = np.asarray(a, dtype=np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF).astype(np.int32).view(np.float32)


def cu_fminf(a, b):
    a, b = F32(a), F32(b)
    if a != a:
        return b
    if b != b:
        return a
    return a if f2i(a) <= f2i(b) else b


def cu_fmaxf(a, b):
    a, b = F32(a), F32(b)
    if a != a:
        return b
    if b != b:
        return a
    return a if f2i(a) >= f2i(b) else b


def bin_index(q):
    """clamp((int)floorf(q), 0, 7) with cvt.rzi.s32.f32 saturation (canonical choice 1)."""
    q = F32(q)
    if q != q:
        return 0
    f = np.floor(q)
    if f >= 7:
        return 7
    if f <= 0:
        return 0
    return int(f)


def area(v):
    x, y, z = F32(v[0]), F32(v[1]), F32(v[2])
    with np.errstate(over="ignore", invalid="ignore"):
        return F32((x * y + y * z + z * x) * F32(2))


def morton_sorted(tri, pos, mn, mx):
    n = tri.shape[0]
    keys = np.zeros(n, np.uint32)
    idx = np.zeros(n, np.int32)
    oracle.lib().orc_lbvh_morton(n, oracle._ptr(tri), oracle._ptr(pos), oracle._ptr(mn), oracle._ptr(mx), oracle._ptr(keys),
                                 oracle._ptr(idx))
    order = np.argsort(keys, kind="stable")
    return keys[order], idx[order]


def woop_rows(tri, pos):
    out = np.zeros((tri.shape[0], 12), np.float32)
    oracle.lib().orc_lbvh_woop(tri.shape[0], oracle._ptr(tri), oracle._ptr(pos), oracle._ptr(out))
    return out


def clusters(keys, bits):
    """Cluster starts (plus n at the end) over the sorted codes."""
    n = keys.shape[0]
    if bits == 0:
        return np.arange(n + 1, dtype=np.int64)
    k = keys >> np.uint32(3 * bits)
    heads = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    return np.concatenate([heads, [n]]).astype(np.int64)


def cluster_boxes(tri, pos, tri_sorted, starts):
    """Raw vertex box per cluster (no epsilon), min / max in the f2i order: (C, 3) lo and hi."""
    v = pos[tri[tri_sorted]]                       # (n, 3 verts, 3)
    lo_i = f2i(v).min(axis=1)
    hi_i = f2i(v).max(axis=1)
    lo = np.minimum.reduceat(lo_i, starts[:-1], axis=0)
    hi = np.maximum.reduceat(hi_i, starts[:-1], axis=0)
    return i2f(lo), i2f(hi)


def find_split(cl_lo, cl_hi, t_lo, t_hi):
    """fillBins + findSplit for one task.  Returns (axis, left_mask, box_left, box_right, bins) with box = (lo[3], hi[3]);
    axis is 0 and the mask None for an object split."""
    m = cl_lo.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mid = (cl_lo + (cl_hi - cl_lo) / F32(2)).astype(np.float32)
        step = ((t_hi - t_lo) / F32(BINS)).astype(np.float32)
        q = ((mid - t_lo) / step).astype(np.float32)
    f = np.floor(q)
    bins = np.where(q != q, NAN_BIN, np.where(f >= 7, 7, np.where(f <= 0, 0, np.nan_to_num(f)))).astype(np.int64).reshape(m, 3)
    lo_i, hi_i = f2i(cl_lo), f2i(cl_hi)
    # bin boxes in the f2i order, empty bins +-FLT_MAX (initBins, :695-711)
    b_lo = np.full((3, BINS, 3), FLT_MAX, np.float32)
    b_hi = np.full((3, BINS, 3), -FLT_MAX, np.float32)
    b_cnt = np.zeros((3, BINS), np.int64)
    for a in range(3):
        for b in range(BINS):
            sel = bins[:, a] == b
            b_cnt[a, b] = int(sel.sum())
            if b_cnt[a, b]:
                b_lo[a, b] = i2f(np.minimum(lo_i[sel].min(axis=0), f2i(FLT_MAX)))
                b_hi[a, b] = i2f(np.maximum(hi_i[sel].max(axis=0), f2i(-FLT_MAX)))
    # sweeps in the f2i domain (min / max there is fminf / fmaxf for the NaN-free bin boxes); plane b of axis a has bins 0..b on
    # the left and b+1..7 on the right.  The sequential `s < best` keeps the FIRST minimum in (axis, plane) order.
    blo, bhi = f2i(b_lo).astype(np.int64), f2i(b_hi).astype(np.int64)
    l_lo = np.minimum.accumulate(blo, axis=1)[:, :BINS - 1]
    l_hi = np.maximum.accumulate(bhi, axis=1)[:, :BINS - 1]
    r_lo = np.minimum.accumulate(blo[:, ::-1], axis=1)[:, ::-1][:, 1:]
    r_hi = np.maximum.accumulate(bhi[:, ::-1], axis=1)[:, ::-1][:, 1:]
    c_l = np.cumsum(b_cnt, axis=1)[:, :BINS - 1]
    c_r = np.cumsum(b_cnt[:, ::-1], axis=1)[:, ::-1][:, 1:]

    def area_v(d):
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        return ((x * y + y * z + z * x) * F32(2)).astype(np.float32)

    with np.errstate(over="ignore", invalid="ignore"):
        dl = (i2f(l_hi.astype(np.int32)) - i2f(l_lo.astype(np.int32))).astype(np.float32)
        dr = (i2f(r_hi.astype(np.int32)) - i2f(r_lo.astype(np.int32))).astype(np.float32)
        s = (c_l.astype(np.float32) * area_v(dl) + c_r.astype(np.float32) * area_v(dr)).astype(np.float32)
    flat = s.reshape(-1)
    ok = flat < FLT_MAX
    win = None
    if ok.any():
        j = int(np.argmin(np.where(ok, flat, np.inf)))
        a, b = divmod(j, BINS - 1)
        win = (a, b, (i2f(l_lo[a, b].astype(np.int32)), i2f(l_hi[a, b].astype(np.int32))),
               (i2f(r_lo[a, b].astype(np.int32)), i2f(r_hi[a, b].astype(np.int32))))
    if win is None:
        # split missed: object split, both children get the box of the first occupied bin on axis 0 (canonical 2, 3)
        b0 = int(np.flatnonzero(b_cnt[0])[0])
        box = (b_lo[0, b0].copy(), b_hi[0, b0].copy())
        return 0, None, box, box, bins
    a, b, bl, br = win
    return a, left_of_plane(bins[:, a], b), bl, br, bins


def hlbvh_build(tri, pos, bits, leaf_size=8, epsilon=0.001, bbox=None):
    """Returns dict(nodes (uint8), woop (uint8), tri_index (int32), num_inner, num_leaves, num_clusters, top_nodes, top_levels,
    lbvh_path, structure, decisions) -- Compact buffers like oracle.lbvh_build; `structure` is the decision record used by the tests,
    `decisions` says per top-level task its level, its range of cluster positions and whether its split was missed."""
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    n = tri.shape[0]
    if not 0 <= bits <= 10:
        raise ValueError("hlbvhBits must be in 0..10")
    mn, mx = bbox if bbox is not None else oracle.scene_bbox(pos)
    mn = np.ascontiguousarray(mn, dtype=np.float32)
    mx = np.ascontiguousarray(mx, dtype=np.float32)
    if bits == 10 or n <= leaf_size:                  # canonical 5
        r = oracle.lbvh_build(tri, pos, leaf_size, epsilon, bbox=(mn, mx))
        r.update(num_clusters=0, top_nodes=0, top_levels=0, lbvh_path=True, structure=None, decisions=None)
        return r
    keys, ts = morton_sorted(tri, pos, mn, mx)
    woop12 = woop_rows(tri, pos)
    starts = clusters(keys, bits)
    C_ = starts.shape[0] - 1
    cl_lo, cl_hi = cluster_boxes(tri, pos, ts, starts)

    # nodes: dict index -> [child0, child1, axis]; a child is ("node", idx) or ("leaf", start, end)
    nodes = {}
    bottom_roots = []                                 # (node index, start, end)
    next_node = [1]

    def new_node():
        i = next_node[0]
        next_node[0] += 1
        return i

    top_levels = 0
    top_nodes = 0
    structure = []
    decisions = []                                    # per top-level task: level, node, cluster positions [beg, end), missed, axis
    if C_ < 2:                                        # canonical 4
        bottom_roots.append((0, 0, n))
    else:
        # (node, clusters in order, task box, first position): a stable partition keeps a task's clusters in one range of positions
        tasks = [(0, list(range(C_)), (mn.copy(), mx.copy()), 0)]
        while tasks:
            top_levels += 1
            nxt = []
            for node, cls, (tlo, thi), beg in tasks:
                top_nodes += 1
                cls = np.array(cls)
                axis, left, bl, br, _ = find_split(cl_lo[cls], cl_hi[cls], tlo, thi)
                missed = left is None
                if missed:
                    cnt_r = missed_cnt_right(len(cls))
                    left = np.arange(len(cls)) < len(cls) - cnt_r
                parts = (cls[left], cls[~left])
                structure.append((node, axis, [list(map(int, p)) for p in parts]))
                decisions.append(dict(level=top_levels - 1, node=node, beg=beg, end=beg + len(cls), missed=missed, axis=axis,
                                      cnt_l=len(parts[0])))
                ch = []
                for part, box, pbeg in zip(parts, (bl, br), (beg, beg + len(parts[0]))):
                    if len(part) > 1:
                        k = new_node()
                        nxt.append((k, list(part), box, pbeg))
                        ch.append(("node", k))
                    else:
                        c = int(part[0])
                        s, e = int(starts[c]), int(starts[c + 1])
                        if e - s <= leaf_size:
                            ch.append(("leaf", s, e))
                        else:
                            k = new_node()
                            bottom_roots.append((k, s, e))
                            ch.append(("node", k))
                nodes[node] = [ch[0], ch[1], axis]
            tasks = nxt

    # bottom level: the LBVH emit, starting level 3 * bits - 1 at every bottom root (HLBVHBuilder.cpp:337-361)
    q = list(bottom_roots)
    level = 0
    while level < 3 * bits and q:
        lv0 = 3 * bits - 1 - level
        nq = []
        for nIdx, s, e in q:
            lv = lv0
            while lv >= 0 and ((int(keys[s]) >> lv) & 1) == ((int(keys[e - 1]) >> lv) & 1):
                lv -= 1
            if lv >= 0:
                start_bit = (int(keys[s]) >> lv) & 1
                a, b = s, e
                while True:
                    split = (a + b) >> 1
                    sb = (int(keys[split]) >> lv) & 1
                    if ((int(keys[split - 1]) >> lv) & 1) != sb:
                        break
                    if sb == start_bit:
                        a = split
                    else:
                        b = split
            else:
                split = (s + e) >> 1
            ch = []
            for cs, ce in ((s, split), (split, e)):
                if ce - cs <= leaf_size or lv0 == 0:
                    ch.append(("leaf", cs, ce))
                else:
                    k = new_node()
                    nq.append((k, cs, ce))
                    ch.append(("node", k))
            nodes[nIdx] = [ch[0], ch[1], int(np.fmod(lv, 3))]
        q = nq
        level += 1
    if q:
        raise AssertionError("bottom level did not terminate")  # level 0 forces leaves

    # Compact buffers: leaves in node order, child 0 before child 1
    num = next_node[0]
    out_nodes = np.zeros((num, 16), np.int32)
    woop = np.zeros(((n * 4 + 4), 4), np.float32)
    tidx = np.zeros(n * 4 + 4, np.int32)
    tri_box_lo = i2f(f2i(pos[tri[ts]]).min(axis=1))   # per sorted triangle
    tri_box_hi = i2f(f2i(pos[tri[ts]]).max(axis=1))
    with np.errstate(over="ignore", invalid="ignore"):
        term_lo = (tri_box_lo - F32(epsilon)).astype(np.float32)
        term_hi = (tri_box_hi + F32(epsilon)).astype(np.float32)
    all_tris = 0
    num_leaves = 0
    boxes = {}

    def leaf_box(s, e):
        lo = np.full(3, FLT_MAX, np.float32)
        hi = np.full(3, -FLT_MAX, np.float32)
        if e > s:
            lo = i2f(np.minimum(f2i(term_lo[s:e]).min(axis=0), f2i(lo)))
            hi = i2f(np.maximum(f2i(term_hi[s:e]).max(axis=0), f2i(hi)))
        return lo, hi

    order = sorted(nodes)
    for i in order:
        ch = nodes[i]
        for k in range(2):
            c = ch[k]
            if c[0] == "leaf":
                s, e = c[1], c[2]
                out = all_tris * 3 + num_leaves
                for j in range(e - s):
                    t = int(ts[s + j])
                    woop[out + 3 * j:out + 3 * j + 3] = woop12[t].reshape(3, 4)
                    tidx[out + 3 * j] = t
                woop[out + 3 * (e - s)].view(np.uint32)[:] = 0x80000000
                all_tris += e - s
                num_leaves += 1
                out_nodes[i, 12 + k] = ~out
            else:
                out_nodes[i, 12 + k] = c[1] * 64
        out_nodes[i, 14] = ch[2]

    def node_box(i):
        """(lo, hi) of node i = union of its child boxes; fills words 0..11 (post order)."""
        stack = [(i, 0)]
        while stack:
            j, st = stack.pop()
            ch = nodes[j]
            if st == 0:
                stack.append((j, 1))
                for c in ch[:2]:
                    if c[0] == "node" and c[1] not in boxes:
                        stack.append((c[1], 0))
                continue
            cb = []
            for c in ch[:2]:
                cb.append(leaf_box(c[1], c[2]) if c[0] == "leaf" else boxes[c[1]])
            (l0, h0), (l1, h1) = cb
            f = out_nodes[j].view(np.float32)
            f[0], f[1], f[2], f[3] = l0[0], h0[0], l0[1], h0[1]
            f[4], f[5], f[6], f[7] = l1[0], h1[0], l1[1], h1[1]
            f[8], f[9], f[10], f[11] = l0[2], h0[2], l1[2], h1[2]
            boxes[j] = (i2f(np.minimum(f2i(l0), f2i(l1))), i2f(np.maximum(f2i(h0), f2i(h1))))
        return boxes[i]

    node_box(0)
    wb = (n * 3 + num_leaves) * 16
    return dict(nodes=out_nodes.reshape(-1).view(np.uint8).copy(), woop=woop.reshape(-1).view(np.uint8)[:wb].copy(),
                tri_index=tidx[:n * 3 + num_leaves].copy(), num_inner=num, num_leaves=num_leaves, num_clusters=C_,
                top_nodes=top_nodes, top_levels=top_levels, lbvh_path=False, structure=structure, decisions=decisions,
                tri_sorted=ts, morton_sorted=keys, cluster_starts=starts, bottom_roots=bottom_roots, tree=nodes)


def canonical_hash(r):
    return oracle.bvh_canonical_hash(r["nodes"], r["woop"], r["tri_index"])
