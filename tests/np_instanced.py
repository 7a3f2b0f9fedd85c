"""numpy spec of instanced scenes: ntr_instance_invert, ntr_tlas_build and ntr_trace_instanced.

EXTENSION: the reference has no instancing.  This docstring is the normative text; the device (csrc/tlas_build_kernels.hip,
csrc/trace_instanced_kernels.hip) equals tlas_build() and trace() bit for bit, the host's ntr_instance_invert equals invert().
All arithmetic is binary32 without contraction unless said otherwise; min and max are taken in the floats' total order
(np_hlbvh.f2i: -0 < +0, NaNs beyond the infinities), as PLOC takes them.

Data.
  pool        three buffers: nodes, triWoop, triIndex.  BLAS k occupies [nodesOffset, +nodesBytes) of the pool's nodes (both multiples
              of 64, nodesBytes >= 64) and [triWoopOffset, +triWoopBytes) of its triWoop (triWoopOffset a multiple of 16); its triIndex
              entries start at entry triWoopOffset / 16 (byte triWoopOffset / 4).  A BLAS is byte for byte what any builder of the
              library wrote when it was handed pool + offset: its links stay relative to its own start, its root is its node 0.  Each
              pool buffer is at most 0xFFFFFF00 bytes.
  instance    (objectToWorld 3x4 row-major, worldToObject 3x4 row-major, blas index)
  xform(m, p, w)   component r is dot4(row r of m, p.x, p.y, p.z, w) in np_tracer._dot4's order:
              r = 0; r += a0 * x; r += a1 * y; r += a2 * z; r += a3 * w

invert(objectToWorld).  In binary64, with m[r][c] the entries and t = column 3:
    c00 = m11 * m22 - m12 * m21      c01 = m12 * m20 - m10 * m22      c02 = m10 * m21 - m11 * m20
    det = (m00 * c00 + m01 * c01) + m02 * c02
    i00 = c00 / det                  i01 = (m02 * m21 - m01 * m22) / det    i02 = (m01 * m12 - m02 * m11) / det
    i10 = c01 / det                  i11 = (m00 * m22 - m02 * m20) / det    i12 = (m02 * m10 - m00 * m12) / det
    i20 = c02 / det                  i21 = (m01 * m20 - m00 * m21) / det    i22 = (m00 * m11 - m01 * m10) / det
    ir3 = -((ir0 * t0 + ir1 * t1) + ir2 * t2)          (the unrounded binary64 ir0, ir1, ir2)
  every product is rounded before the sum or difference that uses it (no contraction); each of the 12 results is rounded once to
  binary32.  A zero or non-finite determinant is an error.

instance_box(pool_nodes, blas, objectToWorld).  The object box is the union of the two child boxes of the BLAS's node 0 (the
  one-triangle tree's empty child, (FLT_MAX, -FLT_MAX), drops out of the union by itself).  Its eight corners in the order c = 0..7 --
  bit 0 of c takes hi.x, bit 1 hi.y, bit 2 hi.z, a clear bit lo -- go through xform(objectToWorld, corner, 1); the world box is the
  min / max of the eight results.  No padding.

tlas_build(pool_nodes, blas_ranges, instances, radius) -> nodes, root_link, records, scene box, stats.
  scene box   the union of all instance boxes
  order       the LBVH's Morton code of the instance box over the scene box: step = (max - min) / 1024, mid = lo + (hi - lo) / 2,
              q = (mid - min) / step; the cell is 0 if !(q >= 0), 1023 if q >= 1024, floor(q) otherwise; cells interleaved
              x | y << 1 | z << 2 (ten bits each); a stable sort by code
  clusters    one per instance in sorted order: its world box, link ~i with i the instance's index in the caller's array, height 0
  rounds      exactly np_bvh_ploc's: same key (d, k, b), same slots from the top, same node words (np_bvh_ploc.neighbours is imported)
  N == 1      no node, root_link = ~0, height 0, no round.  N >= 2: N - 1 nodes, root_link = 0
  record i    16 words in the caller's order: 0..11 worldToObject, 12 nodesOffset (bytes), 13 triWoopOffset / 16 (rows),
              14 nodesBytes, 15 zero

trace(tlas_nodes, root_link, records, pool, rays, any_hit) -> (id, t, u, v, instance).
  A ray has its world form W and a current form R (R starts as W), one tmax that shrinks and one stack of at most 104 entries (the
  device's 16 + 88; the spec raises beyond).  It starts at root_link; a degenerate ray (!(tmin < tmax)) is a miss without traversal.
  top level, inner node    np_tracer's inner step on tlas_nodes with W: same accept test, nearer child first (ties to child 0), the
                           far child pushed, a pop when no child is accepted
  top level, link ~i       the ray enters instance i: push the exit marker; R.o = xform(worldToObject_i, W.o, 1), R.d =
                           xform(worldToObject_i, W.d, 0); tmin and the current tmax stay (the direction is not normalised, so t
                           means the same on both levels); on at node 0 of BLAS i
  bottom level             np_tracer's inner and triangle steps with R; node offsets are relative to nodesOffset, rows to the row
                           offset; an accepted hit sets tmax = t, id = triIndex[rowOffset + row], instance = i and u, v; for any-hit
                           the ray ends there
  popping the exit marker  R = W, the ray is back on the top level, and it pops again
  popping the sentinel     (an empty stack) the ray is done
  miss                     id -1, instance -1, t = ray.tmax, u = v = 0
"""
import numpy as np

import np_hlbvh
from np_bvh_ploc import neighbours

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
TERM = 0x80000000
SENTINEL = 0x76543210
EXIT_MARKER = SENTINEL + 1
MAX_STACK = 104
MAX_HEIGHT = 100
TAIL = 1024
POOL_MAX_BYTES = 0xFFFFFF00

INSTANCE_DTYPE = np.dtype([("objectToWorld", "<f4", (12,)), ("worldToObject", "<f4", (12,)), ("blas", "<i4"), ("reserved", "<i4", (3,))])


# ---- transforms ---------------------------------------------------------------------------------------------------------------------
def invert(object_to_world):
    m = np.asarray(object_to_world, F).reshape(3, 4).astype(np.float64)
    (m00, m01, m02, t0), (m10, m11, m12, t1), (m20, m21, m22, t2) = m
    with np.errstate(all="ignore"):
        c00 = m11 * m22 - m12 * m21
        c01 = m12 * m20 - m10 * m22
        c02 = m10 * m21 - m11 * m20
        det = (m00 * c00 + m01 * c01) + m02 * c02
        if not np.isfinite(det) or det == 0.0:
            raise ValueError("np_instanced.invert: singular or non-finite transform")
        inv = np.array([[c00 / det, (m02 * m21 - m01 * m22) / det, (m01 * m12 - m02 * m11) / det, 0.0],
                        [c01 / det, (m00 * m22 - m02 * m20) / det, (m02 * m10 - m00 * m12) / det, 0.0],
                        [c02 / det, (m01 * m20 - m00 * m21) / det, (m00 * m11 - m01 * m10) / det, 0.0]], np.float64)
        for r in range(3):
            inv[r, 3] = -((inv[r, 0] * t0 + inv[r, 1] * t1) + inv[r, 2] * t2)
        return inv.astype(F).reshape(12)


def xform(m, x, y, z, w):
    """m: (..., 12) float32; x, y, z: arrays; w: 0 or 1 -> three arrays."""
    m = np.asarray(m, F)
    w = F(w)
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            a = m[..., 4 * r:4 * r + 4]
            v = np.zeros_like(x, dtype=F)
            v = (v + (a[..., 0] * x).astype(F)).astype(F)
            v = (v + (a[..., 1] * y).astype(F)).astype(F)
            v = (v + (a[..., 2] * z).astype(F)).astype(F)
            v = (v + (a[..., 3] * w).astype(F)).astype(F)
            out.append(v)
    return out


def instances(transforms, blas):
    """An INSTANCE_DTYPE array from objectToWorld matrices (n, 12) and BLAS indices; worldToObject by invert()."""
    transforms = np.asarray(transforms, F).reshape(-1, 12)
    inst = np.zeros(transforms.shape[0], INSTANCE_DTYPE)
    inst["objectToWorld"] = transforms
    inst["worldToObject"] = np.stack([invert(t) for t in transforms]) if transforms.shape[0] else np.zeros((0, 12), F)
    inst["blas"] = np.asarray(blas, np.int32)
    return inst


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


# ---- the pool -------------------------------------------------------------------------------------------------------------------------
def make_pool(blases, gap_nodes=0, gap_rows=0):
    """blases: a list of (nodes, woop, tri_index) arrays as a builder returns them.  -> dict(nodes uint8, woop uint8, tri_index int32,
    ranges: a list of (nodesOffset, nodesBytes, triWoopOffset, triWoopBytes)).  gap_*: unused slots between two BLASes."""
    nodes, woop, idx, ranges = [], [], [], []
    n_off = w_off = 0
    for nd, wp, ti in blases:
        nd = np.ascontiguousarray(nd).view(np.uint8).reshape(-1)
        wp = np.ascontiguousarray(wp).view(np.uint8).reshape(-1)
        ti = np.ascontiguousarray(ti, np.int32).reshape(-1)
        assert nd.size % 64 == 0 and nd.size >= 64 and wp.size % 16 == 0 and ti.size * 4 == wp.size // 4
        ranges.append((n_off, nd.size, w_off, wp.size))
        nodes += [nd, np.zeros(64 * gap_nodes, np.uint8)]
        woop += [wp, np.zeros(16 * gap_rows, np.uint8)]
        idx += [ti, np.zeros(gap_rows, np.int32)]
        n_off += nd.size + 64 * gap_nodes
        w_off += wp.size + 16 * gap_rows
    return dict(nodes=np.concatenate(nodes), woop=np.concatenate(woop), tri_index=np.concatenate(idx), ranges=ranges)


# ---- the top-level build ------------------------------------------------------------------------------------------------------------
def instance_box(pool_nodes, blas_range, object_to_world):
    """-> (lo, hi), each three float32."""
    w = np.ascontiguousarray(pool_nodes).view(np.uint8).reshape(-1)[blas_range[0]:blas_range[0] + 48].view(F)
    lo0, hi0 = np.array([w[0], w[2], w[8]], F), np.array([w[1], w[3], w[9]], F)
    lo1, hi1 = np.array([w[4], w[6], w[10]], F), np.array([w[5], w[7], w[11]], F)
    lo = np_hlbvh.i2f(np.minimum(np_hlbvh.f2i(lo0), np_hlbvh.f2i(lo1)))
    hi = np_hlbvh.i2f(np.maximum(np_hlbvh.f2i(hi0), np_hlbvh.f2i(hi1)))
    c = np.arange(8)
    x = np.where(c & 1, hi[0], lo[0]).astype(F)
    y = np.where(c & 2, hi[1], lo[1]).astype(F)
    z = np.where(c & 4, hi[2], lo[2]).astype(F)
    p = np.stack(xform(np.asarray(object_to_world, F).reshape(12), x, y, z, 1), axis=1)   # (8, 3)
    pi = np_hlbvh.f2i(p)
    return np_hlbvh.i2f(pi.min(axis=0)), np_hlbvh.i2f(pi.max(axis=0))


def _spread(n):
    n = n.astype(np.uint32) & np.uint32(0x3ff)
    n = (n ^ (n << np.uint32(16))) & np.uint32(0xff0000ff)
    n = (n ^ (n << np.uint32(8))) & np.uint32(0x0300f00f)
    n = (n ^ (n << np.uint32(4))) & np.uint32(0x030c30c3)
    return (n ^ (n << np.uint32(2))) & np.uint32(0x09249249)


def morton_codes(lo, hi, mn, mx):
    """lo, hi: (n, 3) boxes; mn, mx: the scene box -> uint32 codes."""
    with np.errstate(all="ignore"):
        step = ((mx - mn).astype(F) / F(1024)).astype(F)
        mid = (lo + ((hi - lo).astype(F) / F(2)).astype(F)).astype(F)
        q = ((mid - mn).astype(F) / step).astype(F)
        cell = np.where(~(q >= 0), 0, np.where(q >= 1024, 1023, np.floor(np.where(np.isfinite(q), q, 0)))).astype(np.int64)
    return _spread(cell[:, 0]) | (_spread(cell[:, 1]) << np.uint32(1)) | (_spread(cell[:, 2]) << np.uint32(2))


def tlas_build(pool_nodes, blas_ranges, inst, radius=8):
    """-> dict(nodes (N - 1, 16) int32, root_link, records (N, 16) uint32, scene_min, scene_max, codes, order,
    stats dict(numNodes, numRounds, height, tailClusters), sizes)."""
    n = inst.shape[0]
    assert n >= 1 and 1 <= radius <= 64
    boxes = [instance_box(pool_nodes, blas_ranges[int(b)], m) for m, b in zip(inst["objectToWorld"], inst["blas"])]
    lo = np.stack([b[0] for b in boxes]).astype(F)
    hi = np.stack([b[1] for b in boxes]).astype(F)
    lo_i, hi_i = np_hlbvh.f2i(lo), np_hlbvh.f2i(hi)
    mn, mx = np_hlbvh.i2f(lo_i.min(axis=0)), np_hlbvh.i2f(hi_i.max(axis=0))
    records = np.zeros((n, 16), np.uint32)
    records[:, :12] = inst["worldToObject"].view(np.uint32)
    for i, b in enumerate(inst["blas"]):
        r = blas_ranges[int(b)]
        records[i, 12], records[i, 13], records[i, 14] = r[0], r[2] // 16, r[1]
    out = dict(records=records, scene_min=mn, scene_max=mx)
    if n == 1:
        out.update(nodes=np.zeros((0, 16), np.int32), root_link=~0, codes=np.zeros(1, np.uint32), order=np.zeros(1, np.int64),
                   stats=dict(numNodes=0, numRounds=0, height=0, tailClusters=0), sizes=[])
        return out
    codes = morton_codes(lo, hi, mn, mx)
    order = np.argsort(codes, kind="stable")
    lo_i, hi_i = lo_i[order], hi_i[order]
    link = ~order.astype(np.int64)
    height = np.zeros(n, np.int64)
    nodes = np.zeros((n - 1, 16), np.int32)
    written = np.zeros(n - 1, bool)
    sizes = []
    while lo_i.shape[0] > 1:
        c = lo_i.shape[0]
        sizes.append(c)
        nn = neighbours(lo_i, hi_i, radius)
        idx = np.arange(c, dtype=np.int64)
        low = np.flatnonzero((nn[nn] == idx) & (idx < nn))
        up = nn[low]
        m = low.shape[0]
        assert m >= 1
        slot = (c - 1 - m) + np.arange(m, dtype=np.int64)
        assert not written[slot].any()
        written[slot] = True
        lo_f, hi_f = np_hlbvh.i2f(lo_i), np_hlbvh.i2f(hi_i)
        nf = nodes.view(F)
        for k, who in enumerate((low, up)):
            nf[slot, 4 * k + 0], nf[slot, 4 * k + 1] = lo_f[who, 0], hi_f[who, 0]
            nf[slot, 4 * k + 2], nf[slot, 4 * k + 3] = lo_f[who, 1], hi_f[who, 1]
            nf[slot, 8 + 2 * k], nf[slot, 9 + 2 * k] = lo_f[who, 2], hi_f[who, 2]
            nodes[slot, 12 + k] = link[who].astype(np.int32)
        lo_i, hi_i = lo_i.copy(), hi_i.copy()
        lo_i[low] = np.minimum(lo_i[low], lo_i[up])
        hi_i[low] = np.maximum(hi_i[low], hi_i[up])
        link[low] = 64 * slot
        height[low] = 1 + np.maximum(height[low], height[up])
        keep = np.ones(c, bool)
        keep[up] = False
        lo_i, hi_i, link, height = lo_i[keep], hi_i[keep], link[keep], height[keep]
    assert written.all() and link[0] == 0
    out.update(nodes=nodes, root_link=0, codes=codes, order=order,
               stats=dict(numNodes=n - 1, numRounds=len(sizes), height=int(height[0]), tailClusters=next(s for s in sizes if s <= TAIL)),
               sizes=sizes)
    return out


# ---- the two-level trace ------------------------------------------------------------------------------------------------------------
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


def trace(tlas_nodes, root_link, records, pool, rays, any_hit=False):
    """-> (id int32, t float32, u float32, v float32, instance int32)"""
    tl = np.ascontiguousarray(tlas_nodes).view(np.uint8).reshape(-1)
    tl = np.concatenate([tl, np.zeros(64, np.uint8)]).view(F)        # (an empty buffer when N == 1)
    pn = np.ascontiguousarray(pool["nodes"]).view(np.uint8).reshape(-1).view(F)
    pw = np.ascontiguousarray(pool["woop"]).view(np.uint8).reshape(-1).view(F).reshape(-1, 4)
    pw_u = pw.view(np.uint32)
    tri_index = np.asarray(pool["tri_index"], np.int32)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 16)
    rec_f = rec.view(F)
    n = rays.shape[0]
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
    n_off = np.zeros(n, np.int64)
    r_off = np.zeros(n, np.int64)
    stack = np.zeros((n, MAX_STACK), np.int64)
    sp = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        node[~(tmin < tmax)] = SENTINEL

    def push(idx, v):
        if (sp[idx] >= MAX_STACK).any():
            raise RuntimeError("np_instanced: stack overflow")
        stack[idx, sp[idx]] = v
        sp[idx] += 1

    def pop(idx):
        empty = sp[idx] == 0
        e, f = idx[empty], idx[~empty]
        node[e] = SENTINEL
        sp[f] -= 1
        node[f] = stack[f, sp[f]]

    def inner(idx, buf, base):
        b = (base + node[idx]) // 4
        g = lambda k: buf[b + k]
        rx, ry, rz, ex, ey, ez = (a[idx] for a in R)

        def box(lox, hix, loy, hiy, loz, hiz):
            t0x, t0y, t0z = (lox - rx) / ex, (loy - ry) / ey, (loz - rz) / ez
            t1x, t1y, t1z = (hix - rx) / ex, (hiy - ry) / ey, (hiz - rz) / ez
            mn = _smax(_smax(_smin(t0x, t1x), _smin(t0y, t1y)), _smin(t0z, t1z))
            mx = _smin(_smin(_smax(t0x, t1x), _smax(t0y, t1y)), _smax(t0z, t1z))
            return mn, mx
        mn0, mx0 = box(g(0), g(1), g(2), g(3), g(8), g(9))
        mn1, mx1 = box(g(4), g(5), g(6), g(7), g(10), g(11))
        c0 = buf.view(np.int32)[b + 12].astype(np.int64)
        c1 = buf.view(np.int32)[b + 13].astype(np.int64)
        i0 = (mn0 <= mx0) & (mx0 >= tmin[idx]) & (mn0 <= tmax[idx])
        i1 = (mn1 <= mx1) & (mx1 >= tmin[idx]) & (mn1 <= tmax[idx])
        swp = i1 & (~i0 | (mn0 > mn1))
        near, far = np.where(swp, c1, c0), np.where(swp, c0, c1)
        both = i0 & i1
        push(idx[both], far[both])
        some = i0 | i1
        node[idx[some]] = near[some]
        pop(idx[~some])

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
            assert k_top_inner.size + k_enter.size + k_bot_inner.size + k_tri.size + k_exit.size == int(act.sum())
            if k_top_inner.size:
                inner(k_top_inner, tl, 0)
            if k_bot_inner.size:
                inner(k_bot_inner, pn, n_off[k_bot_inner])
            if k_enter.size:
                i = ~node[k_enter]
                push(k_enter, EXIT_MARKER)
                m = rec_f[i, :12]
                o = xform(m, W[0][k_enter], W[1][k_enter], W[2][k_enter], 1)
                d = xform(m, W[3][k_enter], W[4][k_enter], W[5][k_enter], 0)
                for a in range(3):
                    R[a][k_enter] = o[a]
                    R[3 + a][k_enter] = d[a]
                inst[k_enter] = i
                n_off[k_enter] = rec[i, 12]
                r_off[k_enter] = rec[i, 13]
                node[k_enter] = 0
            if k_exit.size:
                for a in range(6):
                    R[a][k_exit] = W[a][k_exit]
                inst[k_exit] = -1
                pop(k_exit)
            if k_tri.size:
                row = r_off[k_tri] + ~node[k_tri]
                term = pw_u[row, 0] == TERM
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
                    node[ti] -= 3
                    if any_hit:
                        node[h] = SENTINEL
    return res_id, res_t, res_u, res_v, res_inst
