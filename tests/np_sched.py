"""Exact numpy restatements of the scheduling layer (ntrace_amd/csrc/sched_kernels.hip) for the tests.

The library is built with -ffp-contract=off, without fast-math and with correctly rounded division, so every float32 operation of the
kernels is one IEEE operation: __frcp_rn(x) is 1 / x correctly rounded, fminf / fmaxf drop a NaN operand as np.fmin / np.fmax do, and
the one explicit fmaf is emulated exactly by fma32.  Costs, classes, orders and batch words are therefore compared for equality."""
import numpy as np

NTR_TOP_DEPTH_MAX = 10
PRED_CLASSES = 64            # NTR_SCHED_PRED_CLASSES
PRED_SAMPLE, PRED_SAMPLE2 = 100, 227
SCHED_MAX_CLASSES = 64
NTR_BATCH_DIVERGENT = 0x10000
GROUP = 64                   # blocks of one predict_kernel workgroup
_M32 = 0xFFFFFFFF
f32 = np.float32


def top_table(nodes, nodes_bytes, depth):
    """top_table_kernel: the child boxes of the inner nodes above `depth`, breadth-first from byte 0, as rows
    (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) float32.  Depth is clamped to [1, NTR_TOP_DEPTH_MAX] (ntr_launch_top_table); children are
    followed when >= 0; a node with ofs + 64 > nodes_bytes is skipped.  Row order inside a level is the kernel's atomics' on the device:
    only the multiset and the first two rows (the root's children) are defined."""
    depth = min(max(int(depth), 1), NTR_TOP_DEPTH_MAX)
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    f = raw[:raw.size // 16 * 16].view(np.float32)
    i = raw[:raw.size // 16 * 16].view(np.int32)
    rows, level = [], [0]
    for d in range(depth):
        nxt = []
        for ofs in level:
            if ofs + 64 > nodes_bytes:
                continue
            q = (ofs >> 4) * 4
            a, b, c, ch = f[q:q + 4], f[q + 4:q + 8], f[q + 8:q + 12], i[q + 12:q + 16]
            rows.append((a[0], a[1], a[2], a[3], c[0], c[1]))
            rows.append((b[0], b[1], b[2], b[3], c[2], c[3]))
            if d + 1 < depth:
                nxt += [int(x) for x in ch[:2] if x >= 0]
        level = nxt
    return np.array(rows, dtype=np.float32).reshape(-1, 6)


def fma32(a, b, c):
    """fmaf: a * b + c rounded once to float32 (round to nearest even), elementwise.  The product of two float32 is exact in float64; the
    float64 sum s is off the exact value by e (TwoSum), and rounding s to float32 goes wrong only when s lies exactly on a float32
    rounding boundary while e != 0 -- those elements are nudged one float64 step towards the exact value first."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        fin = np.isfinite(s) & np.isfinite(e) & (e != 0) & (s != 0)
        # s is a float32 rounding boundary iff s / (half a float32 ulp at |s|) is an odd integer
        _, ex = np.frexp(np.where(fin, s, 1.0))                 # |s| in [2^(ex-1), 2^ex)
        k = np.maximum(ex - 1, -126) - 23                       # float32 ulp = 2^k
        q = np.ldexp(np.where(fin, s, 1.0), -(k - 1))
        mid = fin & (q == np.floor(q)) & (np.fmod(q, 2.0) != 0)
        s = np.where(mid, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _sample_rays(rays, num_blocks, lane):
    n = rays.shape[0]
    return rays[np.minimum(np.arange(num_blocks, dtype=np.int64) * 256 + lane, n - 1)]


def block_costs(rays, table):
    """predict_kernel's box counts (ntr_predict_block_costs): per 256-ray block, the table boxes its sample ray (min(256 b + 100, n - 1))
    intersects, in the kernel's float32 operations and order."""
    n = rays.shape[0]
    nb = (n + 255) // 256
    s = _sample_rays(rays, nb, PRED_SAMPLE)
    out = np.zeros(nb, np.uint32)
    if table.shape[0] == 0:
        return out
    with np.errstate(all="ignore"):
        one = f32(1.0)
        for b0 in range(0, nb, 256):   # (in slices of blocks: the box tests of a slice are a blocks x boxes array)
            c = s[b0:b0 + 256]
            inv = [one / c[k] for k in ("dx", "dy", "dz")]
            add = [(-c[k]) * v for k, v in zip(("ox", "oy", "oz"), inv)]
            t = [[fma32(table[None, :, 2 * ax + j], inv[ax][:, None], add[ax][:, None]) for j in (0, 1)] for ax in range(3)]
            tmin, tmax = c["tmin"][:, None], c["tmax"][:, None]
            (x0, x1), (y0, y1), (z0, z1) = t
            tn = np.fmax(np.fmax(np.fmin(x0, x1), np.fmin(y0, y1)), np.fmax(np.fmin(z0, z1), tmin))
            tf = np.fmin(np.fmin(np.fmax(x0, x1), np.fmax(y0, y1)), np.fmin(np.fmax(z0, z1), tmax))
            out[b0:b0 + 256] = (tn <= tf).sum(axis=1)
    return out


def block_incoherence(rays, table, num_blocks=None):
    """block_incoherence (sched_kernels.hip) of every block: 8 = degenerate sample ray, 1 = the two samples (lanes 100 and 227, clamped
    to the last ray) start apart, 0 = they point within 60 degrees, 6 = they point apart and the sample ray reaches far, 2 = apart but
    short.  `table` rows 0 and 1 are the root's two child boxes."""
    nb = (rays.shape[0] + 255) // 256 if num_blocks is None else num_blocks
    o, o2 = _sample_rays(rays, nb, PRED_SAMPLE), _sample_rays(rays, nb, PRED_SAMPLE2)
    A, B = table[0], table[1]
    with np.errstate(all="ignore"):
        ext = np.fmax(np.fmax(np.fmax(A[1], B[1]) - np.fmin(A[0], B[0]), np.fmax(A[3], B[3]) - np.fmin(A[2], B[2])),
                      np.fmax(A[5], B[5]) - np.fmin(A[4], B[4]))
        eighth = f32(0.125) * ext
        dist = np.fmax(np.fmax(np.abs(o2["ox"] - o["ox"]), np.abs(o2["oy"] - o["oy"])), np.abs(o2["oz"] - o["oz"]))
        dot = o["dx"] * o2["dx"] + o["dy"] * o2["dy"] + o["dz"] * o2["dz"]
        l1 = o["dx"] * o["dx"] + o["dy"] * o["dy"] + o["dz"] * o["dz"]
        l2 = o2["dx"] * o2["dx"] + o2["dy"] * o2["dy"] + o2["dz"] * o2["dz"]
        together = ~((dot < f32(0.0)) | (f32(4.0) * dot * dot < l1 * l2))
        span = o["tmax"] - o["tmin"]
        reach = span * span * l1
        inc = np.where(reach > eighth * eighth, 6, 2)
        inc = np.where(together, 0, inc)
        inc = np.where(dist > eighth, 1, inc)
        inc = np.where(~(o["tmin"] < o["tmax"]), 8, inc)
    return inc.astype(np.int64)


def pool_k(origin_apart, divergence_score, num_blocks, pool_k_wide):
    """pool_k (sched_kernels.hip) in the kernel's unsigned 32-bit arithmetic."""
    a, sc, nb = int(origin_apart) & _M32, int(divergence_score) & _M32, int(num_blocks)
    k = pool_k_wide if (a > 0 and (2 * a) & _M32 >= (nb & _M32)) else 1
    div = nb > 0 and ((4 * a + sc) & _M32) >= (nb & _M32)
    return k | (NTR_BATCH_DIVERGENT if div else 0)


def coherence_words(rays, table, num_blocks, pool_k_wide):
    """[blocks whose samples start apart, divergence score, batch word]: coherence_kernel + coherence_finish_kernel, and the words
    predict_kernel + flatten_kernel derive (blocks are looked at only when the table holds >= 2 boxes)."""
    if num_blocks > 0 and table.shape[0] >= 2:
        inc = block_incoherence(rays, table, num_blocks)
        apart, score = int((inc == 1).sum()), int(4 * (inc == 6).sum() + (inc == 8).sum())
    else:
        apart = score = 0
    return [apart, score, pool_k(apart, score, num_blocks, pool_k_wide)]


def dispatch_class(cost):
    """predict_kernel's class of a block: min(cost >> 1, 63)."""
    return np.minimum(np.asarray(cost, np.int64) >> 1, PRED_CLASSES - 1)


def check_flatten_order(order, classes):
    """What flatten_kernel guarantees of a dispatch order, given every block's class: a permutation of the blocks; classes do not increase
    along it; inside one class the blocks of one group of 64 (a predict workgroup) form ONE contiguous ascending run.  The order of the
    groups among themselves follows the device's atomics and is not checked.  Returns None or the first violation (a string)."""
    order = np.asarray(order, np.int64)
    classes = np.asarray(classes, np.int64)
    nb = classes.size
    if order.size != nb or not np.array_equal(np.sort(order), np.arange(nb)):
        return "not a permutation of %d blocks" % nb
    c = classes[order]
    if np.any(np.diff(c) > 0):
        e = int(np.nonzero(np.diff(c) > 0)[0][0])
        return "class rises at position %d: %d -> %d" % (e, c[e], c[e + 1])
    for k in np.unique(c):
        seg = order[c == k]
        g = seg // GROUP
        starts = np.r_[True, g[1:] != g[:-1]]
        if int(starts.sum()) != np.unique(g).size:
            return "class %d: a group of %d blocks is split into several runs" % (k, GROUP)
        if np.any(np.diff(seg)[~starts[1:]] <= 0):
            return "class %d: a group's run is not ascending" % k
    return None


def sched_order(cost, classes):
    """sched_order_kernel: NTR_SCHED_CLASSES linear classes of the maximum cost (clamped to [1, 64]), heaviest first, blocks in buffer order
    inside a class -- a stable argsort of the class."""
    classes = min(max(int(classes), 1), SCHED_MAX_CLASSES)
    cost = np.asarray(cost, np.uint32)
    mx = cost.max() if cost.size else np.uint32(0)
    to_class = f32(classes) / (f32(mx) + f32(1.0))
    cls = (classes - 1) - np.minimum((cost.astype(np.float32) * to_class).astype(np.int64), classes - 1)
    return np.argsort(cls, kind="stable").astype(np.uint32)
