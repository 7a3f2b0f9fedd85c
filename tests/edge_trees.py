"""Trees whose boxes sit at the ends of the range the FAST slab test admits, with triangles that stay healthy there (test helper).

A natural scene cannot get there: the host builder's Woop rows invert a matrix whose determinant grows with the fourth power of the edge
length, and a soup scaled to 2^54 (or to 2^-60) has non-finite rows and no hit at all.  Here every triangle is an axis-aligned right
triangle on an integer lattice -- corner p in [-16, 16]^3, plane axis a, legs of length l1, l2 in {1, 2, 4} and sign s1, s2 along the
other two axes b = a + 1, c = a + 2 (mod 3) -- and the lattice is mapped to the world by a per-axis power-of-two scale 2^k and a per-axis
offset.  Every vertex is then a float32, and the three Woop rows can be written down (tests/np_tracer.py reads them so):

    z = (e_a, P_a)                                      t = (P_a - o_a) / d_a
    u = (s1 / (l1 2^k_b) e_b, -s1 P_b / (l1 2^k_b))     u = s1 (h_b - P_b) / (l1 2^k_b) at the point h
    v = the same with s2, l2 and axis c

with P the corner in world coordinates.  All twelve words are float32 exactly (asserted).  The tree is the host SAH tree of these vertices
(its boxes are exact minima and maxima); the triangle rows of its Woop buffer are replaced by the rows above, and the oracle and the GPU
both trace THAT buffer, so bit-exact parity needs nothing of the host builder's own rows.

Scenes (700 triangles each, fixed seeds):

    unit       k = 0, no offset: the construction itself -- the analytic rows give the ids the host builder's own rows give.
    far        k = 31 on every axis, offset (1.5, -1.5, 1.25) 2^54: every box coordinate has a magnitude in [2^54, 2^55).
    far_top    far, and the plane coordinate of one x-plane triangle (all three of its vertices' x) moved to 2^55 - 2^31, the float below
               2^55, which is on the lattice: the largest coordinate FASTDIV admits.
    far_out    the same coordinate at exactly 2^55: FASTDIV is withheld, the same rays run GENERIC.
    tinyz      k = (0, 0, -93): the smallest non-zero |z| is exactly 2^-93, the smallest NOTINY admits.  The host builder leaves out the
               x- and y-plane triangles (their squared area underflows); the z-plane third of the lattice is the tree.  Sensitivity of
               this scene: with a divide that flushes quotients below 2^-112 to zero the zero-origin rays' inner visits change
               (14 885 -> 14 935, 13 records; test_edge_trees_cpu.py asserts it and prints the figures); with x * RN(1 / d) nothing
               moved (2049 rays), so on this scene the suite sees a lost small quotient and not a last-bit error.
    tinyz_out  k = (0, 0, -94): NOTINY is withheld, so no zero-origin ray is nice.

Ray sets are functions of a scene (rays()).  Where one axis of the scene is flatter than 2^-20 of the widest (z of the tinyz scenes), a
direction proportional to the extent cannot lie in the nice range [2^-40, 2^20] together with the other two: that component is taken
proportional to 2^-20 of the widest extent instead, and an origin component that would lie inside the flat slab (|o| < 2^-36, not nice)
stands just outside it at 1..2 x 2^-36.

    long     through the box, direction ~ extent, largest component in [1/2, 1); odd rays tmax = +inf (a miss is recorded at FLT_MAX), even
             rays tmax = 1e30, above every hit
    end_hi   the same, each ray's direction scaled by one power of two so that its largest |d| is in [2^19, 2^20)
    end_lo   ... so that its smallest |d| is in [2^-40, 2^-39)
    short    from a quarter of a lattice cell to two cells long, starting next to a triangle: the rays that take certain steps
    one_out  `long`, with one lane of every second wave just outside a nice range: GENERIC waves beside FAST waves
    zero     (tinyz scenes) oz = +-0, (ox, oy) uniform over the box, |dz| in [2^19, 2^20): z quotients of about 2^-113

For far_top and far_out every eighth ray of a set is aimed at the moved triangle instead (dx > 0, so that its origin stays below 2^55)."""
import numpy as np

import ntrace_amd as nt

from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED, expected_flags, node_words
from test_wave_setup_gpu import above, below, rule

F = np.float32
U = np.uint32
FLT_MAX = np.finfo(F).max
NUM_TRIS = 700
TOP = 2.0 ** 55 - 2.0 ** 31
FAR_OFFSET = (1.5 * 2.0 ** 54, -1.5 * 2.0 ** 54, 1.25 * 2.0 ** 54)

#            name: (seed, k per axis, offset per axis, x of the moved triangle or None)
SCENES = {
    "unit": (101, (0, 0, 0), (0.0, 0.0, 0.0), None),
    "far": (102, (31, 31, 31), FAR_OFFSET, None),
    "far_top": (102, (31, 31, 31), FAR_OFFSET, TOP),
    "far_out": (102, (31, 31, 31), FAR_OFFSET, 2.0 ** 55),
    "tinyz": (103, (0, 0, -93), (0.0, 0.0, 0.0), None),
    "tinyz_out": (103, (0, 0, -94), (0.0, 0.0, 0.0), None),
}
# the flags a scene's tree must have and must not have (the table of the module's docstring)
MUST = {
    "unit": (FINITE | FASTDIV | NOTINY | ORDERED, 0),
    "far": (FINITE | FASTDIV | NOTINY | ORDERED, 0),
    "far_top": (FINITE | FASTDIV | NOTINY | ORDERED, 0),
    "far_out": (FINITE | NOTINY | ORDERED, FASTDIV),
    "tinyz": (FINITE | FASTDIV | NOTINY | ORDERED, 0),
    "tinyz_out": (FINITE | FASTDIV | ORDERED, NOTINY),
}
SETS = ("long", "end_hi", "end_lo", "short", "one_out")
NUM_RAYS = {"long": 2049, "end_hi": 1025, "end_lo": 1025, "short": 1025, "one_out": 1025, "zero": 2049}   # whole waves and one ray


def sets_of(name):
    return SETS + (("zero",) if name.startswith("tinyz") else ())


CASES = [(s, r) for s in SCENES for r in sets_of(s)]


def exact32(x, what):
    """float64 -> float32, asserting that nothing is lost"""
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(F)
    assert np.array_equal(y.astype(np.float64), x), what + ": not exactly a float32"
    return y


class Scene:
    """.nodes, .woop, .tri_index: the Compact buffers every tracer here takes (the Woop rows are the analytic ones)"""

    def __init__(self, name):
        seed, k, offset, moved_x = SCENES[name]
        self.name = name
        rng = np.random.default_rng(seed)
        n = NUM_TRIS
        p = rng.integers(-16, 17, (n, 3)).astype(np.float64)
        a = rng.integers(0, 3, n)
        leg = rng.choice((1.0, 2.0, 4.0), (n, 2))
        sgn = rng.choice((-1.0, 1.0), (n, 2))
        b, c = (a + 1) % 3, (a + 2) % 3
        self.a = a
        scale = np.array([2.0 ** e for e in k])
        self.k, self.scale, self.offset = k, scale, np.array(offset)
        self.cell = float(scale.max())
        rows_of = np.arange(n)
        lat = np.repeat(p[:, None, :], 3, axis=1)                   # the corner and the ends of the two legs, on the lattice
        lat[rows_of, 1, b] += sgn[:, 0] * leg[:, 0]
        lat[rows_of, 2, c] += sgn[:, 1] * leg[:, 1]
        world = lat * scale + self.offset
        self.moved = None
        if moved_x is not None:
            self.moved = int(np.flatnonzero(a == 0)[0])             # an x-plane triangle: its three vertices share one x
            world[self.moved, :, 0] = moved_x
        self.world = world
        self.pos = exact32(world.reshape(-1, 3), name + " vertices")
        self.tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
        P = world[:, 0, :]                                          # the corner
        rows = np.zeros((n, 3, 4))
        rows[rows_of, 0, a] = 1.0
        rows[rows_of, 0, 3] = P[rows_of, a]
        for j, ax in ((0, b), (1, c)):
            g = sgn[:, j] / (leg[:, j] * scale[ax])
            rows[rows_of, 1 + j, ax] = g
            rows[rows_of, 1 + j, 3] = -g * P[rows_of, ax]
        rows = rows + 0.0                                           # +0.0, never -0.0: 0x80000000 in a row's first word ends a leaf
        self.rows = exact32(rows, name + " Woop rows")
        assert not (self.rows.view(U)[:, :, 0] == 0x80000000).any()
        # the cluster's box: all triangles but the moved one
        keep = np.ones(n, dtype=bool)
        if self.moved is not None:
            keep[self.moved] = False
        self.lo, self.hi = world[keep].reshape(-1, 3).min(0), world[keep].reshape(-1, 3).max(0)
        self.built = nt.sah_build(self.tri, self.pos)               # the host builder's own rows (unit compares against them)
        self.nodes, self.tri_index = self.built.nodes, self.built.tri_index
        self.woop = self._replace_rows(self.built)
        self.host = nt.HostBvh(self.nodes, self.woop, self.tri_index)
        self._rays = {}
        self._ref = {}

    def _replace_rows(self, built):
        """walk the buffer as test_wave_setup_gpu.expected_uv does: a terminator row counts 1, a triangle 3, tri_index[row] names it"""
        woop = np.frombuffer(built.woop.tobytes(), dtype=F).reshape(-1, 4).copy()
        wu = woop.view(U)
        seen = np.zeros(NUM_TRIS, dtype=bool)
        r = 0
        while r < woop.shape[0]:
            if wu[r, 0] == 0x80000000:
                r += 1
            else:
                t = int(built.tri_index[r])
                assert not seen[t]
                seen[t] = True
                woop[r:r + 3] = self.rows[t]
                r += 3
        # the host builder leaves out a triangle whose squared area underflows: the x- and y-plane triangles of the tinyz scenes
        self.in_tree = seen
        assert seen.all() or self.name.startswith("tinyz"), "every triangle has its rows in the buffer once"
        assert seen.sum() >= NUM_TRIS // 4
        return woop.reshape(-1).view(np.uint8).copy()

    def box_coordinates(self):
        return node_words(self.nodes)[:, :12].view(F).astype(np.float64)

    def flags(self):
        return expected_flags(self.nodes)

    # ---- rays ---------------------------------------------------------------------------------------------------------------------------
    def _eff(self):
        ext = self.hi - self.lo
        return np.maximum(ext, ext.max() * 2.0 ** -20), ext < ext.max() * 2.0 ** -20

    def _directions(self, rng, n):
        eff, _ = self._eff()
        q = rng.uniform(0.2, 1.0, (n, 3)) * rng.choice((-1.0, 1.0), (n, 3))
        m = np.ceil(np.log2(eff.max()))
        return q, q * eff / 2.0 ** m

    def _pack(self, o, d, tmax):
        n = o.shape[0]
        r = np.zeros(n, dtype=nt.RAY_DTYPE)
        _, flat = self._eff()
        o = o.copy()
        for ax in np.flatnonzero(flat):                              # inside a flat slab no origin is nice: stand just outside it
            out = -np.sign(d[:, ax]) * (1.0 + (np.arange(n) % 17) / 17.0) * 2.0 ** -36
            o[:, ax] = np.where(np.abs(o[:, ax]) < 2.0 ** -36, out, o[:, ax])
        r["ox"], r["oy"], r["oz"] = o[:, 0].astype(F), o[:, 1].astype(F), o[:, 2].astype(F)
        r["dx"], r["dy"], r["dz"] = d[:, 0].astype(F), d[:, 1].astype(F), d[:, 2].astype(F)
        r["tmin"], r["tmax"] = 0.0, tmax
        return r

    def _moved_box(self):
        w = self.world[self.moved]
        return w.min(0), w.max(0)

    def _long(self, seed, n):
        rng = np.random.default_rng(seed)
        eff, _ = self._eff()
        q, d = self._directions(rng, n)
        target = rng.uniform(self.lo + 0.2 * (self.hi - self.lo), self.hi - 0.2 * (self.hi - self.lo), (n, 3))
        if self.moved is not None:                                   # every eighth ray at the moved triangle, from below in x
            mlo, mhi = self._moved_box()
            sel = np.arange(n) % 8 == 5
            target[sel] = rng.uniform(mlo, mhi, (n, 3))[sel]
            q[sel, 0], d[sel, 0] = np.abs(q[sel, 0]), np.abs(d[sel, 0])
        o = target - q * eff * rng.uniform(1.0, 2.0, n)[:, None]
        tmax = np.where(np.arange(n) & 1, np.inf, 1e30).astype(F)
        return self._pack(o, d, tmax)

    def _scaled(self, rays, to_top):
        r = rays.copy()
        dd = np.abs(np.stack([r["dx"], r["dy"], r["dz"]], 1))
        _, e = np.frexp(dd.max(1) if to_top else dd.min(1))          # |d| = f 2^e, f in [1/2, 1)
        s = (2.0 ** ((20 if to_top else -39) - e.astype(np.float64))).astype(F)
        for c in ("dx", "dy", "dz"):
            r[c] = r[c] * s                                          # one power of two for all three: exact
        return r

    def _short(self, seed, n):
        rng = np.random.default_rng(seed)
        q, d = self._directions(rng, n)
        # a triangle of the tree whose plane the ray's largest component crosses (from a lattice point -- where a far origin rounds to -- a
        # plane is a whole number of cells away); where one axis is flat, any triangle of the tree
        _, flat = self._eff()
        ids = np.flatnonzero(self.in_tree)
        t = ids[rng.integers(0, ids.size, n)]
        if not flat.any():
            main = np.abs(d).argmax(1)
            for ax in range(3):
                of_ax = np.flatnonzero(self.a == ax)
                pick = of_ax[rng.integers(0, of_ax.size, n)]
                t = np.where(main == ax, pick, t)
        if self.moved is not None:
            sel = np.arange(n) % 8 == 5
            t[sel] = self.moved
            q[sel, 0], d[sel, 0] = np.abs(q[sel, 0]), np.abs(d[sel, 0])
        w = rng.uniform(0.0, 1.0, (n, 2))
        w = np.where((w.sum(1) > 1.0)[:, None], 1.0 - w, w)          # a point of the triangle
        v = self.world[t]
        point = v[:, 0] + w[:, :1] * (v[:, 1] - v[:, 0]) + w[:, 1:] * (v[:, 2] - v[:, 0])
        tmax = rng.uniform(0.25, 2.0, n) * self.cell / np.abs(d).max(1)
        # three of four end behind the point they aim at, the fourth before it (far: the origin then rounds to the lattice, half a cell off)
        ahead = np.where(np.arange(n) % 4 == 3, rng.uniform(1.2, 1.6, n), rng.uniform(0.1, 0.9, n))
        o = point - d * (tmax * ahead)[:, None]
        return self._pack(o, d, tmax.astype(F))

    def _one_out(self, seed, n):
        r = self._long(seed, n)
        rng = np.random.default_rng(seed + 1)
        values = (("dx", below(2.0 ** -40)), ("oy", F(2.0 ** 55)), ("dz", above(2.0 ** 20)), ("ox", below(2.0 ** -36)),
                  ("dy", -above(2.0 ** 20)), ("oz", -F(2.0 ** 55)), ("dx", -below(2.0 ** -40)), ("oy", -below(2.0 ** -36)))
        for w in range(1, n // 64, 2):                               # every second wave: one lane just outside
            c, v = values[(w // 2) % len(values)]
            r[c][64 * w + int(rng.integers(0, 64))] = v
        return r

    def _zero(self, seed, n):
        rng = np.random.default_rng(seed)
        r = np.zeros(n, dtype=nt.RAY_DTYPE)
        o = rng.uniform(self.lo, self.hi, (n, 3))
        r["ox"], r["oy"] = o[:, 0].astype(F), o[:, 1].astype(F)
        r["oz"] = np.where(np.arange(n) & 2, F(-0.0), F(0.0))
        d = rng.uniform(0.2, 1.0, (n, 3)) * rng.choice((-1.0, 1.0), (n, 3))
        r["dx"], r["dy"] = d[:, 0].astype(F), d[:, 1].astype(F)
        r["dz"] = (np.sign(d[:, 2]) * rng.uniform(2.0 ** 19, 2.0 ** 20, n)).astype(F)
        r["tmin"], r["tmax"] = 0.0, np.where(np.arange(n) & 1, np.inf, 1.0).astype(F)
        return r

    def rays(self, which):
        if which not in self._rays:
            n, seed = NUM_RAYS[which], 1000 + 10 * list(NUM_RAYS).index(which)
            if which == "long":
                r = self._long(seed, n)
            elif which in ("end_hi", "end_lo"):
                r = self._scaled(self._long(seed, n), which == "end_hi")
            elif which == "short":
                r = self._short(seed, n)
            elif which == "one_out":
                r = self._one_out(seed, n)
            else:
                r = self._zero(seed, n)
            r.setflags(write=False)
            self._rays[which] = r
        return self._rays[which]

    def nice(self, rays):
        """the rule of trace_lane.h on these rays under this tree's flags"""
        return rule(rays, bool(self.flags() & NOTINY))

    def reference(self, which, any_hit):
        """oracle.trace's records and counters, computed once and shared"""
        from oracle import oracle
        key = (which, bool(any_hit))
        if key not in self._ref:
            self._ref[key] = oracle.trace(self.nodes, self.woop, self.tri_index, self.rays(which), any_hit=any_hit)
        return self._ref[key]


_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = Scene(name)
    return _scenes[name]


def prefix(n):
    """a count that ends in the middle of a wave"""
    return n - 41
