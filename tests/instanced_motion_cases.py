"""The inputs of the motion-blur tests (tests/np_instanced_motion.py is the rule): the key-1 construction used everywhere, the scenes with
their two keys and the motion-refitted tree, and the corner times."""
import numpy as np

import instanced_scenes as isc
import np_instanced as ni
import np_instanced_motion as mo

F = np.float32
SCENES = ["three", "grid", "mirror"]
INTERIOR = [0.25, 0.5, 0.8125]
# -1, 2, NaN, the smallest denormal and 1 - 2^-24: the clamp's two sides, its NaN rule, and the lerp next to its two exact ends
CORNER_TIMES = np.array([0xBF800000, 0x40000000, 0x7FC00000, 0x00000001, 0x3F7FFFFF], np.uint32).view(F)
_cache = {}


def key1_transforms(transforms, seed=3, every=False):
    """Key 1 of objectToWorld matrices (n, 12): every instance with i % 3 == 2 stays (unless `every`); every other one gets a further
    rotation about world z through an angle U(-0.6, 0.6) and its translation shifted by U(-1.5, 1.5)^3, composed in binary64 and
    rounded once."""
    rng = np.random.default_rng(seed)
    tf = np.asarray(transforms, F).reshape(-1, 12)
    out = tf.copy()
    for i in range(tf.shape[0]):
        if i % 3 == 2 and not every:
            continue
        ang, shift = rng.uniform(-0.6, 0.6), rng.uniform(-1.5, 1.5, 3)
        c, s = np.cos(ang), np.sin(ang)
        rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        m = tf[i].astype(np.float64).reshape(3, 4)
        new = np.zeros((3, 4))
        new[:, :3] = rz @ m[:, :3]
        new[:, 3] = m[:, 3] + shift
        out[i] = new.astype(F).reshape(12)
    return out


def keys_of(transforms, blas, **kw):
    """-> (inst0, inst1): INSTANCE_DTYPE arrays of the two keys"""
    return ni.instances(transforms, blas), ni.instances(key1_transforms(transforms, **kw), blas)


class MotionScene:
    """A pool, two keys, the top-level tree built at key 0 and its motion refit (the spec's)."""

    def __init__(self, pool, inst0, inst1):
        self.pool, self.inst0, self.inst1 = pool, inst0, inst1
        self.n = inst0.shape[0]
        self.built = ni.tlas_build(pool["nodes"], pool["ranges"], inst0)
        self.root = self.built["root_link"]
        self.refit = mo.motion_refit(self.built["nodes"], self.root, self.built["records"], pool["nodes"], pool["ranges"], inst0, inst1)

    def trace(self, rays, any_hit=False, **kw):
        return mo.trace(self.refit["nodes"], self.root, self.refit["records"], self.refit["motion_keys"], self.pool, rays, any_hit, **kw)


def named(name):
    if name not in _cache:
        sc = isc.scene(name)
        _cache[name] = MotionScene(isc.pool_of(sc["names"]), *keys_of(sc["transforms"], sc["blas"]))
    return _cache[name]


def big(n=300, seed=41):
    """N = 300 over cornell and soup64: more than one workgroup of the refit kernels."""
    key = ("big", n, seed)
    if key not in _cache:
        tf = isc.seeded_transforms(n, seed, spread=12.0, size=0.02)
        blas = (np.arange(n) % 2).astype(np.int32)
        _cache[key] = MotionScene(isc.pool_of(["cornell", "soup64"]), *keys_of(tf, blas))
    return _cache[key]


def cpu_rays():
    if "cpu_rays" not in _cache:
        _cache["cpu_rays"] = isc.scene_rays((96, 64), 2048)
    return _cache["cpu_rays"]


def two_of_one(m0a, m1a, m0b=None, m1b=None):
    """Two instances of the one-triangle BLAS: instance 0 with keys (m0a, m1a), instance 1 with (m0b, m1b) -- static at a fixed place
    by default.  Key 1's worldToObject is never read, so a key 1 that has no inverse is given key 0's."""
    far = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 3.0))
    m0b = far if m0b is None else m0b
    m1b = m0b if m1b is None else m1b
    inst0 = ni.instances(np.stack([m0a, m0b]), [0, 0])
    inst1 = inst0.copy()
    inst1["objectToWorld"] = np.stack([np.asarray(m1a, F), np.asarray(m1b, F)])
    return MotionScene(isc.pool_of(["one"]), inst0, inst1)


def one_rays(n=96, seed=2):
    """Rays along +z from z = -5 through the square [-1.5, 1.5]^2: they cross the plane of a one-triangle instance wherever it is placed
    along z, and about one in nine hits the triangle at its key-0 place."""
    import ntrace_amd as nt
    rng = np.random.default_rng(seed)
    r = np.zeros(n, nt.RAY_DTYPE)
    r["ox"], r["oy"] = rng.uniform(-1.5, 1.5, n).astype(F), rng.uniform(-1.5, 1.5, n).astype(F)
    r["ox"][:n // 3], r["oy"][:n // 3] = rng.uniform(0.05, 0.45, n // 3).astype(F), rng.uniform(0.05, 0.45, n // 3).astype(F)   # sure hits
    r["oz"], r["dz"], r["tmax"] = F(-5.0), F(1.0), F(100.0)
    return r
