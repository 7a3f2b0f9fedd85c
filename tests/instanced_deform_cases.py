"""The inputs of the deforming-BLAS tests (tests/np_instanced_deform.py is the rule): instanced scenes whose pool has a second key for
some BLASes, built on instanced_motion_cases (the instances' two keys) and np_bvh_refit.moved (the meshes' second key), and the ray sets."""
import numpy as np

import instanced_motion_cases as mc
import instanced_scenes as isc
import np_bvh_refit as rf
import np_instanced as ni
import np_instanced_deform as nd

F = np.float32
SCENES = ["three", "mirror", "grid"]
INTERIOR = mc.INTERIOR
CORNER_TIMES = mc.CORNER_TIMES
_cache = {}


class DeformScene:
    """A pool with key 1 for its deforming BLASes, two keys of the instances, the top-level tree built at key 0 over the refitted pool
    and its deform refit (the spec's).  deforming: {blas index: amplitude for np_bvh_refit.deform, or "collapse", or the mesh's two
    position arrays (pos0, pos1) themselves}."""

    def __init__(self, names, inst0, inst1, deforming, epsilon=0.0):
        self.names, self.inst0, self.inst1, self.how = list(names), inst0, inst1, dict(deforming)
        self.n = inst0.shape[0]
        self.meshes = []
        for b, name in enumerate(self.names):
            tri, pos, _ = isc.blas(name)
            if b not in self.how:
                self.meshes.append(None)
            elif isinstance(self.how[b], tuple):
                self.meshes.append((tri, np.ascontiguousarray(self.how[b][0], F), np.ascontiguousarray(self.how[b][1], F)))
            else:
                self.meshes.append((tri, pos, rf.moved(pos, self.how[b])))
        self.pool = nd.pool_motion_refit(isc.pool_of(self.names), self.meshes, epsilon)
        self.ranges = self.pool["ranges"]
        self.built = ni.tlas_build(self.pool["nodes"], self.ranges, inst0)
        self.root = self.built["root_link"]
        self.refit = nd.deform_refit(self.built["nodes"], self.root, self.built["records"], self.pool["nodes"], self.pool["nodes1"], self.ranges,
                                     self.pool["deforming"], inst0, inst1)

    def trace(self, rays, any_hit=False, **kw):
        return nd.trace(self.refit["nodes"], self.root, self.refit["records"], self.refit["motion_keys"], self.pool, rays, any_hit, **kw)

    def blas_slices(self, b):
        """BLAS b's slices of the pool as np_bvh_motion.motion_refit's dict (nodes0, nodes1, woop, vrows0, vrows1) and its tri_index"""
        n_off, n_bytes, w_off, w_bytes = self.ranges[b]
        p = self.pool
        m = dict(nodes0=p["nodes"][n_off:n_off + n_bytes].view(np.int32).reshape(-1, 16), nodes1=p["nodes1"][n_off:n_off + n_bytes].view(np.int32).reshape(-1, 16),
                 woop=p["woop"][w_off:w_off + w_bytes], vrows0=p["vrows0"][w_off:w_off + w_bytes].view(np.uint32).reshape(-1, 4),
                 vrows1=p["vrows1"][w_off:w_off + w_bytes].view(np.uint32).reshape(-1, 4))
        return m, p["tri_index"][w_off // 16:(w_off + w_bytes) // 16]


def scene_of(name, deforming, every=False, seed=3, static=False):
    sc = isc.scene(name)
    inst0 = ni.instances(sc["transforms"], sc["blas"])
    inst1 = inst0 if static else ni.instances(mc.key1_transforms(sc["transforms"], seed=seed, every=every), sc["blas"])
    return DeformScene(sc["names"], inst0, inst1, deforming)


def named(name):
    """three: only BLAS 1 (soup1000) deforms, so waves mix static and deforming lanes.  mirror: two negatively scaled instances of the
    one deforming BLAS.  grid: the Cornell BLAS deforms and every instance moves -- the four-box case.  three_static: `three`, nothing
    deforming.  collapse: `three` whose BLAS 2 collapses to a point at key 1 -- degenerate posed triangles."""
    if name not in _cache:
        _cache[name] = {"three": lambda: scene_of("three", {1: 0.3}), "mirror": lambda: scene_of("mirror", {0: 0.3}),
                        "grid": lambda: scene_of("grid", {0: 0.3}, every=True), "three_static": lambda: scene_of("three", {}),
                        "collapse": lambda: scene_of("three", {2: "collapse"})}[name]()
    return _cache[name]


def big(n=300, seed=41):
    """N = 300 over cornell and soup64, of which soup64 deforms: more than one workgroup of the refit kernels."""
    key = ("big", n, seed)
    if key not in _cache:
        tf = isc.seeded_transforms(n, seed, spread=12.0, size=0.02)
        blas = (np.arange(n) % 2).astype(np.int32)
        _cache[key] = DeformScene(["cornell", "soup64"], *mc.keys_of(tf, blas), {1: 0.3})
    return _cache[key]


def two_of_one(m0a, m1a, how=0.3, m0b=None, m1b=None):
    """instanced_motion_cases.two_of_one with the one-triangle BLAS deforming."""
    far = isc.transform(np.eye(3), 1.0, (0.0, 0.0, 3.0))
    m0b = far if m0b is None else m0b
    m1b = m0b if m1b is None else m1b
    inst0 = ni.instances(np.stack([m0a, m0b]), [0, 0])
    inst1 = inst0.copy()
    inst1["objectToWorld"] = np.stack([np.asarray(m1a, F), np.asarray(m1b, F)])
    return DeformScene(["one"], inst0, inst1, {} if how is None else {0: how})


def rays_of(kind):
    """cpu: instanced_motion_cases.cpu_rays (8 192); tail: 4 097, whose last wave has one lane; single: 1; odd: instanced_scenes.odd_rays"""
    if ("rays", kind) not in _cache:
        _cache[("rays", kind)] = {"cpu": mc.cpu_rays, "tail": lambda: isc.scene_rays((64, 32), 2049, seed=6),
                                  "single": lambda: isc.scene_rays((64, 32), 2049, seed=6)[1000:1001], "odd": isc.odd_rays}[kind]()
    return _cache[("rays", kind)]


def posed_scene(s, tau):
    """The static scene that s IS at the scalar time tau: (pool with np_bvh_motion.posed_static_tree per deforming BLAS, instances with
    lerped transforms, the posed meshes' (tri, pos) per BLAS)."""
    import np_bvh_motion as bm
    import np_instanced_motion as mo
    t = mo.clamp_time(F(tau))
    nodes, woop = s.pool["nodes"].copy(), s.pool["woop"].copy()
    meshes = []
    for b, name in enumerate(s.names):
        tri, pos, _ = isc.blas(name)
        if s.meshes[b] is None:
            meshes.append((tri, pos))
            continue
        m, tidx = s.blas_slices(b)
        pn, pw = bm.posed_static_tree(m, tidx, tri, s.meshes[b][1], s.meshes[b][2], t)
        n_off, n_bytes, w_off, w_bytes = s.ranges[b]
        nodes[n_off:n_off + n_bytes] = pn.view(np.uint8).reshape(-1)
        woop[w_off:w_off + w_bytes] = pw
        meshes.append((tri, bm.deform_lerp(s.meshes[b][1], s.meshes[b][2], t)))
    tf = mo.lerp(s.inst0["objectToWorld"], s.inst1["objectToWorld"], t)
    pool = dict(nodes=nodes, woop=woop, tri_index=s.pool["tri_index"], ranges=s.ranges)
    return pool, ni.instances(tf, s.inst0["blas"]), meshes


def world_triangles(inst, meshes):
    """The world-space triangles of instances over (tri, pos) meshes in binary64: (n, 3, 3)."""
    verts = []
    for m, b in zip(inst["objectToWorld"], inst["blas"]):
        tri, pos = meshes[int(b)]
        m = m.astype(np.float64).reshape(3, 4)
        verts.append((np.asarray(pos, np.float64) @ m[:, :3].T + m[:, 3])[tri])
    return np.concatenate(verts)
