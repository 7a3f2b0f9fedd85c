"""The scenes, deformations and rays that the deformation motion blur tests share (test_bvh_motion_cpu.py, test_bvh_motion_gpu.py,
test_bvh_motion_host.py), and the comparisons of a record array with the spec's four arrays (tests/np_bvh_motion.py)."""
import numpy as np

import ntrace_amd as nt

import np_bvh_motion as bm
import np_bvh_refit as rf
import ray_sets

F = np.float32
SCENES = ("cornell", "soup1500", "flat", "zero_area", "stacked", "one")
DEFORMATIONS = (0.0, 0.02, 0.3, "collapse")
EPSILONS = (0.0, 0.001)
TIMES = (0.25, 0.37, 0.5)
_scenes, _rays, _specs = {}, {}, {}


def scene(name):
    """(tri, pos) of test_persistent_bvh_gpu._scene."""
    if name not in _scenes:
        import test_persistent_bvh_gpu as tp
        tri, pos = tp._scene(name)
        _scenes[name] = (np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(pos, F))
    return _scenes[name]


def box_rays(pos, n=4096, seed=5):
    """n seeded rays from a box around the scene toward points inside it: origin uniform(-1, 1) * (largest extent + 1) + centre, target
    uniform in the scene box; the ray runs from its origin to twice the distance of its target."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1, 1, (n, 3)) * ((hi - lo).max() + 1) + (lo + hi) / 2
    d = rng.uniform(lo, hi, (n, 3)) - o
    rays = np.zeros(n, nt.RAY_DTYPE)
    for k, c in enumerate("xyz"):
        rays["o" + c], rays["d" + c] = o[:, k].astype(F), d[:, k].astype(F)
    rays["tmin"], rays["tmax"] = 0.0, 2.0
    return rays


def rays_of(name, kind):
    """kind: "box" (4 096), "edge" (ray_sets.edge_rays), "tail" (4 097: a last wave of one lane), "single" (1)."""
    if (name, kind) not in _rays:
        pos = scene(name)[1]
        if kind == "edge":
            r = ray_sets.edge_rays(float(np.abs(pos).max()))
        else:
            r = box_rays(pos, {"box": 4096, "tail": 4097, "single": 1}[kind], {"box": 5, "tail": 6, "single": 7}[kind])
        _rays[(name, kind)] = np.ascontiguousarray(r)
    return _rays[(name, kind)]


def spec_of(key, nodes, woop, idx, tri, pos0, how, eps):
    """np_bvh_motion.motion_refit of the tree `key` names, made once; -> (spec, pos1)."""
    k = (key, how, eps)
    if k not in _specs:
        pos1 = rf.moved(pos0, how)
        _specs[k] = (bm.motion_refit(nodes, woop, idx, tri, pos0, pos1, eps), pos1)
    return _specs[k]


def hashed_times(n, seed=9):
    """Per-ray times in [0, 1) with exact 0, exact 1, NaN, -1 and 2 planted where the batch is long enough."""
    t = np.random.default_rng(seed).random(n).astype(F)
    for i, v in enumerate((0.0, 1.0, np.nan, -1.0, 2.0)):
        if 3 + 7 * i < n:
            t[3 + 7 * i] = v
    return t


def spec_trace(m, idx, rays, any_hit=False, times=None, time=0.0, stats=False):
    return bm.trace(m["nodes0"], m["nodes1"], m["vrows0"], m["vrows1"], idx, rays, any_hit, times, time, return_stats=stats)


def assert_records_equal_spec(got, ref, what):
    """got: RESULT_DTYPE records; ref: the spec's (id, t, u, v[, stats]).  All four words, bitwise."""
    assert np.array_equal(got["id"], ref[0]), (what, "id")
    for k, name in ((1, "t"), (2, "padA"), (3, "padB")):   # the record's third and fourth words are u and v
        bad = np.flatnonzero(got[name].view(np.uint32) != ref[k].view(np.uint32))
        assert bad.size == 0, (what, "tuv"[k - 1], bad.size, bad[:4])
