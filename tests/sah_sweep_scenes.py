"""Scenes of the full-sweep SAH build's tests (test_sah_sweep_cpu.py, test_sah_device_gpu.py): the cases the rule's tie breaks, drop
test, empty children and depth cap are reached by."""
import numpy as np

from ntrace_amd import scenes

F = np.float32
LEAF_PREFS = ((1, 1), (1, 8), (4, 8))
NAMES = ("cornell", "soup1", "soup2", "soup3", "soup7", "soup64", "soup1000", "dropped_mix", "all_dropped", "one_live", "identical",
         "huge", "grid")


def _iota(pos):
    pos = np.asarray(pos, F).reshape(-1, 3)
    return np.arange(pos.shape[0], dtype=np.int32).reshape(-1, 3), pos


def scene(name):
    """(tri, pos) of a named scene."""
    if name == "cornell":
        return scenes.cornell_box()[:2]
    if name.startswith("soup"):
        n = int(name[4:])
        return scenes.random_soup(n, seed=100 + n, walls=False)[:2]
    if name == "dropped_mix":      # points, segments along an axis and flat-in-a-line triangles among real ones
        tri, pos = scenes.random_soup(300, seed=9, walls=False)[:2]
        tri, pos = tri.copy(), pos.copy()
        tri[::7, 1] = tri[::7, 0]
        tri[::7, 2] = tri[::7, 0]                      # points
        for k, t in enumerate(range(3, 300, 11)):      # segments along axis k % 3
            a, b, c = tri[t]
            pos[b] = pos[a]
            pos[b, k % 3] += F(1.5)
            pos[c] = pos[a]
            pos[c, k % 3] -= F(0.25)
        return tri, pos
    if name == "all_dropped":
        pos = np.zeros((30, 3), F)
        pos[:, 0] = np.arange(30, dtype=F)             # every triangle a segment along x
        return _iota(pos)
    if name == "one_live":
        pos = np.zeros((12, 3), F)
        pos[:, 1] = np.arange(12, dtype=F)
        pos[7] = (1.0, 7.0, 2.0)                       # triangle 2 is the only one with two extents
        return _iota(pos)
    if name == "identical":       # equal keys on every axis (the id tie rule) and equal sah everywhere (the balance rule)
        return _iota([(0, 0, 0), (1, 0, 0), (0, 1, 0.5)] * 40)
    if name == "huge":            # areas times counts overflow: no split wins, the all-right chain runs to the depth-64 leaf
        rng = np.random.default_rng(1)
        return _iota((rng.uniform(-1, 1, (90, 3)) * 1e19).astype(F))
    if name == "grid":            # integer coordinates, -0 / +0: many equal keys and equal costs
        rng = np.random.default_rng(2)
        pos = rng.integers(-3, 4, (3 * 500, 3)).astype(F)
        pos[rng.random(pos.shape) < 0.1] = F(-0.0)
        return _iota(pos)
    raise KeyError(name)


def buffers(r):
    """(nodes, woop, tri_index) of a spec result or a HostBvh."""
    if isinstance(r, dict):
        return r["nodes"], r["woop"], r["tri_index"]
    return r.nodes, r.woop, r.tri_index
