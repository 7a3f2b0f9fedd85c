"""Binary trees and ray sets of the 4-wide BVH's tests (test_bvh_wide_cpu.py, test_bvh_wide_gpu.py): Compact trees of every origin the
widening pass has to take, by name, each built once."""
import numpy as np

import ntrace_amd as nt
from ntrace_amd import scenes

import instanced_scenes as isc
import np_bvh_wide as wd
import ray_sets
import sah_sweep_scenes as ss

F = np.float32
_cache = {}
_wide = {}
_rays = {}


def _nodes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int32).reshape(-1, 16).copy()


def spread(nodes, stride=2):
    """The same tree with slot s at stride * s and all-zero slots in between: an LBVH-shaped buffer with unreached zero slots."""
    ni = _nodes(nodes)
    out = np.zeros((ni.shape[0] * stride, 16), np.int32)
    out[::stride] = ni
    links = out[::stride, 12:14]
    links[links > 0] *= stride
    return out


def tree(name):
    """(nodes int32[slots, 16], woop, tri_index) of a named binary tree:
    'one' 'nested90' 'soup<N>'   the PLOC spec's tree, one triangle per leaf
    'cornell' 'grid' 'identical' the host SAH builder's tree, one triangle per leaf
    'sah8'                       the host SAH tree of soup1000 with leaves of up to eight triangles
    'spread'                     soup64's tree with all-zero slots between its nodes
    'leaves2'                    two leaves under the root: the smallest tree"""
    if name not in _cache:
        if name in ("cornell", "grid", "identical"):
            b = nt.sah_build(*ss.scene(name))
            t = (b.nodes, b.woop, b.tri_index)
        elif name == "sah8":
            b = nt.sah_build(*ss.scene("soup1000"), 4, 8)
            t = (b.nodes, b.woop, b.tri_index)
        elif name == "spread":
            t = tree("soup64")
            t = (spread(t[0]), t[1], t[2])
        elif name == "leaves2":
            t = tree("soup2")
        else:
            t = ss.buffers(isc.blas(name)[2])
        _cache[name] = (_nodes(t[0]), np.ascontiguousarray(t[1]), np.ascontiguousarray(t[2]).view(np.int32).reshape(-1))
    return _cache[name]


def wide(name):
    """np_bvh_wide.widen of tree(name), computed once."""
    if name not in _wide:
        _wide[name] = wd.widen(tree(name)[0])
    return _wide[name]


CAMERA = dict(eye=(2.0, 3.0, -34.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=50.0, far=200.0)


def degenerate_rays():
    r = scenes.random_rays(96, 9)
    r["tmax"][:32] = F(-1.0)                      # tmax < tmin
    r["tmin"][32:64] = r["tmax"][32:64] = F(3.0)  # tmin == tmax
    r["tmax"][64:] = F(np.nan)
    return r


def rays_for(name):
    """A 128 x 64 primary batch towards the scene, 4 096 random rays, ray_sets.edge_rays() and degenerate rays."""
    key = "cornell" if name == "cornell" else "soup"
    if key not in _rays:
        cam = scenes.cornell_box()[2] if name == "cornell" else scenes.random_soup(1000, seed=1100, walls=False)[2]
        _rays[key] = np.concatenate([scenes.primary_rays(cam, 128, 64)[0], scenes.random_rays(4096, 3), ray_sets.edge_rays(), degenerate_rays()])
    return _rays[key]


def deep_rays(n=1000):
    """The origin-clustered rays of the instanced deep test: most origins near the small end of nested90's chain."""
    rng = np.random.default_rng(2)
    rays = scenes.random_rays(n, 6, extent=1.0)
    for k in ("ox", "oy", "oz"):
        rays[k] = (rng.uniform(0, 1, n) ** 8 * 4.0).astype(F)
    rays["oz"] -= F(2.0)
    rays["dx"], rays["dy"], rays["dz"] = rng.normal(0, 0.1, n).astype(F), rng.normal(0, 0.1, n).astype(F), F(1.0)
    return rays
