"""The inputs of the deforming-frame tests (tests/np_instanced_deform_frame.py is the rule): the geometry of the deforming scenes as
ntr_instanced_hit_attributes_deform takes it -- key 0's vertices, key 1's, the flag per BLAS -- hashed times and the spec's deform-traced
records per scene, and the self-occlusion demonstration: a convex cube whose second vertex key is the cube turned and stretched, so that
only the deformation moves anything and an AO ray may never hit the cube it starts from."""
import numpy as np

from ntrace_amd import scenes

import bvh_motion_cases as bc
import instanced_deform_cases as dc
import instanced_scenes as isc
import np_bvh_ploc as pl
import np_instanced as ni
from instanced_motion_frame_cases import (CUBE_POS, CUBE_TRI, DEMO_AO_SEED, DEMO_CAM, DEMO_H, DEMO_NS, DEMO_RADIUS, DEMO_W, ao_batch,  # noqa: F401
                                          records)
from test_instanced_frame_cpu import geometry

F = np.float32
SCENES = ["three", "mirror", "grid", "collapse", "three_static", "big"]
INTERIOR = dc.INTERIOR
_cache = {}


def scene_of(name):
    return dc.big() if name == "big" else dc.named(name)


def geometry_of(s, poison=False):
    """A DeformScene's meshes in ntr_instanced_hit_attributes' form -> (tri, pos0, pos1, blas_tris): pos1 holds each deforming BLAS's
    second key and, for a static BLAS, key 0's vertices again -- or NaN with `poison`: no rule may read them."""
    tri, pos0, blas_tris = geometry(s.names)
    pos1, v0 = pos0.copy(), 0
    for b, name in enumerate(s.names):
        nv = isc.blas(name)[1].shape[0]
        if s.meshes[b] is not None:
            assert s.meshes[b][1].tobytes() == pos0[v0:v0 + nv].tobytes()
            pos1[v0:v0 + nv] = s.meshes[b][2]
        elif poison:
            pos1[v0:v0 + nv] = np.nan
        v0 += nv
    return tri, pos0, pos1, blas_tris


def rays_and_times():
    """instanced_deform_cases.rays_of("cpu") and one time per ray, bvh_motion_cases.hashed_times with its planted corner values"""
    if "rays" not in _cache:
        rays = dc.rays_of("cpu")
        _cache["rays"] = (rays, bc.hashed_times(rays.shape[0]))
    return _cache["rays"]


def traced(name):
    """The spec's closest-hit records of the scene's rays at the hashed times
    -> dict(s, tri, pos0, pos1, blas_tris, deforming, keys, rays, times, res, ids)"""
    if ("traced", name) not in _cache:
        s = scene_of(name)
        rays, times = rays_and_times()
        rid, rt, ru, rv, rinst, _ = s.trace(rays, False, times=times)
        tri, pos0, pos1, blas_tris = geometry_of(s)
        _cache[("traced", name)] = dict(s=s, tri=tri, pos0=pos0, pos1=pos1, blas_tris=blas_tris, deforming=s.pool["deforming"],
                                        keys=s.refit["motion_keys"], rays=rays, times=times, res=records(rid, rt, ru, rv),
                                        ids=rinst.astype(np.int32))
    return _cache[("traced", name)]


# ---- the demonstration ------------------------------------------------------------------------------------------------------------------------
CUBE = "deform_frame_cube"      # the name the cube's mesh and build go by in instanced_scenes' table of meshes


def demo():
    """Two cube BLASes, of which BLAS 0 deforms into the cube turned and stretched; instance 0 over BLAS 0, instance 1 over BLAS 1 below
    it; key 1 of the instances is key 0 -> dict(s, tri, pos0, pos1, blas_tris, deforming, rays (pixel-table order), s2i)"""
    if "demo" not in _cache:
        pos0 = CUBE_POS
        mn, mx = pl.scene_box(pos0)
        isc._cache[CUBE] = (CUBE_TRI, pos0, pl.build(CUBE_TRI, pos0, mn, mx, 8))
        rng = np.random.default_rng(1)
        R = isc.rotation(rng)
        pos1 = (pos0.astype(np.float64) @ (R @ np.diag([1.0, 1.6, 0.7])).T + np.array([0.3, 0.1, 0.0])).astype(F)
        inst0 = ni.instances(np.stack([isc.transform(isc.rotation(rng), 5.0, (-1.0, 0.5, 0.0)), isc.transform(np.eye(3), 5.0, (0.0, -6.0, 0.0))]),
                             [0, 1])
        s = dc.DeformScene([CUBE, CUBE], inst0, inst0.copy(), {0: (pos0, pos1)})
        rays, s2i = scenes.primary_rays(DEMO_CAM, DEMO_W, DEMO_H)
        tri, p0, p1, blas_tris = geometry_of(s)
        _cache["demo"] = dict(s=s, tri=tri, pos0=p0, pos1=p1, blas_tris=blas_tris, deforming=s.pool["deforming"], rays=rays,
                              s2i=s2i.astype(np.int32))
    return _cache["demo"]
