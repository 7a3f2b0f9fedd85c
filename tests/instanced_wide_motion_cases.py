"""The inputs of the wide motion-blur tests (tests/np_instanced_wide_motion.py is the rule): instanced_motion_cases' scenes, widened with
np_instanced_wide.widen_pool / widen_tlas at key 0 and refitted by the spec's wide motion refit."""
import numpy as np

import instanced_motion_cases as mc
import np_instanced_wide as niw
import np_instanced_wide_motion as wm

F = np.float32
_cache = {}


class WideMotionScene:
    """A MotionScene (pool, two keys, the binary tree built at key 0 and its motion refit), the wide pool, the wide top-level tree
    widened at key 0 and its wide motion refit (the spec's)."""

    def __init__(self, ms):
        self.ms, self.pool, self.inst0, self.inst1, self.n, self.root = ms, ms.pool, ms.inst0, ms.inst1, ms.n, ms.root
        self.wp = niw.widen_pool(ms.pool)
        self.wt = niw.widen_tlas(ms.built["nodes"], ms.root, ms.inst0, ms.pool["ranges"], self.wp["ranges"])
        self.refit = self.refit_of(ms.inst0, ms.inst1)

    def refit_of(self, inst0, inst1, nodes=None):
        return wm.wide_motion_refit(self.wt["nodes"] if nodes is None else nodes, self.root, self.wt["records"], self.wp["nodes"],
                                    self.pool["ranges"], self.wp["ranges"], inst0, inst1)

    def records_of(self, inst):
        """The wide records of a scene posed at `inst`: what a plain widening writes."""
        return niw.widen_tlas(None, ~0, inst, self.pool["ranges"], self.wp["ranges"])["records"]

    def trace(self, rays, any_hit=False, **kw):
        r = self.refit
        return wm.trace(r["nodes"], self.root, r["records"], r["motion_keys"], self.pool, self.wp, rays, any_hit, **kw)


def of(ms, key):
    if key not in _cache:
        _cache[key] = WideMotionScene(ms)
    return _cache[key]


def named(name):
    return of(mc.named(name), name)


def big():
    return of(mc.big(), "big")


def two_of_one(*a):
    return WideMotionScene(mc.two_of_one(*a))
