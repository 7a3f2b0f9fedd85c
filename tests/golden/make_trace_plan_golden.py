"""Generates tests/golden/plan/trace_plan.npz (its own directory: every .npz directly under tests/golden/ is a trace fixture, which
tests/test_oracle_cpu.py replays): ntr_trace_plan's answer (every field of NtrTracePlan) over a grid of batches, under the default
tunables and under each tunable that steers the plan.  tests/test_trace_plan_cpu.py recomputes every row and compares.

The fixture freezes the launch policy of trace_plan.h: a change to the plan is a deliberate, visible edit of this fixture, never a
side effect of a refactor.  Re-run: python tests/golden/make_trace_plan_golden.py
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ntrace_amd as nt  # noqa: E402

MB = 1 << 20
KERNELS = ("fermi_speculative_while_while", "tesla_persistent_while_while", "tesla_persistent_speculative_while_while", "kepler_dynamic_fetch")
# the tunables that steer the plan, one per configuration ("" = the defaults)
CONFIGS = ("", "NTR_TRACE_ROUTE=0", "NTR_TRACE_MINIPOOL=0", "NTR_TRACE_MINIPOOL=4", "NTR_TRACE_PREDICT=0", "NTR_TRACE_PERSISTENT_HINTS=0",
           "NTR_TRACE_UNIFIED=0", "NTR_TRACE_CHUNK=48", "NTR_TRACE_FLAT_FETCH=0")
# around every size threshold of the plan: auto hint (2^17 rays), prediction (2^20), wide mini-pool (3 * 2^19 rays, 32 MB of nodes)
RAYS = (1, 63, 1000, (1 << 17) - 1, 1 << 17, 3 * (1 << 19) - 1, (1 << 20) - 1, 1 << 20, 1920 * 1080, 1 << 21)
TREES = ((6400, 4800), (17 * MB, 17 * MB), (32 * MB - 64, 32 * MB), (32 * MB, 32 * MB - 64), (600 * MB, 700 * MB))
PLAN_FLAGS = (0, nt._capi.PLAN_FLAG_STATS, nt._capi.PLAN_FLAG_CAPTURING, nt._capi.PLAN_FLAG_CALLER_HINT)
BVH_FLAGS = (0, nt.BVH_WIDE_LEAVES, nt.BVH_ORDERED | nt.BVH_FASTDIV)
# the node buffer lies at NODES_GIB GiB; the Woop buffer follows it (one 4 GiB window) or lies 5 GiB above it (two windows)
NODES_GIB = 4
TWO_WINDOWS_OFS64 = (5 << 30) // 64
INPUTS = ("config", "kernel", "any_hit", "num_rays", "nodes_bytes", "woop_bytes", "woop_ofs64", "bvh_flags", "num_cus", "flags")


def batches(config):
    """The grid: the full product of kernels, ray kinds, ray counts, trees and plan flags under the defaults, plus BVH flags, CU counts
    and windows on fewer counts and trees; under a tunable, the counts and trees around its thresholds."""
    if config == "":
        for k, a, n, (nb, wb), f in itertools.product(range(len(KERNELS)), (0, 1), RAYS, TREES, PLAN_FLAGS):
            yield k, a, n, nb, wb, nb // 64, 0, 256, f
        for k, a, n, (nb, wb), bf, cus, two in itertools.product(range(len(KERNELS)), (0, 1), (1000, 1 << 20, 1 << 21), TREES[1::3],
                                                                  BVH_FLAGS, (1, 256), (False, True)):
            if (bf, cus, two) != (0, 256, False):
                yield k, a, n, nb, wb, TWO_WINDOWS_OFS64 if two else nb // 64, bf, cus, 0
    else:
        for k, a, n, (nb, wb), f in itertools.product(range(len(KERNELS)), (0, 1), (1000, 1 << 17, 3 * (1 << 19), 1 << 20, 1 << 21),
                                                      TREES[:2] + TREES[3:], PLAN_FLAGS[:2]):
            yield k, a, n, nb, wb, nb // 64, 0, 256, f


def plan(kernel, any_hit, num_rays, nodes_bytes, woop_bytes, woop_ofs64, bvh_flags, num_cus, flags):
    nodes_addr = NODES_GIB << 30
    p = nt.trace_plan(KERNELS[kernel], num_rays, any_hit, nodes_bytes, woop_bytes, nodes_addr=nodes_addr, woop_addr=nodes_addr + woop_ofs64 * 64,
                      bvh_flags=bvh_flags, num_cus=num_cus, flags=flags)
    return [getattr(p, name) for name, _ in nt._capi.TracePlan._fields_]


def set_config(config):
    for k in list(os.environ):
        if k.startswith("NTR_"):
            del os.environ[k]
    name, _, value = config.partition("=")
    nt.set_tunables(**({name: value} if name else {}))


if __name__ == "__main__":
    inputs, plans = [], []
    for c, config in enumerate(CONFIGS):
        set_config(config)
        for b in batches(config):
            inputs.append((c,) + b)
            plans.append(plan(*b))
    set_config("")
    os.makedirs(os.path.join(HERE, "plan"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "plan", "trace_plan.npz"), configs=np.array(CONFIGS), kernels=np.array(KERNELS),
                        inputs_names=np.array(INPUTS), fields=np.array([n for n, _ in nt._capi.TracePlan._fields_]),
                        inputs=np.array(inputs, dtype=np.int32), plans=np.array(plans, dtype=np.int32), nodes_gib=np.int32(NODES_GIB))
    print("trace_plan rows", len(inputs))
