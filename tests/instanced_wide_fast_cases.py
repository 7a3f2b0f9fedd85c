"""The inputs the FAST wide two-level tests share (test_instanced_wide_fast_cpu.py, test_instanced_wide_fast_gpu.py): the thirteen cases
of tests/instanced_fast_cases.py, each widened by the numpy spec (np_instanced_wide.widen_pool / widen_tlas, which ntr_pool_widen and
ntr_tlas_widen equal byte for byte), with the same 64 * 3 + 17 rays and the same `expect` -- which tests/test_instanced_wide_fast_cpu.py
checks from the wide spec alone, so that no device case passes by never running FAST.
One change: the wide pool has no gaps, so object_origin_zero_tiny plants its -2^-100 in a 128-byte slack slot appended behind the last
wide BLAS, which the wide pool's size covers.
A case dict: the binary case's keys, and wide_pool (bytes, slack included), wide_tlas (nodes, root_link, records)."""
import numpy as np

import instanced_fast_cases as fc
import np_instanced_wide as nw

F = np.float32
N_RAYS = fc.N_RAYS
NAMES = fc.NAMES
_cache = {}


def _build(name):
    c = dict(fc.case(name))
    pool = c["pool"]
    wp = nw.widen_pool(pool)
    wt = nw.widen_tlas(c["tlas"][0], c["tlas"][1], c["inst"], pool["ranges"], wp["ranges"])
    nodes = wp["nodes"]
    if name == "object_origin_zero_tiny":
        slack = np.zeros(32, np.uint32)
        slack[:1].view(F)[0] = F(-2.0 ** -100)           # a lo below its hi of 0: still ordered
        nodes = np.concatenate([nodes, slack.view(np.uint8)])
    c["wide_pool"] = nodes
    c["wide_tlas"] = (np.ascontiguousarray(wt["nodes"]), wt["root_link"], wt["records"])
    return c


def case(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]
