"""Inputs of the instance update's tests (test_instance_update_cpu.py, test_instance_update_gpu.py): seeded transform hierarchies and the
error cases of the rule (tests/np_instance_update.py), each as (local (numNodes, 12), parent or None, node or None, blas)."""
import numpy as np

import instanced_scenes as isc

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def translation(x, y=0.0, z=0.0):
    m = IDENTITY.copy()
    m[3], m[7], m[11] = x, y, z
    return m


def scale(s):
    m = IDENTITY.copy()
    m[0] = m[5] = m[10] = s
    return m


def mild(rng):
    """A transform that a chain of 16 neither blows up nor flattens: rotation x scale in [0.8, 1.25] per axis x translation within +-3."""
    return isc.transform(isc.rotation(rng), 1.25 ** rng.uniform(-1, 1, 3), rng.uniform(-3, 3, 3))


def random_affine(n, seed):
    """n matrices whose twelve entries are +-2^u, u uniform in [-20, 20]."""
    rng = np.random.default_rng(seed)
    return (rng.choice((-1.0, 1.0), (n, 12)) * 2.0 ** rng.uniform(-20, 20, (n, 12))).astype(F)


def hierarchy(n, depth, seed, shuffle=True, node_array=True, share=1):
    """n instances under a hierarchy in which every instance's chain has exactly `depth` transforms: one root, max(1, n // 64) nodes on
    every level between, and ceil(n / share) nodes on the last level (share > 1: that many instances per node); depth 1: the last level only,
    all roots.  shuffle: the nodes in a seeded order, so that parents come after children; node_array False: instance i uses node i (the
    last level's nodes stay first, the shuffle moves the others only).  blas is seeded in 0..2."""
    rng = np.random.default_rng(seed)
    last = -(-n // share)
    widths = [last] if depth == 1 else [1] + [max(1, n // 64)] * (depth - 2) + [last]
    local, parent, first = [], [], []
    for lv, w in enumerate(widths):
        first.append(len(local))
        for _ in range(w):
            local.append(mild(rng))
            parent.append(-1 if lv == 0 else first[lv - 1] + int(rng.integers(0, widths[lv - 1])))
    local, parent = np.stack(local), np.array(parent, np.int32)
    node = (first[-1] + np.arange(n) // share).astype(np.int32) if share > 1 else first[-1] + rng.permutation(n).astype(np.int32)
    num = local.shape[0]
    blas = rng.integers(0, 3, n).astype(np.int32)          # (before the shuffle's draws: the same instances in either order)
    if not node_array:
        # the last level first, in instance order: instance i uses node i
        order = np.concatenate([node, rng.permutation(first[-1]) if shuffle else np.arange(first[-1])]).astype(np.int64)
        assert share == 1
    else:
        order = rng.permutation(num) if shuffle else np.arange(num)
    new_of = np.empty(num, np.int64)
    new_of[order] = np.arange(num)
    local, parent = local[order], parent[order]
    parent = np.where(parent >= 0, new_of[np.maximum(parent, 0)], -1).astype(np.int32)
    node = new_of[node].astype(np.int32)
    if not node_array:
        assert np.array_equal(node, np.arange(n))
    return local, (None if depth == 1 and not node_array else parent), (node if node_array else None), blas


ERROR_CASES = ("chain17", "self_parent", "cycle2", "parent_eq_num_nodes", "parent_minus2", "node_minus1", "node_eq_num_nodes", "zero_column",
               "nan", "inf", "overflow")
CHAIN_CASES = ERROR_CASES[:7]


def with_errors(n, seed, placed):
    """A depth-2 hierarchy of n good instances in which each (case, i) of `placed` makes instance i bad, by nodes appended for it (NaN and
    infinite entries sit in roots: no arithmetic touches them before the rounding).  -> (local, parent, node, blas, {i: bit})."""
    local, parent, node, blas = hierarchy(n, 2, seed)
    local, parent, node = list(local), list(parent), node.copy()
    fix, bits = [], {}

    def add(m, p):
        local.append(np.asarray(m, F))
        parent.append(p)
        return len(local) - 1

    for case, i in placed:
        bits[i] = 2 if case in CHAIN_CASES else 1
        if case == "chain17":
            k = add(translation(1.0), -1)
            for _ in range(16):
                k = add(translation(1.0), k)
        elif case == "self_parent":
            k = add(IDENTITY, len(local))
        elif case == "cycle2":
            k = add(IDENTITY, len(local) + 1)
            add(IDENTITY, k)
        elif case == "parent_eq_num_nodes":
            k = add(IDENTITY, None)
            fix.append(k)
        elif case == "parent_minus2":
            k = add(IDENTITY, -2)
        elif case == "node_minus1":
            k = -1
        elif case == "node_eq_num_nodes":
            k = None
        elif case == "zero_column":
            m = IDENTITY.copy()
            m[1] = m[5] = m[9] = 0.0
            k = add(m, 0)
        elif case in ("nan", "inf"):
            m = translation(1.0, 2.0, 3.0)
            m[6] = np.nan if case == "nan" else np.inf
            k = add(m, -1)
        elif case == "overflow":
            k = add(scale(3e38), add(scale(3e38), -1))
        else:
            raise KeyError(case)
        node[i] = -7 if k is None else k
    num = len(local)
    for k in fix:
        parent[k] = num
    node = np.where(node == -7, num, node).astype(np.int32)
    return np.stack(local), np.array(parent, np.int32), node, blas, bits
