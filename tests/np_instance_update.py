"""numpy spec of the instance update: ntr_instances_update (csrc/instances_update_kernels.hip) and ntr_instances_update_host
(csrc/instances_update_host.cpp).

EXTENSION: the reference has no instancing.  This docstring is the normative text; the device call and the host restatement equal
update() byte for byte.  It makes the NtrInstance array (np_instanced.INSTANCE_DTYPE) that ntr_tlas_build, ntr_tlas_refit and the
two-level traces take, from a hierarchy of transforms.

Inputs.
  nodes       numNodes transform nodes, each a `local` (3x4 row-major binary32) and a `parent` (int32, -1 for a root).  parent == None:
              every node is a root.  The order of the nodes in the array is free: a parent may come after its child.
  instances   numInstances instances, each a `node` (int32) and a `blas` (int32).  node == None: instance i uses node i, which requires
              numNodes >= numInstances.

Rule, per instance i.
  chain(i)    starting at node[i], follow parent up to a root: nodes k_0 (the root) .. k_m (the instance's own node).  At most
              MAX_CHAIN = 16 transforms (NTR_INSTANCE_MAX_CHAIN).
  compose(P, L)   in binary64 without contraction, every product rounded before the sum that uses it:
                W[r][c] = (P[r][0]*L[0][c] + P[r][1]*L[1][c]) + P[r][2]*L[2][c]                       c = 0..2
                W[r][3] = ((P[r][0]*L[0][3] + P[r][1]*L[1][3]) + P[r][2]*L[2][3]) + P[r][3]
  fold        acc = float64(local[k_0]); acc = compose(acc, float64(local[k_j])) for j = 1..m: a left fold from the root, carried in
              binary64
  objectToWorld   float32(acc): twelve roundings, once each
  worldToObject   np_instanced.invert(objectToWorld), of the ROUNDED matrix: worldToObject equals ntr_instance_invert(objectToWorld)
              bit for bit, as for every instance array of the library
  blas        copied through; reserved is zero

Errors, per instance.
  CHAIN (bit 2)      node[i] outside [0, numNodes); a parent on the way outside [-1, numNodes); more than 16 transforms (which is also
                     how a cycle shows).  objectToWorld and worldToObject are twelve +0 each.
  SINGULAR (bit 1)   invert finds a zero or non-finite determinant (a composition that overflowed to infinity in the rounding falls
                     here too).  objectToWorld as rounded, worldToObject twelve +0.
  status      four uint32 words: the OR of the bits; the lowest bad instance index, 0xFFFFFFFF if none; the number of bad instances;
              zero.
  NaNs        a NaN that arithmetic produces or passes on has the sign and payload the processor gives it, which this text does not
              fix; the tests place NaN and infinite entries in roots, where objectToWorld is the entry itself, widened and rounded back.

A flat call (parent == None, node == None) returns exactly np_instanced.instances(local, blas), byte for byte.
"""
import numpy as np

from np_instanced import INSTANCE_DTYPE, invert

F = np.float32
MAX_CHAIN = 16
SINGULAR, CHAIN = 1, 2
NO_BAD = 0xFFFFFFFF


def compose(p, l):
    """p, l: (3, 4) float64 -> (3, 4) float64."""
    w = np.zeros((3, 4), np.float64)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                w[r, c] = (p[r, 0] * l[0, c] + p[r, 1] * l[1, c]) + p[r, 2] * l[2, c]
            w[r, 3] = ((p[r, 0] * l[0, 3] + p[r, 1] * l[1, 3]) + p[r, 2] * l[2, 3]) + p[r, 3]
    return w


def chain(num_nodes, parent, start):
    """-> the node indices from the root down to `start`, or None for a CHAIN error."""
    if not 0 <= start < num_nodes:
        return None
    ks, k = [], start
    while True:
        ks.append(k)
        p = -1 if parent is None else int(parent[k])
        if p == -1:
            return ks[::-1]
        if not 0 <= p < num_nodes or len(ks) == MAX_CHAIN:
            return None
        k = p


def update(local, parent, num_instances, node, blas):
    """local: (numNodes, 12); parent: (numNodes,) or None; node: (numInstances,) or None; blas: (numInstances,)
    -> (INSTANCE_DTYPE array, status: 4 uint32)."""
    local = np.asarray(local, F).reshape(-1, 12)
    num_nodes = local.shape[0]
    assert num_nodes >= 1 and num_instances >= 1 and (node is not None or num_nodes >= num_instances)
    parent = None if parent is None else np.asarray(parent, np.int32).reshape(num_nodes)
    node = None if node is None else np.asarray(node, np.int32).reshape(num_instances)
    inst = np.zeros(num_instances, INSTANCE_DTYPE)
    inst["blas"] = np.asarray(blas, np.int32).reshape(num_instances)
    bits, first, count = 0, NO_BAD, 0
    for i in range(num_instances):
        ks = chain(num_nodes, parent, i if node is None else int(node[i]))
        if ks is None:
            bad = CHAIN
        else:
            acc = local[ks[0]].reshape(3, 4).astype(np.float64)
            for k in ks[1:]:
                acc = compose(acc, local[k].reshape(3, 4).astype(np.float64))
            with np.errstate(all="ignore"):
                inst["objectToWorld"][i] = acc.astype(F).reshape(12)
            try:
                inst["worldToObject"][i] = invert(inst["objectToWorld"][i])
                bad = 0
            except ValueError:
                bad = SINGULAR
        if bad:
            bits |= bad
            first = min(first, i)
            count += 1
    return inst, np.array([bits, first, count, 0], np.uint32)
