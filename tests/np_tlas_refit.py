"""The rule of the on-device top-level refit (ntr_tlas_refit, csrc/tlas_refit_kernels.hip) in numpy.  EXTENSION: the reference has no
instancing, so this docstring, not a reference line, is the normative text.  The device's node buffer, record buffer and scene box
equal this module's byte for byte.  np_instanced.py states the pool, the instance, the record and instance_box; it is imported.

Input: a top-level tree as np_instanced.tlas_build makes it (tlas_nodes: N - 1 Compact nodes whose leaf links are ~i, root_link 0; or
no node and root_link ~0 for N == 1), its records, the pool's nodes as they are NOW (a BLAS may have been refitted since the build),
the BLAS ranges and the instances as they are NOW (new transforms, possibly new blas indices).

1. Topology stays.  Words 12..15 of every node come back untouched, and so does every word of a slot no link reaches.  Reached means,
   as in np_bvh_refit: the root (slot 0), and every slot named by a positive child word of a reached slot.
2. Record i is np_instanced.tlas_build's record for the current inst[i]: words 0..11 worldToObject, 12 nodesOffset, 13
   triWoopOffset / 16, 14 nodesBytes, 15 zero -- of the BLAS inst[i].blas names now (an instance may have switched its BLAS since the
   build, a level of detail; the record follows it).
3. Leaf box.  The box of a child whose link is ~i is np_instanced.instance_box(pool_nodes, blas_ranges[inst[i].blas],
   inst[i].objectToWorld): the pool's current node 0, eight corners, min / max in the total order, no padding.
4. Inner box.  The box of an inner child is the union of the two boxes stored in that child's node, in the np_hlbvh.f2i order
   (-0 < +0), so no result depends on the order of the operands.
5. Scene box.  For N >= 2 the union of node 0's two boxes, as min.xyz max.xyz.  For N == 1 (root_link == ~0, no node) instance 0's box,
   and only record 0 is written.
6. stats: numNodes, the reached slots; numLeaves, the leaf links of reached slots (N == 1: 0 and 1, the root link).

PLOC forms a merged cluster's box by the same integer-order union of the boxes it stores in the new node, and a leaf cluster's box is
instance_box.  It follows that refit() of a freshly built tree with unchanged instances and an unchanged pool returns nodes and records
unchanged, byte for byte.  That property ties ntr_tlas_build and ntr_tlas_refit together, and the tests demand it of the device at every
size.

7. A bad part is never followed (err_bits; the device's blocking form reports them, its asynchronous form skips silently).
   1: inst[i].blas outside [0, numBlas): record i keeps its bytes, and a leaf ~i is bad.  2: a link > 0 that names no slot (not a
   multiple of 64, or 64 * s with s >= N - 1): the child is bad.  4: a leaf link ~i with i >= N: the child is bad.  A link 0 names
   nobody and is bad without a bit, as in np_bvh_refit.  A child is WELL FORMED when it is a leaf that is not bad, or an inner link
   whose node has two well-formed children.  The box of a child is rewritten (rules 3, 4) exactly where the child is well formed;
   every other box word keeps its bytes.  The scene box is written when both children of node 0 are well formed, else it is six
   zeros here (the device leaves d_sceneBox alone and reports zeros).  Slots that only a bad link named are outside this rule; the
   tests make none.
"""
import numpy as np

import np_hlbvh
import np_instanced as ni
from np_bvh_refit import BOX_WORDS, HI, LO, _union, levels_of

F = np.float32
ERR_BLAS, ERR_LINK, ERR_LEAF = 1, 2, 4


def record_of(inst_i, blas_ranges):
    r = blas_ranges[int(inst_i["blas"])]
    rec = np.zeros(16, np.uint32)
    rec[:12] = np.asarray(inst_i["worldToObject"], F).view(np.uint32)
    rec[12], rec[13], rec[14] = r[0], r[2] // 16, r[1]
    return rec


def _box6(lo, hi):
    b = np.empty(6, F)
    b[LO], b[HI] = lo, hi
    return b


def refit(tlas_nodes, root_link, records, pool_nodes, blas_ranges, inst):
    """-> dict(nodes int32 (N - 1, 16), records uint32 (N, 16), scene_box float32[6] min.xyz max.xyz, stats, err_bits)"""
    n = inst.shape[0]
    num_blas = len(blas_ranges)
    nodes = np.ascontiguousarray(tlas_nodes).reshape(-1).view(np.int32).reshape(-1, 16).copy()
    nf = nodes.view(F)
    rec = np.ascontiguousarray(records).reshape(-1).view(np.uint32).reshape(-1, 16)[:n].copy()
    assert n >= 1 and nodes.shape[0] == n - 1 and rec.shape[0] == n and int(root_link) == (0 if n >= 2 else ~0)
    err = 0
    good_inst = (inst["blas"] >= 0) & (inst["blas"] < num_blas)
    if not good_inst.all():
        err |= ERR_BLAS
    for i in np.flatnonzero(good_inst):
        rec[i] = record_of(inst[i], blas_ranges)                                               # rule 2
    box_of = lambda i: _box6(*ni.instance_box(pool_nodes, blas_ranges[int(inst[i]["blas"])], inst[i]["objectToWorld"]))
    if n == 1:
        scene = box_of(0) if good_inst[0] else np.zeros(6, F)
        return dict(nodes=nodes, records=rec, scene_box=np.concatenate([scene[LO], scene[HI]]).astype(F),
                    stats=dict(numNodes=0, numLeaves=1), err_bits=err)

    # rule 7's tolerant walk: links that name no slot are noted and not followed
    S = n - 1
    links = nodes[:, 12:14].astype(np.int64)
    bad_link = (links > 0) & ((links % 64 != 0) | (links // 64 >= S))
    if bad_link.any():
        err |= ERR_LINK
    walk = nodes.copy()
    walk[:, 12:14][bad_link] = 0
    levels = levels_of(walk)
    reached = np.concatenate(levels)
    leaf = links[reached] < 0
    if ((~links[reached])[leaf] >= n).any():
        err |= ERR_LEAF

    well = np.zeros((S, 2), bool)                # child (slot, k) is well formed
    for slots in reversed(levels):               # deepest level first: by then both boxes inside every child node are final
        for s in slots:
            for k in (0, 1):
                c = int(links[s, k])
                if c < 0:
                    i = ~c
                    if i < n and good_inst[i]:
                        nf[s, BOX_WORDS[k]] = box_of(i)                                         # rule 3
                        well[s, k] = True
                elif c > 0 and not bad_link[s, k]:
                    ch = c // 64
                    if well[ch].all():
                        nf[s, BOX_WORDS[k]] = _union(nf[ch:ch + 1, BOX_WORDS[0]], nf[ch:ch + 1, BOX_WORDS[1]])[0]   # rule 4
                        well[s, k] = True
    if well[0].all():
        root = _union(nf[0:1, BOX_WORDS[0]], nf[0:1, BOX_WORDS[1]])[0]
        scene = np.concatenate([root[LO], root[HI]]).astype(F)
    else:
        scene = np.zeros(6, F)
    stats = dict(numNodes=int(reached.size), numLeaves=int(leaf.sum()))
    return dict(nodes=nodes, records=rec, scene_box=scene, stats=stats, err_bits=err)
