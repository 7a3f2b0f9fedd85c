"""numpy spec of ntr_bvh_optimize_batch and ntr_bvh_sah_cost_batch: treelet restructuring and SAH cost of many BLASes inside one pool.

EXTENSION: the reference has neither treelet restructuring nor instancing.  The rule is two lines.  optimize: for every entry -- a
BLAS's range (nodesOffset, nodesBytes[, triWoopOffset, triWoopBytes]), of which only the node part is read -- np_bvh_optimize.optimize
runs over that entry's node slice of the pool and the result is written back into the slice; every byte outside the entries' node
ranges stays, and the rows are not even passed.  sah_costs: np_bvh_optimize.sah_cost over every entry's node slice and row slice, so a
leaf counts its rows to the terminator inside its own BLAS's row range only.  Entries of optimize are disjoint; those of sah_costs may
repeat, since it only reads.  A BLAS whose slot 0 has fewer than 7 leaf links below it forms no treelet and so never changes.
An entry's error bits: ERR_LINK, a child link > 0 that names no slot of its own BLAS (np_bvh_optimize's bad_links; never followed, it
counts as a leaf link); ERR_NO_TREE, both link words of its slot 0 are 0, as in a zero-filled slot (nothing is reached, nothing changes).
"""
import numpy as np

import np_bvh_optimize as opt

MAX_ENTRIES = 1 << 20
ERR_LINK, ERR_ROW, ERR_NO_TREE = 1, 2, 4


def optimize(entries, nodes, passes):
    """entries: a list of ranges (nodesOffset, nodesBytes, ...); nodes: the pool's bytes.  -> dict(nodes uint8, per_entry:
    np_bvh_optimize.optimize's results, formed / rewritten: per pass, summed over the entries, heightBefore / heightAfter: per entry, before
    the first and after the last pass)."""
    nodes = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8).copy()
    per_entry = []
    for e in entries:
        no, nb = int(e[0]), int(e[1])
        r = opt.optimize(nodes[no:no + nb], passes)
        nodes[no:no + nb] = r["nodes"].reshape(-1).view(np.uint8)
        per_entry.append(r)
    formed = [sum(r["passes"][p]["formed"] for r in per_entry) for p in range(passes)]
    rewritten = [sum(r["passes"][p]["rewritten"] for r in per_entry) for p in range(passes)]
    err = []
    for e, r in zip(entries, per_entry):         # 1: a child link outside the BLAS's extent; 4: slot 0 has no child at all, so no tree
        links = nodes[int(e[0]) + 48:int(e[0]) + 56].view(np.int32)
        err.append((ERR_LINK if r["bad_links"] else 0) | (ERR_NO_TREE if not links.any() else 0))
    return dict(nodes=nodes, per_entry=per_entry, formed=formed, rewritten=rewritten, errBits=err,
                heightBefore=[r["passes"][0]["heightBefore"] for r in per_entry],
                heightAfter=[r["passes"][-1]["heightAfter"] for r in per_entry])


def sah_costs(entries, nodes, woop, dtype=np.float32):
    """-> a list of np_bvh_optimize.sah_cost results, one per entry (nodesOffset, nodesBytes, triWoopOffset, triWoopBytes)."""
    nodes = np.ascontiguousarray(nodes).reshape(-1).view(np.uint8)
    woop = np.ascontiguousarray(woop).reshape(-1).view(np.uint8)
    return [opt.sah_cost(nodes[no:no + nb], woop[wo:wo + wb], dtype) for no, nb, wo, wb in entries]
