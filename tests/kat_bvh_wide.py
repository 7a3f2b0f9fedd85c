"""A hand-derived known answer for the 4-wide BVH (tests/np_bvh_wide.py, ntr_bvh_widen): a binary tree of six nodes and seven leaves
in which the area rule expands a deeper node before a shallower one, and its wide tree written out word by word.

The binary tree (leaf Lk is the link ~(4 * k); areas are dx*dy + dy*dz + dz*dx of the box stored beside the link):

    slot 0:  slot 1  [0,8] x [0,8] x [0,8]    area 192      slot 2  [10,12] x [0,2] x [0,2]   area 12
    slot 1:  L0      [0,1] x [0,1] x [0,1]                  slot 3  [2,8] x [0,8] x [0,8]     area 160
    slot 2:  L1      [10,11] x [0,1] x [0,1]                L2      [11,12] x [1,2] x [1,2]
    slot 3:  slot 4  [2,5] x [0,8] x [0,8]    area 112      L3      [6,8] x [0,2] x [0,2]
    slot 4:  L4      [2,3] x [0,1] x [0,1]                  slot 5  [3,5] x [0,8] x [0,8]     area 96
    slot 5:  L5      [3,4] x [0,1] x [0,1]                  L6      [4,5] x [7,8] x [7,8]

Slot 0 is kept.  E = [slot 1, slot 2]; slot 1 (192) beats slot 2 (12): E = [L0, slot 3, slot 2]; now slot 3 (160), two levels down,
beats slot 2 (12), one level down: E = [L0, slot 4, L3, slot 2].  Four entries: slots 4 and 2 are kept.
Slot 2: E = [L1, L2], no inner entry.  Slot 4: E = [L4, slot 5] -> [L4, L5, L6].
Kept slots in ascending order: 0, 2, 4 -> wide nodes 0, 1, 2.  counts = [1, 1, 1], seven leaf links, height 2.
stackBound: the root holds 4 - 1 = 3; below it wide node 1 adds 2 - 1 and wide node 2 adds 3 - 1: max(3 + 1, 3 + 2) = 5."""
import numpy as np

F = np.float32


def _leaf(k):
    return ~(4 * k)


# slot: ((link, box) of child 0, (link, box) of child 1); a box is (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z)
BINARY = [
    ((64 * 1, (0, 8, 0, 8, 0, 8)), (64 * 2, (10, 12, 0, 2, 0, 2))),
    ((_leaf(0), (0, 1, 0, 1, 0, 1)), (64 * 3, (2, 8, 0, 8, 0, 8))),
    ((_leaf(1), (10, 11, 0, 1, 0, 1)), (_leaf(2), (11, 12, 1, 2, 1, 2))),
    ((64 * 4, (2, 5, 0, 8, 0, 8)), (_leaf(3), (6, 8, 0, 2, 0, 2))),
    ((_leaf(4), (2, 3, 0, 1, 0, 1)), (64 * 5, (3, 5, 0, 8, 0, 8))),
    ((_leaf(5), (3, 4, 0, 1, 0, 1)), (_leaf(6), (4, 5, 7, 8, 7, 8))),
]

# wide node: its children (link, box) in slot order; the rest of the four slots are empty
WIDE = [
    [(_leaf(0), (0, 1, 0, 1, 0, 1)), (128 * 2, (2, 5, 0, 8, 0, 8)), (_leaf(3), (6, 8, 0, 2, 0, 2)), (128 * 1, (10, 12, 0, 2, 0, 2))],
    [(_leaf(1), (10, 11, 0, 1, 0, 1)), (_leaf(2), (11, 12, 1, 2, 1, 2))],
    [(_leaf(4), (2, 3, 0, 1, 0, 1)), (_leaf(5), (3, 4, 0, 1, 0, 1)), (_leaf(6), (4, 5, 7, 8, 7, 8))],
]
KEPT = [0, 2, 4]
STATS = dict(numNodes=3, counts=[1, 1, 1], numLeafLinks=7, height=2, stackBound=5)


def before():
    """The binary node buffer, int32 [6, 16]: words 0..3 child 0's x and y, 4..7 child 1's, 8..9 child 0's z, 10..11 child 1's z,
    12 and 13 the links, 14 a split word (7: nobody reads it), 15 zero."""
    out = np.zeros((len(BINARY), 16), np.int32)
    f = out.view(F)
    for s, ((l0, b0), (l1, b1)) in enumerate(BINARY):
        f[s, 0:4] = b0[0:4]
        f[s, 4:8] = b1[0:4]
        f[s, 8:10] = b0[4:6]
        f[s, 10:12] = b1[4:6]
        out[s, 12], out[s, 13], out[s, 14] = l0, l1, 7
    return out


def after():
    """The wide node buffer, int32 [3, 32]: words 0..11 as a Compact node's for children 0 and 1, 12..15 the four links, 16..27 as
    words 0..11 for children 2 and 3, 28 the count; an empty slot holds link 0 and child 0's box."""
    out = np.zeros((len(WIDE), 32), np.int32)
    f = out.view(F)
    for w, kids in enumerate(WIDE):
        full = kids + [(0, kids[0][1])] * (4 - len(kids))
        for base, (a, b) in ((0, full[0:2]), (16, full[2:4])):
            f[w, base + 0:base + 4] = a[1][0:4]
            f[w, base + 4:base + 8] = b[1][0:4]
            f[w, base + 8:base + 10] = a[1][4:6]
            f[w, base + 10:base + 12] = b[1][4:6]
        out[w, 12:16] = [k[0] for k in full]
        out[w, 28] = len(kids)
    return out
