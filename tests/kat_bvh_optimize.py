"""Hand-derived known answers for ntr_bvh_optimize (one treelet) and ntr_bvh_sah_cost (two nodes), in the manner of kat_lbvh.py.

Nothing here is produced by an implementation under test: the boxes are exact binary fractions and the expected records are worked
out below from the rule in tests/np_bvh_optimize.py.  Checked by tests/test_bvh_optimize_cpu.py (numpy spec, and an independent
enumeration of all 10 395 topologies in integers) and tests/test_bvh_optimize_gpu.py (device).

THE TREELET.  Seven leaves on the x axis, every box [0, 1] in y and z, so that a box of x extent w has the area w*1 + 1*1 + 1*w =
2 w + 1 (rule 4) and the cost of a topology is 2 * (the sum of its six inner nodes' x extents) + 6; all numbers are integers far
below 2^24, exact in binary32.  Distinct power-of-two widths:

  A [0, 1]  B [1, 5]  C [-4, -2]  D [1024, 1032]  E [1032, 1048]  F [1056, 1088]  G [1088, 1152]

The leaves are linked in a scrambled order, in scrambled slots (slot 6 is not linked at all):
  slot 0 = (slot 4, slot 5)   slot 4 = (G, slot 2)   slot 2 = (A, E)   slot 5 = (slot 1, slot 3)   slot 1 = (C, F)   slot 3 = (D, B)
with the extents  slot 4: [0, 1152] = 1152   slot 2: [0, 1048] = 1048   slot 5: [-4, 1088] = 1092   slot 1: [-4, 1088] = 1092
slot 3: [1, 1032] = 1031   root: [-4, 1152] = 1156.   c_orig = 2 * (1156 + 1152 + 1048 + 1092 + 1092 + 1031) + 6 = 13148.

FORMATION (rule 3; the inner entry of the largest area is expanded, child 0 in its place, child 1 appended):
  (slot 4: 1152, slot 5: 1092)                  -> slot 4:  (G, slot 5, slot 2: 1048)
  slot 5 (1092) beats slot 2 (1048)             -> (G, slot 1: 1092, slot 2, slot 3: 1031)
  slot 1 (1092)                                 -> (G, C, slot 2, slot 3, F)
  slot 2 (1048) beats slot 3 (1031)             -> (G, C, A, slot 3, F, E)
  slot 3                                        -> (G, C, A, D, F, E, B)
so entry 0 .. 6 = G C A D F E B, and the internal slots other than the root are 4, 5, 1, 2, 3: handed out as 1, 2, 3, 4, 5.

THE OPTIMUM.  The left cluster X = {A, B, C} spans [-4, 5] (9) and the right one {D, E, F, G} spans [1024, 1152] (128); any inner
node that mixes the clusters, other than the root, spans more than 1000, so the root splits X from the rest.  On the right the chain
((D E) F) G costs 24 + 64 + 128 = 216; (D E)(F G) costs 24 + 96 + 128, and every other pairing is wider still.  In X, A u B = [0, 5]
and A u C = [-4, 1] both span 5 (THE DELIBERATE TIE), B u C spans 9.  The sum is 5 + 9 + 24 + 64 + 128 + 1156 = 1386 and
c[full] = 2 * 1386 + 6 = 2778 < 13148: the treelet is rewritten.  Exactly two topologies reach 1386 (X as (A B) C or (A C) B).

THE CHOICES (rule 5; p holds the lowest entry of s; entry i is bit i: G 1, C 2, A 4, D 8, F 16, E 32, B 64):
  s = 127: p = {G, D, F, E} = 57, the other part X = 70
  s = 57:  p = {G} = 1, the other part {D, F, E} = 56         s = 56: p = {D, E} = 40, the other part F        s = 40: p = {D}, E
  s = 70:  p must hold C.  p = 2 ({C} | {A, B}): 0 + 11;  p = 6 ({C, A} | {B}): 11 + 0;  p = 66 ({C, B} | {A}): 19.  The tie goes to the
           lowest mask, p = 2: child 0 = C, child 1 = {A, B} = 68         s = 68: p = {A}, B
EMISSION (rule 7; preorder, child 0's subtree first; slots 1, 2, 3, 4, 5 in that order):
  index 0 = slot 0 over 127: child 0 = index 1, child 1 = index 1 + (4 - 1) = 4
  index 1 = slot 1 over 57:  (G, index 2)      index 2 = slot 2 over 56: (index 3, F)      index 3 = slot 3 over 40: (D, E)
  index 4 = slot 4 over 70:  (C, index 5)      index 5 = slot 5 over 68: (A, B)
Every rewritten record gets split word 0 and keeps its fourth word; slot 6 keeps all its bytes.  The longest path holds 3 inner nodes
before (0, 4, 2) and 4 after (0, 1, 2, 3).

THE TWO-NODE TREE for the SAH cost: cubes, whose area is 2 * 3 * side^2 (6, 24, 96), so that every quotient is a binary fraction.
  slot 0 = (slot 1 with box [0, 2]^3, a leaf of 3 triangles with box [0, 4]^3)     slot 1 = (1 triangle [0, 1]^3, 2 triangles [0, 2]^3)
  slot 1: pa = 24, 1 + (6 / 24) * 1 + (24 / 24) * 2 = 3.25       slot 0: pa = 96, 1 + (24 / 96) * 3.25 + (96 / 96) * 3 = 4.8125
"""
import numpy as np

F32 = np.float32
LEAF = dict(A=(0, 1), B=(1, 5), C=(-4, -2), D=(1024, 1032), E=(1032, 1048), F=(1056, 1088), G=(1088, 1152))
LEAF_LINK = dict(A=~0, B=~40, C=~8, D=~72, E=~16, F=~100, G=~24)        # any distinct negative words
SPLIT_BEFORE = (2, 1, -1, 0, 2, 1, 1)                                     # slot 0 .. 6
FOURTH = (0x1111, 0x2222, -3, 0, 0x5555, 0x66666666, 0x7777)              # slot 0 .. 6: must survive
C_ORIG, C_FULL = 13148.0, 2778.0
HEIGHT_BEFORE, HEIGHT_AFTER = 3, 4

# slot: (child 0, its x interval, child 1, its x interval); a child is a leaf name or a slot number
BEFORE = {0: (4, (0, 1152), 5, (-4, 1088)), 4: ("G", LEAF["G"], 2, (0, 1048)), 2: ("A", LEAF["A"], "E", LEAF["E"]),
          5: (1, (-4, 1088), 3, (1, 1032)), 1: ("C", LEAF["C"], "F", LEAF["F"]), 3: ("D", LEAF["D"], "B", LEAF["B"])}
AFTER = {0: (1, (1024, 1152), 4, (-4, 5)), 1: ("G", LEAF["G"], 2, (1024, 1088)), 2: (3, (1024, 1048), "F", LEAF["F"]),
         3: ("D", LEAF["D"], "E", LEAF["E"]), 4: ("C", LEAF["C"], 5, (0, 5)), 5: ("A", LEAF["A"], "B", LEAF["B"])}


def _nodes(table, split):
    ni = np.zeros((7, 16), np.int32)
    nf = ni.view(F32)
    for slot, (c0, x0, c1, x1) in table.items():
        nf[slot, 0:4] = (x0[0], x0[1], 0, 1)
        nf[slot, 4:8] = (x1[0], x1[1], 0, 1)
        nf[slot, 8:12] = (0, 1, 0, 1)
        ni[slot, 12] = LEAF_LINK[c0] if isinstance(c0, str) else 64 * c0
        ni[slot, 13] = LEAF_LINK[c1] if isinstance(c1, str) else 64 * c1
        ni[slot, 14] = split[slot]
    ni[6, :15] = np.arange(15) * 0x01010101 + 7                            # the unlinked slot: arbitrary bytes, none of them 0
    ni[6, 12:14] = (64 * 2, ~4)                                            # ... that look like links
    ni[:, 15] = FOURTH
    return ni


def before():
    return _nodes(BEFORE, SPLIT_BEFORE)


def after():
    return _nodes(AFTER, (0, 0, 0, 0, 0, 0, SPLIT_BEFORE[6]))


# ---- the two-node tree of the SAH cost ----------------------------------------------------------------------------------
SAH_COST, SAH_SLOT1 = 4.8125, 3.25
SAH_COUNTS = dict(numNodes=2, numLeaves=3, numTris=6, height=2)


def sah_tree():
    """(nodes int32[2, 16], woop uint32[21, 4]): leaves at rows 0 (1 triangle), 4 (2 triangles), 11 (3 triangles)."""
    ni = np.zeros((2, 16), np.int32)
    nf = ni.view(F32)
    nf[0, 0:12] = (0, 2, 0, 2, 0, 4, 0, 4, 0, 2, 0, 4)
    ni[0, 12:14] = (64, ~11)
    nf[1, 0:12] = (0, 1, 0, 1, 0, 2, 0, 2, 0, 1, 0, 2)
    ni[1, 12:14] = (~0, ~4)
    w = np.full((21, 4), np.float32(1.0).view(np.uint32), np.uint32)
    w[[3, 10, 20], 0] = 0x80000000
    return ni, w
