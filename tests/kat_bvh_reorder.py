"""A hand-derived known answer for ntr_bvh_reorder, in the manner of kat_bvh_optimize.py.

Nothing here is produced by an implementation under test: the expected buffers are worked out below from the rule in
tests/np_bvh_reorder.py and stated as literal tables.  Checked by tests/test_bvh_reorder_cpu.py (numpy spec) and
tests/test_bvh_reorder_gpu.py (device).

THE TREE.  Seven slots in scrambled order; five are reached:
  slot 0 = (slot 5, slot 2)        the root: two inner children
  slot 5 = (leaf A, slot 3)        a leaf in position 0, an inner child in position 1
  slot 2 = (slot 6, leaf B)        an inner child in position 0, a leaf in position 1
  slot 3 = (leaf C, leaf B)        the SAME link word as slot 2's child 1: leaf B is shared by two links
  slot 6 = (nothing, leaf D)       child word 0: LINK_NONE, the shape of the one-triangle tree's root
  slot 1   every byte 0xAB; no link reaches it (its "links" 0xABABABAB read as a leaf at row 0x54545454, far outside)
  slot 4   zero-filled; no link reaches it
Word 15 is non-zero in slots 0, 5, 3 and 6 and must travel with the node; so must the split word 14.

THE ROWS.  20 input rows, leaves out of order with rows between them that no link names (J = junk):
  rows 0-1  J       rows 2-5  D: one triangle, terminator at 5        row 6  J
  rows 7-13 B: two triangles (7-9, 10-12), terminator at 13
  rows 14-17 A: one triangle whose SECOND row (15) has x = -0.0f = 0x80000000 -- not a terminator, only rows 14 and 17 are tested
  row 18    C: no triangle, the terminator alone              row 19  J, whose x word is also 0x80000000
Terminator rows carry distinct y, z, w words and a non-zero triIndex word: they are copied bit for bit, not regenerated.

THE WALK (rule 4).  stack [0], nextSlot 1, nextRow 0.
  pop 0:  child 0 = slot 5 -> new slot 1, pushed;  child 1 = slot 2 -> new slot 2, pushed                       stack [5, 2]
  pop 2:  child 0 = slot 6 -> new slot 3, pushed;  child 1 = B (7 rows) -> rows 0-6, nextRow 7                  stack [5, 6]
  pop 6:  child 0 = nothing -> 0;                  child 1 = D (4 rows) -> rows 7-10, nextRow 11                stack [5]
  pop 5:  child 0 = A (4 rows) -> rows 11-14, nextRow 15;   child 1 = slot 3 -> new slot 4, pushed              stack [3]
  pop 3:  child 0 = C (1 row) -> row 15, nextRow 16;        child 1 = B again -> rows 16-22, nextRow 23
5 nodes, 5 leaf links, 23 rows (3 more than the input holds: B is copied twice), 2 slots dropped.

THE CLOSED FORM gives the same.  I(3) = I(6) = 1, I(5) = I(2) = 2, I(0) = 5;  W(6) = 4, W(3) = 1 + 7 = 8, W(5) = 4 + 8 = 12,
W(2) = 4 + 7 = 11, W(0) = 23.  f(0) = 1, g(0) = 0, a(0) = 2, d(0) = 0: newSlot(5) = 1, newSlot(2) = 1 + 1 = 2;
f(2) = 1 + 2 = 3, g(2) = 0;  f(5) = 1 + 2 + (I(2) - 1) = 4, g(5) = 0 + 0 + W(2) = 11.
Slot 2 (a = 1, d_0 = 0, d_1 = 7): newSlot(6) = f(2) = 3, newRow(B) = g(2) + d_0 = 0;  child 1 is no inner node, so
f(6) = 3 + 1 = 4, g(6) = 0 + 7 = 7.  Slot 6: newRow(D) = g(6) + 0 = 7.
Slot 5 (a = 1, d_0 = 4, d_1 = 0): newRow(A) = g(5) = 11, newSlot(3) = f(5) + [child 0 inner] = 4;  f(3) = 4 + 1 = 5,
g(3) = 11 + 4 = 15.  Slot 3: newRow(C) = 15, newRow(B) = 15 + 1 = 16.
"""
import numpy as np

TERM = 0x80000000
NUM_SLOTS, NUM_ROWS = 7, 20
LEAF_ROW = dict(A=14, B=7, C=18, D=2)
FOURTH = {0: 0x1111, 5: -3, 3: 0x66666666, 6: 0x7777, 2: 0}               # word 15 of the reached slots
# slot: (child 0, child 1); a child is a leaf name, a slot number or None
BEFORE = {0: (5, 2), 5: ("A", 3), 2: (6, "B"), 3: ("C", "B"), 6: (None, "D")}
# new slot: (the old slot its words 0-11, 14, 15 come from, word 12, word 13)
AFTER = [(0, 64 * 1, 64 * 2), (5, ~11, 64 * 4), (2, 64 * 3, ~0), (6, 0, ~7), (3, ~15, ~16)]
# output row: the input row it is a copy of
ROW_FROM = [7, 8, 9, 10, 11, 12, 13,   2, 3, 4, 5,   14, 15, 16, 17,   18,   7, 8, 9, 10, 11, 12, 13]
STATS = dict(numNodes=5, numLeaves=5, numRows=23, numDroppedSlots=2)


def _link(c):
    return 0 if c is None else (~LEAF_ROW[c] if isinstance(c, str) else 64 * c)


def before():
    """(nodes int32[7, 16], woop uint32[20, 4], tri_index int32[20])."""
    ni = np.zeros((NUM_SLOTS, 16), np.int32)
    for slot, (c0, c1) in BEFORE.items():
        ni.view(np.float32)[slot, 0:12] = 100.0 * slot + np.arange(12)        # twelve distinct box words per slot
        ni[slot, 12:16] = (_link(c0), _link(c1), 0x1400 + slot, FOURTH[slot])
    ni[1] = np.int32(np.uint32(0xABABABAB).view(np.int32))
    w = (0x3F000000 + 16 * np.arange(NUM_ROWS, dtype=np.uint32)[:, None] + np.arange(4, dtype=np.uint32)[None, :]).astype(np.uint32)
    w[[5, 13, 17, 18, 19], 0] = TERM                                          # the four terminators and the junk row 19
    w[15, 0] = TERM                                                           # -0.0f in the x of A's second row
    ti = (1000 + np.arange(NUM_ROWS)).astype(np.int32)
    return ni, w, ti


def after():
    """The expected (nodes int32[5, 16], woop uint32[23, 4], tri_index int32[23])."""
    ni, w, ti = before()
    out = np.zeros((len(AFTER), 16), np.int32)
    for new, (old, l0, l1) in enumerate(AFTER):
        out[new] = ni[old]
        out[new, 12:14] = (l0, l1)
    return out, w[ROW_FROM].copy(), ti[ROW_FROM].copy()
