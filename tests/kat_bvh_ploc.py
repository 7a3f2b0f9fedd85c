"""Known answer of the PLOC rule (tests/np_bvh_ploc.py), worked by hand: six triangles, radius 2, every number a binary fraction.

Triangle T of x interval [x0, x1] is (x0,0,0), (x1,0,0), (x0,1,1): its box is [x0, x1] x [0, 1] x [0, 1].  A union of such boxes
has dy = dz = 1, so d = dx * 1 + 1 * 1 + 1 * dx = 2 * dx + 1 exactly, dx the length of the union of the x intervals.

  interval     mesh id    Morton cell on x (scene box [0,16] x [0,1] x [0,1]: 64 cells per unit; y and z cells are 512 for all)
  A [0, 1]        1        32
  B [0, 1]        3        32
  C [0, 1]        5        32
  D [4, 5]        4       288
  E [4.5, 5.5]    0       320
  F [8, 9]        2       544
With equal y and z cells the codes order as the x cells; A, B, C tie and go by id.  Sorted: A B C D E F = ids 1 3 5 4 0 2.  Leaf p
owns rows 4p .. 4p + 3, link ~(4p).

Round 1, n = 6 (candidates within 2 positions; key (d, k, b)):
  A (0): B (3, 1, 0)  C (3, 2, 0)                            -> B    a distance tie decided by k
  B (1): A (3, 1, 0)  C (3, 1, 1)  D (11, 2, 0)              -> A    a tie decided by b: (0 / 1) & 1 = 0 against (1 / 1) & 1 = 1
  C (2): B (3, 1, 1)  A (3, 2, 0)  D (11, 1, 0)  E (12, 2, 1) -> B    decided by k; B's neighbour is A, so C waits a round
  D (3): C (11, 1, 0)  B (11, 2, 0)  E (4, 1, 1)  F (11, 2, 1) -> E
  E (4): D (4, 1, 1)  C (12, 2, 1)  F (10, 1, 0)             -> D
  F (5): E (10, 1, 0)  D (11, 2, 1)                          -> E    not mutual: F waits
  Pairs (A, B) and (D, E): m = 2, slots (6 - 1 - 2) + r = 3 and 4.
Round 2, n = 4: AB [0,1] (link 192)  C  DE [4,5.5] (link 256)  F:
  AB (0): C (3, 1, 0)  DE (12, 2, 0)                         -> C
  C  (1): AB (3, 1, 0)  DE (12, 1, 1)  F (19, 2, 0)          -> AB
  DE (2): C (12, 1, 1)  AB (12, 2, 0)  F (11, 1, 0)          -> F
  F  (3): DE (11, 1, 0)  C (19, 2, 0)                        -> DE
  Pairs (AB, C) and (DE, F): slots (4 - 1 - 2) + r = 1 and 2.
Round 3, n = 2: ABC [0,1] (link 64) and DEF [4,9] (link 128) -> slot 0.  Three rounds, height 3."""
import numpy as np

F32 = np.float32
RADIUS = 2
SCENE_MIN, SCENE_MAX = np.array([0, 0, 0], F32), np.array([16, 1, 1], F32)
# in mesh order: E A F B D C
_INTERVALS = [(4.5, 5.5), (0, 1), (8, 9), (0, 1), (4, 5), (0, 1)]
SORTED_IDS = [1, 3, 5, 4, 0, 2]
NN = [[1, 0, 1, 4, 3, 4], [1, 0, 3, 2], [1, 0]]
MERGED_LOW = [[0, 3], [0, 2], [0]]
SIZES = [6, 4, 2]
STATS = dict(numNodes=5, numLeaves=6, numRounds=3, height=3)


def scene():
    pos = []
    for x0, x1 in _INTERVALS:
        pos += [(x0, 0, 0), (x1, 0, 0), (x0, 1, 1)]
    return np.arange(18, dtype=np.int32).reshape(-1, 3), np.array(pos, F32)


def _node(x0, link0, x1, link1):
    """A Compact node whose children have the x intervals x0 and x1 and the unit square on y and z."""
    nd = np.zeros(16, np.int32)
    nd.view(F32)[:12] = (x0[0], x0[1], 0, 1, x1[0], x1[1], 0, 1, 0, 1, 0, 1)
    nd[12], nd[13] = link0, link1
    return nd


def nodes():
    return np.stack([_node((0, 1), 64, (4, 9), 128),          # slot 0: ABC, DEF
                     _node((0, 1), 192, (0, 1), ~8),          # slot 1: AB, C
                     _node((4, 5.5), 256, (8, 9), ~20),       # slot 2: DE, F
                     _node((0, 1), ~0, (0, 1), ~4),           # slot 3: A, B
                     _node((4, 5), ~12, (4.5, 5.5), ~16)])    # slot 4: D, E


def tri_index():
    ti = np.zeros(24, np.int32)
    ti[0::4] = SORTED_IDS
    return ti
