"""ntr_bvh_validate at its thresholds and at its kernel's seams, against the two statements of tests/np_bvh_validate.py.

The buffers are cut from a real tree -- the host SAH tree of the 1000-triangle soup, seed 11 -- so that the top-of-tree table refresh at
the end of ntr_bvh_validate walks real nodes; the large ones tile it (a copy's child offsets point into the first copy).  A buffer is
uploaded once and single words are patched on the device between calls.

* every threshold value in each of the 12 box slots of the nodes 0, 63 and 64 of a 65-node buffer (two workgroups, the seam at node 64)
* words 12 to 15 of a node are not floats: patterns that read as inf, NaN, a denormal and FLT_MAX change no box flag
* the grid-stride tail: 131 072 nodes are exactly one sweep of the 2048 workgroups; 131 073 and 300 000 nodes have a second one
* NTR_BVH_WIDE_LEAVES at the ratio 7.0, for 2 leaves and for some thousands spread over many workgroups
* arguments: null pointers and the sizes check_nodes_bytes refuses"""
import ctypes as C

import numpy as np
import pytest
import torch

import ntrace_amd as nt

import np_bvh_validate as nv
from gpu_util import up
from np_bvh_validate import FASTDIV, FINITE, NOTINY, ORDERED, WIDE_LEAVES, VALUE_BITS, ORDER_PAIRS, expected_flags, node_words
from test_wave_setup_gpu import soup

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
BOX = FINITE | FASTDIV | NOTINY | ORDERED
SWEEP = 2048 * 256 // 4            # nodes one sweep of the capped grid covers
NODE_BYTES = 64
ERR_INVALID = -1                   # NTR_ERR_INVALID (include/ntrace_amd.h)
MAX_NODES_BYTES = 0x76543200       # compact_bvh.h kMaxNodesBytes: the largest multiple of 64 below the sentinel


def i32(word):
    return int(np.array([word], dtype=U).view(np.int32)[0])


def soup_nodes():
    return node_words(soup()[0].nodes).copy()


def cut(n):
    """the first n nodes of the tiled soup tree; an inner link that leaves the buffer becomes a leaf at row 0"""
    base = soup_nodes()
    w = np.tile(base, ((n + base.shape[0] - 1) // base.shape[0], 1))[:n].copy()
    ch = w[:, 12:14]
    ch[(ch >= 0) & (ch >= n * NODE_BYTES)] = ~0
    return w


class Device:
    """a node array on the device and its host copy, patched together one word at a time"""

    def __init__(self, words):
        self.host = words
        self.d = up(words)
        self.d32 = self.d.view(torch.int32)
        self.nbytes = words.nbytes

    def set(self, node, word, value):
        old = int(self.host[node, word])
        self.host[node, word] = value
        self.d32[16 * node + word] = value
        return old

    def flags(self):
        return nt.bvh_validate(self.d.data_ptr(), self.nbytes)


def ordered_after(host, node, slot):
    lo, hi = host[node, slot & ~1:(slot & ~1) + 2].view(F)
    return bool(lo <= hi)


# ---- every slot, every value -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", (0, 63, 64))
def test_every_threshold_value_in_every_box_slot(node):
    dev = Device(cut(65))
    clean = dev.flags()
    assert clean & BOX == BOX, "a cleared bit proves something only on a tree that has it"
    assert clean == expected_flags(dev.host)
    cleared_orders = 0
    for slot in range(12):
        for word, cleared in sorted(VALUE_BITS.items()):
            old = dev.set(node, slot, i32(word))
            want = clean & ~cleared
            if not ordered_after(dev.host, node, slot):
                want &= ~ORDERED
                cleared_orders += 1
            got = dev.flags()
            assert got == want, "0x%08x in slot %d of node %d: flags 0x%x, the table says 0x%x" % (word, slot, node, got, want)
            assert got == expected_flags(dev.host), "0x%08x in slot %d of node %d" % (word, slot, node)
            dev.set(node, slot, old)
    assert 12 < cleared_orders < 12 * len(VALUE_BITS) - 12
    assert dev.flags() == clean, "every word was put back"


@pytest.mark.parametrize("node", (0, 63, 64))
def test_ordered_pairs(node):
    dev = Device(cut(65))
    clean = dev.flags()
    assert clean & BOX == BOX
    for pair in range(6):
        for (lo, hi), ordered in ORDER_PAIRS.items():
            old = dev.set(node, 2 * pair, i32(lo)), dev.set(node, 2 * pair + 1, i32(hi))
            got = dev.flags()
            want = clean & ~VALUE_BITS.get(lo, 0) & ~VALUE_BITS.get(hi, 0) & ~(0 if ordered else ORDERED)
            assert got == want, "(0x%08x, 0x%08x) in pair %d of node %d: flags 0x%x, the table says 0x%x" % (lo, hi, pair, node, got, want)
            assert got == expected_flags(dev.host)
            dev.set(node, 2 * pair, old[0]), dev.set(node, 2 * pair + 1, old[1])


# ---- words 12 to 15 --------------------------------------------------------------------------------------------------------------------
def test_child_words_and_unused_words_are_not_floats():
    words = soup_nodes()
    n = words.shape[0]
    depth = np.full(n, -1)
    depth[0] = 0
    for i in range(n):                       # the host builder numbers a parent before its children
        assert depth[i] >= 0
        for c in words[i, 12:14]:
            if c >= 0:
                assert c // 64 > i
                depth[c // 64] = depth[i] + 1
    dev = Device(words)
    clean = dev.flags()
    assert clean & BOX == BOX and clean == expected_flags(dev.host)
    leaf_nodes = [i for i in range(n) if depth[i] > 3 and words[i, 12] < 0][:3] + [i for i in range(n) if depth[i] > 3 and words[i, 13] < 0][-3:]
    assert len(leaf_nodes) == 6
    stats_changed = 0
    for word in (0x7F800000, 0x7FC00000, 0xFF800000, 0x00000001, 0x7F7FFFFF):
        places = [(i, col) for i in (0, 1, 63, 64, n - 1) for col in (14, 15)]
        places += [(i, 12 if k < 3 else 13) for k, i in enumerate(leaf_nodes)]
        for node, col in places:
            old = dev.set(node, col, i32(word))
            got, want = dev.flags(), expected_flags(dev.host)
            assert got & BOX == BOX, "0x%08x in word %d of node %d read as a box coordinate: flags 0x%x" % (word, col, node, got)
            assert got == want, "0x%08x in word %d of node %d: flags 0x%x, restated 0x%x" % (word, col, node, got, want)
            stats_changed += got != clean
            dev.set(node, col, old)
    assert stats_changed >= 6, "0xFF800000 as a leaf word is a leaf at a huge offset: WIDE_LEAVES flips"
    assert dev.flags() == clean


# ---- the grid-stride tail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (SWEEP, SWEEP + 1, 300000))
def test_nodes_past_the_first_sweep_are_seen(n):
    assert SWEEP == 131072
    dev = Device(cut(n))
    clean = dev.flags()
    assert clean & BOX == BOX and not clean & WIDE_LEAVES
    assert clean == expected_flags(dev.host)
    leaves = int((dev.host[:, 12:14] < 0).sum())
    for node in sorted({SWEEP - 1, min(SWEEP, n - 1), n - 1}):
        pairs = dev.host[node, :12].view(F).reshape(6, 2)
        pair = int(np.flatnonzero((pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] > 0))[0])
        lo, hi = int(dev.host[node, 2 * pair]), int(dev.host[node, 2 * pair + 1])
        # 2^55 as a hi: FASTDIV alone
        dev.set(node, 2 * pair + 1, i32(nv.P55))
        assert dev.flags() == clean & ~VALUE_BITS[nv.P55] == clean & ~FASTDIV, "2^55 in node %d of %d" % (node, n)
        # the float below 2^-93 as that hi: NOTINY, and ORDERED when lo lies above it
        dev.set(node, 2 * pair + 1, i32(nv.M93_BELOW))
        want = clean & ~NOTINY & ~(0 if ordered_after(dev.host, node, 2 * pair) else ORDERED)
        assert dev.flags() == want, "a value below 2^-93 in node %d of %d" % (node, n)
        # the pair inverted: ORDERED alone
        dev.set(node, 2 * pair, hi), dev.set(node, 2 * pair + 1, lo)
        assert dev.flags() == clean & ~ORDERED, "an inverted pair in node %d of %d" % (node, n)
        dev.set(node, 2 * pair, lo), dev.set(node, 2 * pair + 1, hi)
    # the only leaf at the largest offset sits in the last node: with L leaves, 7 L sets WIDE_LEAVES and 7 L - 1 does not
    last = n - 1
    old = int(dev.host[last, 13])
    L = leaves + (1 if old >= 0 else 0)
    assert 7 * L > int((~dev.host[:, 12:14][dev.host[:, 12:14] < 0]).max())
    dev.set(last, 13, ~(7 * L))
    assert dev.flags() == clean | WIDE_LEAVES == expected_flags(dev.host), "the leaf at offset 7 L in the last of %d nodes" % n
    dev.set(last, 13, ~(7 * L - 1))
    assert dev.flags() == clean, "the leaf at offset 7 L - 1"
    dev.set(last, 13, old)
    assert dev.flags() == clean


# ---- the ratio -------------------------------------------------------------------------------------------------------------------------
def _hand_made(n, L, M):
    """n nodes of unit boxes; the first L have a leaf as child 1 at offsets 0, 4, 8, ... (capped below M); node L // 2 holds the leaf at M"""
    w = np.zeros((n, 16), dtype=np.int32)
    w[:, 0:12:2].view(F)[:] = -1.0
    w[:, 1:12:2].view(F)[:] = 1.0
    w[:, 12] = 64 if n > 1 else 0
    w[:, 13] = 64 if n > 1 else 0
    w[:L, 13] = ~np.minimum(4 * np.arange(L, dtype=np.int32), M - 1)
    w[L // 2, 13] = ~M
    return w


@pytest.mark.parametrize("n,L", ((2, 2), (4096, 3001), (4096, 4096)))
def test_wide_leaves_at_the_ratio_seven(n, L):
    for M, want in ((7 * L, WIDE_LEAVES), (7 * L - 1, 0)):
        w = _hand_made(n, L, M)
        assert int((w[:, 12:14] < 0).sum()) == L and int((~w[:, 12:14][w[:, 12:14] < 0]).max()) == M
        got = Device(w).flags()
        assert got == BOX | want, "L = %d, M = %d: flags 0x%x" % (L, M, got)
        assert got == expected_flags(w)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def _raw(d_nodes, nbytes, flags_ref):
    return nt.lib().ntr_bvh_validate(C.c_void_p(d_nodes), C.c_int64(nbytes), flags_ref, None)


def test_arguments():
    dev = Device(cut(3))
    ptr = dev.d.data_ptr()
    flags = C.c_uint32(0xFFFFFFFF)
    ref = C.byref(flags)
    assert _raw(ptr, dev.nbytes, None) == ERR_INVALID, "null flags"
    assert _raw(0, dev.nbytes, ref) == ERR_INVALID and flags.value == 0, "null nodes"
    # check_nodes_bytes: a multiple of 64 in [64, kMaxNodesBytes]
    for nbytes, ok in ((0, False), (63, False), (64, True), (65, False), (127, False), (128, True), (192, True), (-64, False),
                       (MAX_NODES_BYTES + 64, False), (1 << 40, False)):
        flags.value = 0xFFFFFFFF
        rc = _raw(ptr, nbytes, ref)
        assert (rc == 0) == ok and (ok or rc == ERR_INVALID), (nbytes, rc)
        if ok:
            assert flags.value == expected_flags(dev.host[:nbytes // 64]), nbytes
        else:
            assert flags.value == 0, nbytes


def test_the_largest_node_buffer_is_accepted():
    big = torch.zeros(MAX_NODES_BYTES, dtype=torch.uint8, device="cuda:0")      # all-zero nodes: boxes of zeros, no leaf
    flags = C.c_uint32(0)
    assert _raw(big.data_ptr(), MAX_NODES_BYTES, C.byref(flags)) == 0
    assert flags.value == BOX
    big.view(torch.int32)[MAX_NODES_BYTES // 4 - 16 + 11] = i32(nv.P55)             # the last box word of the last node
    assert _raw(big.data_ptr(), MAX_NODES_BYTES, C.byref(flags)) == 0
    assert flags.value == BOX & ~FASTDIV
