"""The instance update without a device: the numpy rule (tests/np_instance_update.py) and ntr_instances_update_host equal
np_instanced.instances byte for byte on flat input and each other over hierarchies; exact cases against hand-written words; every
error case with its bytes and all four status words; argument refusals of the host and the device form; the device form without a
device."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import instance_update_cases as uc
import instanced_scenes as isc
import np_instance_update as iu
import np_instanced as ni

F = np.float32
NEG0 = 0x80000000


def _host(local, parent, n, node, blas):
    """ntr_instances_update_host -> (instances, status, return code)"""
    try:
        inst, st = nt.instances_update_host(local, parent, n, node, blas)
        return inst, st, 0
    except nt.NtrError as e:
        return e.instances, e.status, e.code


def _both(local, parent, n, node, blas):
    """spec and host agree byte for byte -> (instances, status)"""
    want, wst = iu.update(local, parent, n, node, blas)
    got, gst, rc = _host(local, parent, n, node, blas)
    assert got.tobytes() == want.tobytes() and gst.tobytes() == wst.tobytes(), (wst, gst)
    assert rc == (-1 if wst[0] else 0)
    return want, wst


def _words(x):
    return [int(w) for w in np.asarray(x, F).view(np.uint32)]


def _w(*vals):
    """float32 words of values; the string '-0' is the negative zero"""
    return [NEG0 if isinstance(v, str) else int(np.array(v, F).view(np.uint32)) for v in vals]


# ---- flat ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "grid", "mirror"])
def test_flat_equals_np_instanced_on_the_instanced_scenes(name):
    sc = isc.scene(name)
    want = ni.instances(sc["transforms"], sc["blas"])
    got, st = _both(sc["transforms"], None, want.shape[0], None, sc["blas"])
    assert got.tobytes() == want.tobytes() and list(st) == [0, iu.NO_BAD, 0, 0]


def test_flat_equals_np_instanced_on_random_affine_matrices():
    tf = uc.random_affine(1000, 31)
    assert np.log2(np.abs(tf)).min() < -19 and np.log2(np.abs(tf)).max() > 19
    blas = np.arange(1000, dtype=np.int32) % 7
    want = ni.instances(tf, blas)
    got, st = _both(tf, None, 1000, None, blas)
    assert got.tobytes() == want.tobytes() and list(st) == [0, iu.NO_BAD, 0, 0]
    # all roots, stated: the same bytes; more nodes than instances: the first numInstances are used
    assert _both(tf, np.full(1000, -1, np.int32), 1000, None, blas)[0].tobytes() == want.tobytes()
    assert _both(tf, None, 10, None, blas[:10])[0].tobytes() == want[:10].tobytes()
    # the existing invariant: worldToObject is ntr_instance_invert(objectToWorld)
    for i in (0, 499, 999):
        assert nt.instance_invert(got["objectToWorld"][i]).tobytes() == got["worldToObject"][i].tobytes()


# ---- hierarchies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3, 16])
def test_hierarchy_host_equals_spec(depth):
    for node_array in (True, False):
        local, parent, node, blas = uc.hierarchy(70, depth, 40 + depth, node_array=node_array)
        inst, st = _both(local, parent, 70, node, blas)
        assert list(st) == [0, iu.NO_BAD, 0, 0] and np.array_equal(inst["blas"], blas) and not inst["reserved"].any()
        if depth > 1:
            chains = [iu.chain(local.shape[0], parent, i if node is None else int(node[i])) for i in range(70)]
            assert all(len(c) == depth for c in chains)
            assert any(c[j] > c[j + 1] for c in chains for j in range(depth - 1)), "no parent comes after its child"
            # worldToObject is of the rounded objectToWorld
            assert ni.invert(inst["objectToWorld"][3]).tobytes() == inst["worldToObject"][3].tobytes()


@pytest.mark.parametrize("depth", [2, 3, 16])
def test_node_order_is_free(depth):
    a = uc.hierarchy(33, depth, 7, shuffle=False)
    b = uc.hierarchy(33, depth, 7, shuffle=True)
    assert not np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert _both(a[0], a[1], 33, a[2], a[3])[0].tobytes() == _both(b[0], b[1], 33, b[2], b[3])[0].tobytes()


def test_many_instances_share_one_node():
    local, parent, node, blas = uc.hierarchy(64, 3, 9, share=16)
    inst, _ = _both(local, parent, 64, node, blas)
    assert len(set(node.tolist())) == 4
    for i in range(64):
        assert inst["objectToWorld"][i].tobytes() == inst["objectToWorld"][i // 16 * 16].tobytes()
    assert len({inst["objectToWorld"][i].tobytes() for i in range(64)}) == 4


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------
def _chain_of(mats):
    """nodes 0..m, node j's parent j - 1; one instance at the last"""
    local = np.stack(mats)
    parent = np.arange(-1, local.shape[0] - 1, dtype=np.int32)
    inst, st = _both(local, parent, 1, np.array([local.shape[0] - 1], np.int32), np.array([5], np.int32))
    assert list(st) == [0, iu.NO_BAD, 0, 0] and inst["blas"][0] == 5
    return _words(inst["objectToWorld"][0]), _words(inst["worldToObject"][0])


def test_exact_translations():
    o2w, w2o = _chain_of([uc.translation(1, 2, 3), uc.translation(10, 20, 30)])
    assert o2w == _w(1, 0, 0, 11, 0, 1, 0, 22, 0, 0, 1, 33)
    assert w2o == _w(1, 0, 0, -11, 0, 1, 0, -22, 0, 0, 1, -33)


def test_exact_power_of_two_scales():
    p, l = uc.scale(2.0), uc.scale(4.0)
    p[3], l[7] = 1.0, 1.0
    o2w, w2o = _chain_of([p, l])
    assert o2w == _w(8, 0, 0, 1, 0, 8, 0, 2, 0, 0, 8, 0)
    # the last translation is -((0 * 1 + 0 * 2) + 0.125 * 0): the negative of a positive zero
    assert w2o == _w(0.125, 0, 0, -0.125, 0, 0.125, 0, -0.25, 0, 0, 0.125, "-0")


def test_exact_quarter_turns():
    rz = np.array([0, -1, 0, 1, 1, 0, 0, 2, 0, 0, 1, 3], F)     # a quarter turn about z, then (1, 2, 3)
    rx = np.array([1, 0, 0, 4, 0, 0, -1, 5, 0, 1, 0, 6], F)     # a quarter turn about x, then (4, 5, 6)
    o2w, w2o = _chain_of([rz, rx])
    assert o2w == _w(0, 0, 1, -4, 1, 0, 0, 6, 0, 1, 0, 9)        # every zero positive: a sum of +0 and -0 is +0
    assert w2o == _w(0, 1, 0, -6, 0, 0, 1, -9, 1, 0, 0, 4)


def test_exact_chain_of_sixteen_translations():
    o2w, w2o = _chain_of([uc.translation(1.0)] * 16)
    assert o2w == _w(1, 0, 0, 16, 0, 1, 0, 0, 0, 0, 1, 0)
    assert w2o == _w(1, 0, 0, -16, 0, 1, 0, "-0", 0, 0, 1, "-0")


def test_the_chain_is_carried_in_binary64():
    """(1 + 2^-30) - 1 is 2^-30 in binary64 and 0 in binary32: the fold rounds once, at the end."""
    tiny = 2.0 ** -30
    assert F(F(1.0) + F(tiny)) == F(1.0)
    o2w, w2o = _chain_of([uc.translation(1.0), uc.translation(tiny), uc.translation(-1.0)])
    assert o2w == [0x3F800000, 0, 0, 0x30800000, 0, 0x3F800000, 0, 0, 0, 0, 0x3F800000, 0]
    assert w2o == [0x3F800000, 0, 0, 0xB0800000, 0, 0x3F800000, 0, NEG0, 0, 0, 0x3F800000, NEG0]
    # the same through scales: under a scale by 2^-30 a translation by 1 adds 2^-30 to the carried 1; the scale by 2^30 restores the
    # linear part, and the final translation by -1 leaves what binary32 would have lost
    o2w, w2o = _chain_of([uc.translation(1.0), uc.scale(tiny), uc.translation(1.0), uc.scale(2.0 ** 30), uc.translation(-1.0)])
    assert o2w == [0x3F800000, 0, 0, 0x30800000, 0, 0x3F800000, 0, 0, 0, 0, 0x3F800000, 0]
    assert w2o == [0x3F800000, 0, 0, 0xB0800000, 0, 0x3F800000, 0, NEG0, 0, 0, 0x3F800000, NEG0]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
ZERO12 = bytes(48)


@pytest.mark.parametrize("case", uc.ERROR_CASES)
def test_error_case_bytes_and_status(case):
    n, at = 8, 5
    local, parent, node, blas, bits = uc.with_errors(n, 60, [(case, at)])
    hl, hp, hn, hb = uc.hierarchy(n, 2, 60)
    good = iu.update(hl, hp, n, hn, hb)[0]
    inst, st = _both(local, parent, n, node, blas)
    bit = iu.CHAIN if case in uc.CHAIN_CASES else iu.SINGULAR
    assert bits == {at: bit} and list(st) == [bit, at, 1, 0]
    assert inst["worldToObject"][at].tobytes() == ZERO12 and inst["blas"][at] == blas[at]
    if bit == iu.CHAIN:
        assert inst["objectToWorld"][at].tobytes() == ZERO12
    else:
        o2w = inst["objectToWorld"][at]
        assert o2w.tobytes() != ZERO12
        if case == "nan":
            assert np.isnan(o2w[6]) and _words(o2w)[3] == _w(1.0)[0]
        if case == "inf":
            assert _words(o2w)[6] == 0x7F800000
        if case == "overflow":
            assert _words(o2w) == [0x7F800000, 0, 0, 0, 0, 0x7F800000, 0, 0, 0, 0, 0x7F800000, 0]
    others = np.arange(n) != at
    assert inst[others].tobytes() == good[others].tobytes()
    with pytest.raises(nt.NtrError) as e:
        nt.instances_update_host(local, parent, n, node, blas)
    assert e.value.code == -1 and "ntr_instances_update_host: instance %d " % at in str(e.value)


def test_chain_of_exactly_sixteen_is_accepted_and_seventeen_is_not():
    for m, bad in ((16, False), (17, True)):
        local = np.stack([uc.translation(1.0)] * m)
        parent = np.arange(-1, m - 1, dtype=np.int32)
        _, st = _both(local, parent, 1, np.array([m - 1], np.int32), np.zeros(1, np.int32))
        assert list(st) == ([iu.CHAIN, 0, 1, 0] if bad else [0, iu.NO_BAD, 0, 0])


def test_lowest_bad_index_and_count_with_several_bad_instances():
    placed = [("overflow", 66), ("cycle2", 9), ("nan", 64), ("node_eq_num_nodes", 130), ("zero_column", 63)]
    local, parent, node, blas, bits = uc.with_errors(131, 61, placed)
    inst, st = _both(local, parent, 131, node, blas)
    assert list(st) == [iu.CHAIN | iu.SINGULAR, 9, 5, 0]
    for i in range(131):
        assert (inst["worldToObject"][i].tobytes() == ZERO12) == (i in bits)
    # singular ones only: bit 1 alone
    local, parent, node, blas, _ = uc.with_errors(20, 62, [("inf", 19), ("zero_column", 3)])
    assert list(_both(local, parent, 20, node, blas)[1]) == [iu.SINGULAR, 3, 2, 0]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _no_device():
    cnt = C.c_int(-1)
    return not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0)


def test_host_form_refuses_bad_arguments_before_touching_anything():
    L = nt.lib()
    local, blas = np.tile(uc.IDENTITY, (4, 1)), np.zeros(4, np.int32)
    out = np.full(4, 0xAB, np.uint8).repeat(112).view(ni.INSTANCE_DTYPE)
    st = (C.c_uint32 * 4)(7, 7, 7, 7)
    p = lambda a: a.ctypes.data  # noqa: E731
    bad = [(4, None, None, 4, None, p(blas), p(out), st), (4, p(local), None, 4, None, None, p(out), st),
           (4, p(local), None, 4, None, p(blas), None, st), (4, p(local), None, 4, None, p(blas), p(out), None),
           (4, p(local), None, 0, None, p(blas), p(out), st), (0, p(local), None, 4, None, p(blas), p(out), st),
           (4, p(local), None, -1, None, p(blas), p(out), st), (3, p(local), None, 4, None, p(blas), p(out), st)]
    for args in bad:
        assert L.ntr_instances_update_host(*args) == -1 and "ntr_instances_update_host" in L.ntr_last_error().decode(), args
        assert list(st) == [7, 7, 7, 7] and (out.view(np.uint8) == 0xAB).all()
    assert "numNodes 3 < numInstances 4" in L.ntr_last_error().decode()
    # fewer nodes than instances is fine with an instanceNode array
    node = np.array([2, 2, 0, 1], np.int32)
    assert L.ntr_instances_update_host(3, p(local), None, 4, p(node), p(blas), p(out), st) == 0 and list(st) == [0, iu.NO_BAD, 0, 0]


def test_device_form_refuses_bad_arguments_before_any_device_work():
    L = nt.lib()
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16          # host memory: the checks come before anything reads it
    res = nt.InstancesUpdateResult()
    for r in (None, C.byref(res)):
        res.numInstances = 77
        bad = [(4, None, None, 4, None, a, a, a), (4, a, None, 4, None, None, a, a), (4, a, None, 4, None, a, None, a),
               (4, a, None, 4, None, a, a, None), (4, a, None, 0, None, a, a, a), (0, a, None, 4, None, a, a, a),
               (3, a, None, 4, None, a, a, a), (4, a + 4, None, 4, None, a, a, a), (4, a, None, 4, None, a, a + 8, a),
               (4, a, None, 4, None, a, a, a + 4), (4, a, a + 2, 4, None, a, a, a), (4, a, None, 4, a + 1, a, a, a)]
        for args in bad:
            assert L.ntr_instances_update(*args, r, None) == -1 and "ntr_instances_update" in L.ntr_last_error().decode(), args
        assert r is None or res.numInstances == 0          # a failed call zeroes the result
    st = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert L.ntr_instances_status_read(None, st, None) == -1 and L.ntr_instances_status_read(a, None, None) == -1
    assert L.ntr_instances_status_read(a + 4, st, None) == -1 and list(st) == [0, 0, 0, 0]
    assert (buf == 0).all()


def test_device_form_without_a_device():
    if not _no_device():
        return          # (with a device the GPU tier runs these calls)
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    for blocking in (False, True):
        with pytest.raises(nt.NtrError) as e:
            nt.instances_update(4, a, 0, 4, 0, a, a + 1024, a + 2048, blocking=blocking)
        assert e.value.code in (-2, -3), str(e.value)
    with pytest.raises(nt.NtrError) as e:
        nt.instances_status_read(a)
    assert e.value.code in (-2, -3)
    assert (buf == 0).all()
