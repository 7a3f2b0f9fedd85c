"""ntr_instances_update on the device against the numpy rule (tests/np_instance_update.py), byte for byte: every word of the instance
array and all four status words.  d_instances and d_status carry 64 bytes of 0xAB beyond their extents, which must stay.  The sizes
are the smallest where the launch can go wrong: one instance, less than a wave, a wave edge, more than one workgroup; the chains are
the lengths 1, 2, 3 and the limit 16.  The error tests compare written bytes only: nothing is traced through a bad instance."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instance_update_cases as uc
import instanced_scenes as isc
import np_instance_update as iu
import np_instanced as ni
from gpu_util import up
from test_tlas_refit_gpu import _Tlas, _assert_trace, _trace

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 64
CLEAN = [0, iu.NO_BAD, 0, 0]


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


class _Update:
    """The inputs of one update on the device and 0xAB-bordered outputs."""

    def __init__(self, local, parent, n, node, blas):
        self.n, self.num_nodes = n, np.asarray(local).reshape(-1, 12).shape[0]
        self.d_local = up(np.asarray(local, F))
        self.d_parent = None if parent is None else up(np.asarray(parent, np.int32))
        self.d_node = None if node is None else up(np.asarray(node, np.int32))
        self.d_blas = up(np.asarray(blas, np.int32))
        self.d_inst, self.d_status = _filled(112 * n), _filled(16)

    def run(self, blocking=True, stream=0):
        return nt.instances_update(self.num_nodes, self.d_local.data_ptr(), 0 if self.d_parent is None else self.d_parent.data_ptr(), self.n,
                                   0 if self.d_node is None else self.d_node.data_ptr(), self.d_blas.data_ptr(), self.d_inst.data_ptr(),
                                   self.d_status.data_ptr(), stream=stream, blocking=blocking)

    def download(self):
        """-> (instances, status words); the borders are checked"""
        torch.cuda.synchronize()
        inst, st = self.d_inst.cpu().numpy(), self.d_status.cpu().numpy()
        assert (inst[112 * self.n:] == 0xAB).all() and (st[16:] == 0xAB).all(), "bytes beyond the extents were written"
        return inst[:112 * self.n].view(ni.INSTANCE_DTYPE).copy(), [int(w) for w in st[:16].view(np.uint32)]

    def assert_equals(self, want, wst, what=""):
        got, gst = self.download()
        bad = np.flatnonzero(got.view(np.uint32).reshape(self.n, 28) != want.view(np.uint32).reshape(self.n, 28))
        assert bad.size == 0, ("instance words differ", what, bad.size, int(bad[0]) // 28, int(bad[0]) % 28)
        assert gst == [int(w) for w in wst], ("status differs", what, gst, list(wst))
        return got


# ---- 0. capturable from the first call on --------------------------------------------------------------------------------------------------
def test_capture_of_the_update_alone_as_the_first_call_on_a_fresh_stream():
    """No allocation, no host table, no earlier uncaptured call: the first call this file makes is a captured one."""
    local, parent, node, blas = uc.hierarchy(65, 3, 5)
    u = _Update(local, parent, 65, node, blas)
    want, wst = iu.update(local, parent, 65, node, blas)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        assert u.run(blocking=False, stream=torch.cuda.current_stream().cuda_stream) is None
    torch.cuda.synchronize()
    for _ in range(2):
        u.d_inst[:112 * 65].fill_(0xCD)
        u.d_status[:16].fill_(0xCD)
        g.replay()
        u.assert_equals(want, wst, "replay")
    # a captured call cannot read a result back
    errs = []
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        u.d_status[:16].fill_(0)      # so that the graph is not empty
        try:
            u.run(blocking=True, stream=torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            errs.append((e.code, str(e)))
        try:
            nt.instances_status_read(u.d_status.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        except nt.NtrError as e:
            errs.append((e.code, str(e)))
    torch.cuda.synchronize()
    assert [c for c, _ in errs] == [-1, -1] and "captured" in errs[0][1] and "captured" in errs[1][1], errs


# ---- 1. bytes == spec -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_update_equals_spec(n):
    tf = isc.seeded_transforms(n, 100 + n, mirrored=min(n, 3))
    blas = (np.arange(n) % 3).astype(np.int32)
    flat = ni.instances(tf, blas)
    u = _Update(tf, None, n, None, blas)
    res = u.run()
    assert (res.numInstances, res.numNodes, res.statusBits, res.firstBad, res.numBad) == (n, n, 0, iu.NO_BAD, 0)
    assert res.updateMs > 0 and res.seconds > 0
    u.assert_equals(flat, CLEAN, (n, "flat"))            # a flat call is np_instanced.instances
    for depth in (1, 2, 3, 16):
        for node_array in (False, True):
            local, parent, node, blas = uc.hierarchy(n, depth, 1000 * depth + n, node_array=node_array)
            want, wst = iu.update(local, parent, n, node, blas)
            assert list(wst) == CLEAN
            u = _Update(local, parent, n, node, blas)
            u.run()
            u.assert_equals(want, wst, (n, depth, node_array))


def test_many_instances_share_one_node():
    local, parent, node, blas = uc.hierarchy(257, 3, 77, share=64)
    assert len(set(node.tolist())) == 5
    want, wst = iu.update(local, parent, 257, node, blas)
    u = _Update(local, parent, 257, node, blas)
    u.run()
    u.assert_equals(want, wst, "shared nodes")


def test_random_affine_matrices_flat_and_chained():
    """Entries across 2^-20 .. 2^20: quotients and products far from one, in which a division that is not correctly rounded would show."""
    tf = uc.random_affine(1000, 31)
    blas = np.zeros(1000, np.int32)
    u = _Update(tf, None, 1000, None, blas)
    u.run()
    u.assert_equals(ni.instances(tf, blas), CLEAN, "flat")
    parent = np.where(np.arange(1000) % 3 == 0, -1, np.arange(1000) - 1).astype(np.int32)     # chains of 1, 2, 3
    want, wst = iu.update(tf, parent, 1000, None, blas)
    u = _Update(tf, parent, 1000, None, blas)
    try:
        u.run()
    except nt.NtrError:
        assert wst[0] != 0
    u.assert_equals(want, wst, "chained")


# ---- 2. errors ------------------------------------------------------------------------------------------------------------------------------
N_ERR = 130
GOOD = {}


def _good():
    if not GOOD:
        local, parent, node, blas = uc.hierarchy(N_ERR, 2, 60)
        GOOD["inst"] = iu.update(local, parent, N_ERR, node, blas)[0]
    return GOOD["inst"]


@pytest.mark.parametrize("case", uc.ERROR_CASES)
def test_error_case_at_the_wave_edges(case):
    bit = iu.CHAIN if case in uc.CHAIN_CASES else iu.SINGULAR
    for at in (0, 63, 64, N_ERR - 1):
        local, parent, node, blas, bits = uc.with_errors(N_ERR, 60, [(case, at)])
        want, wst = iu.update(local, parent, N_ERR, node, blas)
        assert list(wst) == [bit, at, 1, 0] and bits == {at: bit}
        u = _Update(local, parent, N_ERR, node, blas)
        with pytest.raises(nt.NtrError) as e:
            u.run()
        assert e.value.code == -1 and "ntr_instances_update: instance %d " % at in str(e.value), str(e.value)
        res = e.value.result
        assert (res.numInstances, res.numNodes, res.statusBits, res.firstBad, res.numBad) == (N_ERR, local.shape[0], bit, at, 1)
        got = u.assert_equals(want, wst, (case, at))
        others = np.arange(N_ERR) != at
        assert got[others].tobytes() == _good()[others].tobytes(), "a good instance changed"
        assert got["worldToObject"][at].tobytes() == bytes(48) and (bit != iu.CHAIN or got["objectToWorld"][at].tobytes() == bytes(48))
        # the asynchronous form writes the same bytes and the same status
        u.d_inst[:112 * N_ERR].fill_(0xCD)
        assert u.run(blocking=False) is None
        assert nt.instances_status_read(u.d_status.data_ptr()) == [bit, at, 1, 0]
        u.assert_equals(want, wst, (case, at, "asynchronous"))
        # a following clean call resets the status
        node2 = node.copy()
        node2[at] = 0
        u.d_node.copy_(up(node2))
        res = u.run()
        assert res.statusBits == 0 and nt.instances_status_read(u.d_status.data_ptr()) == CLEAN
        u.assert_equals(*iu.update(local, parent, N_ERR, node2, blas), (case, at, "clean"))


def test_several_bad_instances_lowest_index_and_count():
    placed = [("overflow", 66), ("cycle2", 9), ("nan", 64), ("node_eq_num_nodes", 130), ("zero_column", 63), ("chain17", 128), ("inf", 192),
              ("self_parent", 255), ("parent_minus2", 256), ("node_minus1", 257), ("parent_eq_num_nodes", 127)]
    n = 258
    local, parent, node, blas, bits = uc.with_errors(n, 61, placed)
    want, wst = iu.update(local, parent, n, node, blas)
    assert list(wst) == [3, 9, 11, 0]
    u = _Update(local, parent, n, node, blas)
    with pytest.raises(nt.NtrError) as e:
        u.run()
    assert (e.value.result.statusBits, e.value.result.firstBad, e.value.result.numBad) == (3, 9, 11)
    got = u.assert_equals(want, wst, "several")
    assert [i for i in range(n) if got["worldToObject"][i].tobytes() == bytes(48)] == sorted(bits)


# ---- 3. blocking and asynchronous -------------------------------------------------------------------------------------------------------------
def test_blocking_and_asynchronous_forms_agree():
    local, parent, node, blas = uc.hierarchy(257, 3, 12)
    want, wst = iu.update(local, parent, 257, node, blas)
    u = _Update(local, parent, 257, node, blas)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert u.run(blocking=False, stream=st.cuda_stream) is None
        assert nt.instances_status_read(u.d_status.data_ptr(), stream=st.cuda_stream) == CLEAN       # blocks on the stream
    a = u.assert_equals(want, wst, "asynchronous")
    u.d_inst[:112 * 257].fill_(0xCD)
    res = u.run()
    assert (res.numInstances, res.numNodes, res.statusBits, res.firstBad, res.numBad) == (257, local.shape[0], 0, iu.NO_BAD, 0)
    assert u.assert_equals(want, wst, "blocking").tobytes() == a.tobytes()


# ---- 4. one graph: update -> TLAS refit -> trace ---------------------------------------------------------------------------------------------
def test_update_tlas_refit_and_trace_as_one_graph():
    """65 instances of a small soup under 5 group nodes; between replays one device-to-device copy rewrites one group's 48 bytes."""
    n, groups = 65, 5
    p = isc.pool_of(["soup100"])
    d_pool = (up(p["nodes"]), up(p["woop"]), up(p["tri_index"]))
    sizes = (p["nodes"].size, p["woop"].size)
    rng = np.random.default_rng(3)
    group = lambda: isc.transform(isc.rotation(rng), 1.25 ** rng.uniform(-1, 1, 3), rng.uniform(-7, 7, 3))  # noqa: E731
    leaves = [isc.transform(isc.rotation(rng), 0.15 * 2.0 ** rng.uniform(-1, 1, 3), rng.uniform(-4, 4, 3)) for _ in range(n)]
    local = np.stack(leaves + [group() for _ in range(groups)])          # parents after children
    parent = np.concatenate([n + np.arange(n) % groups, np.full(groups, -1)]).astype(np.int32)
    node = rng.permutation(n).astype(np.int32)
    blas = np.zeros(n, np.int32)
    moved = [local.copy() for _ in range(3)]
    for k, m in enumerate(moved):
        m[n + 2] = group() if k < 2 else local[n + 2]                   # (the last replay returns to the start)
    d_moved = [up(m[n + 2]) for m in moved]

    u = _Update(local, parent, n, node, blas)
    s = _Tlas(p["ranges"], d_pool[0], p["nodes"].size, iu.update(local, parent, n, node, blas)[0])
    s.d_inst = u.d_inst                                                  # the refit reads what the update writes
    rays = isc.scene_rays((16, 8), 128)
    assert rays.shape[0] == 256
    d_rays = up(rays)
    st = torch.cuda.Stream()

    def frame(stream):
        u.run(blocking=False, stream=stream)
        s.refit(blocking=False, stream=stream)
        return _trace(s, d_pool, sizes, d_rays, 256, False, stream)

    def check(loc, d_res, d_ids, what):
        want_inst, wst = iu.update(loc, parent, n, node, blas)
        u.assert_equals(want_inst, wst, what)
        want = s.spec(p["nodes"], want_inst)
        s.assert_equals(want, None, what)
        return _assert_trace(d_res, d_ids, 256, want, p, rays, False, what)

    # an uncaptured pass first: the refit uploads its range table and reserves its scratch there
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_res, d_ids = frame(st.cuda_stream)
    hits = int((check(local, d_res, d_ids, "uncaptured") >= 0).sum())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        d_res, d_ids = frame(torch.cuda.current_stream().cuda_stream)
    for k in range(3):
        u.d_local[48 * (n + 2):48 * (n + 3)].copy_(d_moved[k])          # device to device, one group's transform and nothing else
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        u.d_inst[:112 * n].fill_(0xCD)
        torch.cuda.synchronize()
        g.replay()
        hits += int((check(moved[k], d_res, d_ids, "graph replay %d" % k) >= 0).sum())
    assert hits > 0
    assert not np.array_equal(iu.update(moved[0], parent, n, node, blas)[0], iu.update(moved[1], parent, n, node, blas)[0])
