"""ntr_tlas_refit on the device against the numpy rule (tests/np_tlas_refit.py), byte for byte.  The top-level trees are built on the
device by ntr_tlas_build and downloaded: those bytes are the rule's input.  Node, record and scene-box buffers carry 64 bytes of 0xAB
beyond their extents, which must stay.  The shapes are the smallest where the two launches can go wrong: one node, less than a wave, a
wave edge, more child slots than one workgroup, a tree from PLOC rounds plus tail; the refit of a fresh build must change no byte at
any of them, which is what keeps the world box of tlas_refit_kernels.hip and the one of tl_boxes the same statement."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import instanced_scenes as isc
import np_bvh_refit as rf
import np_instanced as ni
import np_tlas_refit as tr
import test_refit_batch_gpu as rbg
from gpu_util import up
from test_tlas_refit_cpu import moved, placed, pool

pytestmark = pytest.mark.gpu

F = np.float32
SLACK = 64
_cache = {}


def _filled(nbytes):
    return torch.full((int(nbytes) + SLACK,), 0xAB, dtype=torch.uint8, device="cuda:0")


class _Tlas:
    """A pool's nodes (a dict as np_instanced.make_pool's, or device tensors with their sizes) and instances on the device, and the
    top-level tree ntr_tlas_build makes of them in 0xAB-bordered buffers.  built_*: the downloaded tree, the rule's input."""

    def __init__(self, ranges, d_pool_nodes, pool_nodes_bytes, inst):
        self.ranges, self.d_pool_nodes, self.pool_nodes_bytes = ranges, d_pool_nodes, pool_nodes_bytes
        self.n = inst.shape[0]
        self.nodes_bytes, self.rec_bytes = 64 * (self.n - 1), 64 * self.n
        self.root = -1 if self.n == 1 else 0
        self.d_inst = up(inst)
        caps = nt.tlas_capacity(self.n)
        d_tlas, d_rec = _filled(caps[0]), _filled(caps[1])
        res = nt.tlas_build(self.n, self.d_inst.data_ptr(), ranges, d_pool_nodes.data_ptr(), pool_nodes_bytes, d_tlas.data_ptr(), caps[0],
                            d_rec.data_ptr(), caps[1])
        torch.cuda.synchronize()
        assert (res.nodesBytes, res.recordsBytes, res.rootLink) == (self.nodes_bytes, self.rec_bytes, self.root)
        # the refit's buffers: exactly the extents, then the border
        self.d_tlas, self.d_rec, self.d_scene = _filled(self.nodes_bytes), _filled(self.rec_bytes), _filled(24)
        self.d_tlas[:self.nodes_bytes] = d_tlas[:self.nodes_bytes]
        self.d_rec[:self.rec_bytes] = d_rec[:self.rec_bytes]
        torch.cuda.synchronize()
        self.built_nodes = self.d_tlas.cpu().numpy()[:self.nodes_bytes].view(np.int32).reshape(-1, 16).copy()
        self.built_records = self.d_rec.cpu().numpy()[:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy()
        self.built_scene = np.concatenate([np.array(list(res.sceneMin), F), np.array(list(res.sceneMax), F)])

    def set_instances(self, inst):
        self.d_inst.copy_(up(inst))

    def set_tree(self, nodes, records):
        self.d_tlas[:self.nodes_bytes] = up(nodes)
        self.d_rec[:self.rec_bytes] = up(records)
        self.d_scene.fill_(0xAB)

    def args(self, scene=True):
        return (self.n, self.d_inst.data_ptr(), self.ranges, self.d_pool_nodes.data_ptr(), self.pool_nodes_bytes, self.d_tlas.data_ptr(),
                self.nodes_bytes, self.root, self.d_rec.data_ptr(), self.rec_bytes, self.d_scene.data_ptr() if scene else 0)

    def refit(self, blocking=True, stream=0, scene=True):
        return nt.tlas_refit(*self.args(scene), stream=stream, blocking=blocking)

    def download(self):
        """-> (nodes int32 (N - 1, 16), records uint32 (N, 16), scene bytes); the borders are checked"""
        torch.cuda.synchronize()
        raw = [b.cpu().numpy() for b in (self.d_tlas, self.d_rec, self.d_scene)]
        for x, e in zip(raw, (self.nodes_bytes, self.rec_bytes, 24)):
            assert (x[e:] == 0xAB).all(), "bytes beyond the extents were written"
        return (raw[0][:self.nodes_bytes].view(np.int32).reshape(-1, 16).copy(), raw[1][:self.rec_bytes].view(np.uint32).reshape(-1, 16).copy(),
                raw[2][:24].copy())

    def spec(self, pool_nodes, inst, nodes=None, records=None):
        return tr.refit(self.built_nodes if nodes is None else nodes, self.root, self.built_records if records is None else records,
                        pool_nodes, self.ranges, inst)

    def assert_equals(self, want, res=None, what="", scene=True):
        nodes, records, sb = self.download()
        bad = np.flatnonzero((nodes != want["nodes"]).any(axis=1))
        assert bad.size == 0, ("nodes differ", what, int(bad[0]), nodes[bad[0]], want["nodes"][bad[0]])
        assert np.array_equal(records, want["records"]), ("records differ", what)
        if scene:
            assert sb.tobytes() == want["scene_box"].tobytes(), ("d_sceneBox differs", what)
        if res is not None:
            assert (res.numNodes, res.numLeaves, res.errBits) == (want["stats"]["numNodes"], want["stats"]["numLeaves"], want["err_bits"]), what
            got = np.concatenate([np.array(list(res.sceneMin), F), np.array(list(res.sceneMax), F)])
            assert got.tobytes() == want["scene_box"].tobytes(), ("sceneMin / sceneMax differ", what)
        return nodes, records


def _three(n, seed=None):
    """pool() on the device and placed(n) instances with their device-built tree"""
    p = pool()
    if "dev" not in _cache:
        _cache["dev"] = (up(p["nodes"]), up(p["woop"]), up(p["tri_index"]))
    inst = placed(n, 500 + n if seed is None else seed)
    return inst, _Tlas(p["ranges"], _cache["dev"][0], p["nodes"].size, inst)


def _refitted(n):
    """(_Tlas, moved instances, spec) after (a) the refit with unchanged instances and (b) the blocking refit to moved instances"""
    p = pool()
    inst, s = _three(n)
    before = [b.clone() for b in (s.d_tlas, s.d_rec)]
    res = s.refit()
    torch.cuda.synchronize()
    assert torch.equal(before[0], s.d_tlas) and torch.equal(before[1], s.d_rec), ("the refit of a fresh build changed a byte", n)
    assert res.errBits == 0 and (res.numNodes, res.numLeaves) == (n - 1, n) and res.seconds > 0
    assert s.download()[2].tobytes() == s.built_scene.tobytes(), n
    assert np.concatenate([np.array(list(res.sceneMin), F), np.array(list(res.sceneMax), F)]).tobytes() == s.built_scene.tobytes()
    new = moved(inst, 900 + n)
    s.set_instances(new)
    s.d_scene.fill_(0xAB)
    res = s.refit()
    want = s.spec(p["nodes"], new)
    s.assert_equals(want, res, n)
    assert want["err_bits"] == 0 and res.seconds > 0
    assert np.array_equal(_cache["dev"][0].cpu().numpy(), p["nodes"]), "the pool's bytes changed"
    return s, new, want, res


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, nt.PLOC_TAIL + 1])
def test_refit_equals_spec(n):
    s, new, want, res = _refitted(n)
    print("N=%d: %.1f us" % (n, res.seconds * 1e6))
    # without a scene box pointer the blocking form reports the same box and writes none
    s.d_scene.fill_(0xAB)
    res2 = s.refit(scene=False)
    assert s.download()[2].tobytes() == bytes([0xAB]) * 24
    s.assert_equals(want, res2, (n, "no scene pointer"), scene=False)


# ---- 2. trace ---------------------------------------------------------------------------------------------------------------------------
def _trace(s, d_pool, pool_sizes, d_rays, num_rays, any_hit, stream=0):
    d_res, d_ids = _filled(16 * num_rays), _filled(4 * num_rays)
    nt.trace_instanced(num_rays, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), s.d_tlas.data_ptr(), s.nodes_bytes, s.root,
                       s.d_rec.data_ptr(), s.n, d_pool[0].data_ptr(), pool_sizes[0], d_pool[1].data_ptr(), pool_sizes[1], d_pool[2].data_ptr(),
                       stream=stream, timed=False)
    return d_res, d_ids


def _assert_trace(d_res, d_ids, num_rays, want_tlas, spool, rays, any_hit, what):
    torch.cuda.synchronize()
    assert nt.trace_status() == 0
    res, ids = d_res.cpu().numpy(), d_ids.cpu().numpy()
    assert (res[16 * num_rays:] == 0xAB).all() and (ids[4 * num_rays:] == 0xAB).all()
    gid, gt, gu, gv = isc.result_words(res[:16 * num_rays].view(nt.RESULT_DTYPE))
    rid, rt, ru, rv, rinst = ni.trace(want_tlas["nodes"], -1 if want_tlas["records"].shape[0] == 1 else 0, want_tlas["records"], spool, rays, any_hit)
    for name, g, e in (("id", gid, rid), ("t", gt, rt.view(np.uint32)), ("u", gu, ru.view(np.uint32)), ("v", gv, rv.view(np.uint32)),
                       ("instance", ids[:4 * num_rays].view(np.int32), rinst)):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, "%s anyHit=%d: %d %s mismatches of %d rays, first at ray %d" % (what, any_hit, bad.size, name, num_rays, bad[0])
    return rid


@pytest.mark.parametrize("n", [65, nt.PLOC_TAIL + 1])
def test_trace_over_the_refitted_buffers_equals_the_spec(n):
    s, new, want, _ = _refitted(n)
    p = pool()
    rays = isc.scene_rays((64, 32), 2048)
    d_rays = up(rays)
    hits = 0
    for any_hit in (False, True):
        d_res, d_ids = _trace(s, _cache["dev"], (p["nodes"].size, p["woop"].size), d_rays, rays.shape[0], any_hit)
        hits += int((_assert_trace(d_res, d_ids, rays.shape[0], want, p, rays, any_hit, n) >= 0).sum())
    assert hits > rays.shape[0] // 8


# ---- 3. after a BLAS refit, and 4. one graph -----------------------------------------------------------------------------------------------
def _deforming():
    """A ntr_ploc_build_batch pool of five small meshes, seven instances of them, and their tree"""
    bp = rbg._Pool(ploc=rbg._soups((1, 2, 40, 300, 1200), 21))
    ranges = [e[0] for e in bp.entries]

    def instances(seed):
        rng = np.random.default_rng(seed)
        blas = np.array([0, 1, 2, 3, 4, 3, 4])
        rng.shuffle(blas)
        tf = [isc.transform(isc.rotation(rng), 0.15 * 2.0 ** rng.uniform(-1, 1, 3) * (-1 if i == 2 else 1), rng.uniform(-8, 8, 3)) for i in range(7)]
        return ni.instances(np.stack(tf), blas.astype(np.int32))

    inst = instances(1)
    return bp, ranges, instances, inst, _Tlas(ranges, bp.bufs[0], bp.caps[0], inst)


def _spool(bp, sp):
    return dict(nodes=sp["nodes"], woop=sp["woop"], tri_index=bp.host[2][:bp.caps[2]].view(np.int32), ranges=[e[0] for e in bp.entries])


def test_asynchronous_blas_refit_then_tlas_refit_on_one_stream():
    bp, ranges, instances, inst, s = _deforming()
    p = rf.moved(bp.pos, 0.3)
    d_pos = up(p)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert nt.bvh_refit_batch(*bp.args(bp.bufs, bp.entries, d_pos, None), stream=st.cuda_stream, blocking=False) is None
        assert s.refit(blocking=False, stream=st.cuda_stream) is None
    torch.cuda.synchronize()
    sp = bp.assert_pool(bp.entries, p, d_pos, None, "deforming", loop=False)
    want = s.spec(sp["nodes"], inst)
    s.assert_equals(want, None, "after the BLAS refit")
    assert want["nodes"].tobytes() != s.built_nodes.tobytes()      # the root boxes of the BLASes did move


def test_blas_refit_tlas_refit_and_trace_as_one_graph():
    bp, ranges, instances, inst, s = _deforming()
    rays = isc.scene_rays((32, 16), 512)
    d_rays = up(rays)
    sizes = (bp.caps[0], bp.caps[1])
    uploads = [(rf.moved(bp.pos, how), instances(seed)) for how, seed in ((0.02, 2), (0.3, 3), (0.1, 4))]
    d_pos = up(uploads[0][0])
    st = torch.cuda.Stream()

    def frame(stream):
        nt.bvh_refit_batch(*bp.args(bp.bufs, bp.entries, d_pos, None), stream=stream, blocking=False)
        s.refit(blocking=False, stream=stream)
        return _trace(s, bp.bufs, sizes, d_rays, rays.shape[0], False, stream)

    def check(k, d_res, d_ids, what):
        pk, ik = uploads[k]
        sp = bp.assert_pool(bp.entries, pk, d_pos, None, what, loop=False)
        want = s.spec(sp["nodes"], ik)
        s.assert_equals(want, None, what)
        return _assert_trace(d_res, d_ids, rays.shape[0], want, _spool(bp, sp), rays, False, what)

    # an identical uncaptured pass first: it uploads the two tables and reserves the scratch
    s.set_instances(uploads[0][1])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_res, d_ids = frame(st.cuda_stream)
    hits = int((check(0, d_res, d_ids, "uncaptured") >= 0).sum())
    held = nt.tlas_refit_scratch_bytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        d_res, d_ids = frame(torch.cuda.current_stream().cuda_stream)
    assert nt.tlas_refit_scratch_bytes() == held
    for rep, k in enumerate((1, 2, 0)):
        d_pos.copy_(up(uploads[k][0]))
        s.set_instances(uploads[k][1])
        bp.reset()
        d_res.fill_(0xAB)
        d_ids.fill_(0xAB)
        s.d_scene.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        hits += int((check(k, d_res, d_ids, "graph replay %d" % rep) >= 0).sum())
    assert hits > 0
    del g
    # refused captures: other ranges, a result pointer, after the workspace was released; the library works afterwards
    errs = []

    def capture(ranges2, blocking=False):
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=st):
            cs = torch.cuda.current_stream().cuda_stream
            s.d_scene.fill_(0xAB)    # so that the graph is not empty
            try:
                args = list(s.args())
                args[2] = ranges2
                nt.tlas_refit(*args, stream=cs, blocking=blocking)
            except nt.NtrError as e:
                errs.append((e.code, str(e)))
        torch.cuda.synchronize()

    other = [ranges[k] for k in (1, 0, 2, 3, 4)]
    capture(other)
    capture(ranges, blocking=True)
    nt.lbvh_release_workspace()
    assert nt.tlas_refit_scratch_bytes() == 0
    capture(ranges)
    assert [c for c, _ in errs] == [-1, -1, -1] and "uncaptured call" in errs[0][1] and "uncaptured call" in errs[2][1], errs
    assert all("ntr_tlas_refit" in m for _, m in errs)
    res = s.refit()
    pk, ik = uploads[0]
    s.assert_equals(s.spec(bp.spec(bp.entries, pk)["nodes"], ik), res, "after the refused captures")


# ---- 5. malformed input is never followed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [("blas",), ("link",), ("leaf",), ("blas", "link", "leaf")])
def test_a_bad_part_is_never_followed(which):
    """An uploaded tree of 5 instances with a link that names no slot (64 * 9), a leaf link beyond the instances (~7) and an instance
    whose blas index is numBlas, one at a time and all three: error code and bits, and every byte -- the bad words, the boxes of their
    ancestors, the bad instance's record, the borders -- is the rule's (np_tlas_refit rule 7: a box is rewritten exactly where
    everything below it is well formed)."""
    p = pool()
    inst, s = _three(5, seed=77)
    new = moved(inst, 78)
    nodes = s.built_nodes.copy()
    leaves = [(a, k) for a in range(4) for k in (0, 1) if nodes[a, 12 + k] < 0]
    if "link" in which:
        a, k = leaves[0]
        nodes[a, 12 + k] = 64 * 9
    if "leaf" in which:
        a, k = leaves[2]
        nodes[a, 12 + k] = ~7
    bad_i = -1
    if "blas" in which:
        a, k = leaves[4]
        bad_i = ~int(nodes[a, 12 + k])
        new["blas"][bad_i] = 3
    s.set_tree(nodes, s.built_records)
    s.set_instances(new)
    want = s.spec(p["nodes"], new, nodes=nodes)
    bits = sum(b for name, b in (("blas", 1), ("link", 2), ("leaf", 4)) if name in which)
    assert want["err_bits"] == bits
    with pytest.raises(nt.NtrError) as e:
        s.refit()
    assert e.value.code == (-1 if "blas" in which else -4) and "ntr_tlas_refit" in str(e.value), str(e.value)
    assert ("blas index" in str(e.value)) == ("blas" in which)
    res = e.value.result
    got_nodes, got_records = s.assert_equals(want, res, which, scene=False)
    assert res.errBits == bits and not any(res.sceneMin) and not any(res.sceneMax)
    assert s.download()[2].tobytes() == bytes([0xAB]) * 24          # the root was not refitted: d_sceneBox keeps its bytes
    assert np.array_equal(got_nodes[:, 12:], nodes[:, 12:])
    if bad_i >= 0:
        assert np.array_equal(got_records[bad_i], s.built_records[bad_i])
    # something was refitted all the same: the spec is neither the input nor the clean refit
    assert want["nodes"].tobytes() != nodes.tobytes() or len(which) == 3
    # the asynchronous form skips the bad part silently and writes the same bytes
    s.set_tree(nodes, s.built_records)
    assert s.refit(blocking=False) is None
    s.assert_equals(want, None, (which, "asynchronous"), scene=False)
    assert s.download()[2].tobytes() == bytes([0xAB]) * 24
    assert nt.trace_status() == 0


# ---- 6. determinism, scratch and release --------------------------------------------------------------------------------------------------
def test_determinism_scratch_and_release():
    nt.lbvh_release_workspace()
    assert nt.tlas_refit_scratch_bytes() == 0
    inst, s = _three(700)
    new = moved(inst, 5)
    s.set_instances(new)
    s.refit()
    a = s.download()
    held = nt.tlas_refit_scratch_bytes()
    assert held >= 8 * 699 + 16 * 3
    s.set_tree(s.built_nodes, s.built_records)
    s.refit()
    b = s.download()
    assert nt.tlas_refit_scratch_bytes() == held
    nt.lbvh_release_workspace()
    assert nt.tlas_refit_scratch_bytes() == 0
    s.set_tree(s.built_nodes, s.built_records)
    assert s.refit(blocking=False) is None
    c = s.download()
    assert nt.tlas_refit_scratch_bytes() == held
    for other in (b, c):
        for x, y in zip(a, other):
            assert x.tobytes() == y.tobytes()
    assert nt.trace_status() == 0
    print("scratch: %d B for 699 slots and 3 BLASes" % held)
    nt.lbvh_release_workspace()
    assert nt.tlas_refit_scratch_bytes() == 0
