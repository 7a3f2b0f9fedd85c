"""Every row of the trace-tunable sweep (tests/trace_sweep.py) on the GPU: whatever the tunables say, every record ntr_trace_bvh writes
equals the CPU oracle's bit for bit -- id exactly, t by its 32 bits; no tolerance anywhere --, the status word stays zero and nothing is
written past the records.

* pairwise rows (every value of every tunable beside every value of every other one): all four kernel names, closest hit and any hit, on
  a one-triangle-leaf SAH tree and a device-built LBVH tree with wide leaves, a mixed batch of ragged size and its first 1 000 rays; rows
  that change a loop parameter also trace the comb tree of test_unified_loop_gpu.py, whose stack crosses the LDS boundary;
* shape rows (one per launch shape plan_trace can return): the kernel name, hit mode and batch size the shape belongs to, on the SAH
  tree -- a camera batch the device calls coherent and a scattered one it calls incoherent, so that both sides of a routed launch trace.

Every case launches its batch through the same buffers REPEATS times after one launch with bvhFlags = 0: the automatic hint first runs
the predicted order and measures, then orders by what it measured and measures again, and the last launch runs a learned order without
measuring.  The sizes and thresholds are small; what is swept is the code path, not the scale."""
import numpy as np
import pytest

import ntrace_amd as nt
import trace_sweep as ts
from ntrace_amd import scenes
from oracle import oracle

pytestmark = pytest.mark.gpu

REPEATS = 4
GUARD = 64
CAMERA_N, SCATTERED_N, SMALL_N = 12288 - 27, 8229, 1000
SHORT = {"fermi_speculative_while_while": "fermi", "tesla_persistent_while_while": "tesla",
         "tesla_persistent_speculative_while_while": "tesla_spec", "kepler_dynamic_fetch": "kepler"}

PAIRWISE = ts.pairwise_rows()
SHAPES = ts.shape_rows((CAMERA_N, SCATTERED_N, SMALL_N))


@pytest.fixture(autouse=True)
def default_tunables(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("NTR_"):
            monkeypatch.delenv(k, raising=False)
    nt.set_tunables()
    yield
    ts.clear()
    nt.set_tunables()


class Tree:
    def __init__(self, name, host):
        from gpu_util import DeviceBvh
        self.name, self.host, self.dev = name, host, DeviceBvh(host)
        self.flags = self.dev.flags

    def revalidate(self):
        """ntr_bvh_validate rebuilds the BVH's top-of-tree table: with the NTR_TRACE_PREDICT_DEPTH in force now."""
        assert self.dev.view.validate() == self.flags


class Batch:
    def __init__(self, name, rays):
        from gpu_util import up
        import torch
        self.name, self.rays, self.n = name, rays, rays.shape[0]
        self.d_rays = up(rays)
        self.d_res = torch.empty(self.n * 16 + GUARD, dtype=torch.uint8, device="cuda:0")
        self.refs = {}     # (tree name, any hit) -> (records, counters) of the oracle


@pytest.fixture(scope="module")
def world():
    """The trees, the batches and the oracle's records, each made once."""
    import torch
    from gpu_util import up
    from test_unified_loop_gpu import comb_rays, comb_tree
    tri, pos, cam = scenes.random_soup(3000, seed=31, walls=True)
    sah = Tree("sah", nt.sah_build(tri, pos, 1, 1))
    assert not (sah.flags & nt.BVH_WIDE_LEAVES)
    n = tri.shape[0]
    capn, capw, capi = nt.lbvh_capacity(n)
    d_tri, d_pos = up(tri), up(pos)
    bufs = [torch.zeros(c, dtype=torch.uint8, device="cuda:0") for c in (capn, capw, capi)]
    mn, mx = oracle.scene_bbox(pos)
    res = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw,
                        bufs[2].data_ptr(), capi)
    torch.cuda.synchronize()
    lbvh = Tree("lbvh", nt.HostBvh(bufs[0].cpu().numpy()[:res.nodesBytes].copy(), bufs[1].cpu().numpy()[:res.triWoopBytes].copy(),
                                   bufs[2].cpu().numpy()[:res.triIndexBytes].view(np.int32).copy()))
    assert lbvh.flags & nt.BVH_WIDE_LEAVES
    for t in (sah, lbvh):      # above the lowered prediction threshold, below the wide pool's and the stand-in the shapes were computed for
        assert 64 * ts.FIXED["NTR_TRACE_PREDICT_MIN_NODES"] <= t.host.nodes.nbytes < 32 << 20
    combs = [Tree("comb%d" % flip, comb_tree(flip)) for flip in (0, 1)]

    camera, scattered, mixed = sweep_batches(cam, pos)
    batches = {"camera": Batch("camera", camera), "scattered": Batch("scattered", scattered), "mixed": Batch("mixed", mixed),
               "small": Batch("small", mixed[:SMALL_N])}
    assert (batches["camera"].n, batches["scattered"].n, batches["small"].n) == (CAMERA_N, SCATTERED_N, SMALL_N)
    assert mixed.shape[0] % 64 == 37 and mixed.shape[0] % 256 != 0 and mixed.shape[0] <= 21000
    for flip in (0, 1):        # the comb's own batch, seven times over (enough rays for the automatic hint) and ragged
        batches["comb%d" % flip] = Batch("comb%d" % flip, np.tile(comb_rays(17 + flip), 7)[:-13])
    for b in batches.values():
        trees = [t for t in combs if t.name == b.name] if b.name.startswith("comb") else [sah] + ([lbvh] if b.name in ("mixed", "small") else [])
        for t in trees:
            for any_hit in (False, True):
                b.refs[t.name, any_hit] = oracle.trace(t.host.nodes, t.host.woop, t.host.tri_index, b.rays, any_hit=any_hit, threads=8)
    for (t, ah), (ref, _) in batches["mixed"].refs.items():
        hits = int((ref["id"] >= 0).sum())
        assert 0 < hits < ref.shape[0], "the mixed batch must hit and miss"
    return dict(sah=sah, lbvh=lbvh, comb0=combs[0], comb1=combs[1]), batches


def sweep_batches(cam, pos):
    """camera: one pinhole's rays in pixel-table order; scattered: origins all over the scene's box; mixed: both, the edge-case rays and 300
    short occlusion-like rays -- its first 1 000 rays hold some of each --, cut (in its camera part) to a count that is 37 mod 64."""
    from ray_sets import edge_rays
    camera = scenes.primary_rays(cam, 128, 96)[0][:CAMERA_N]
    scattered = scenes.box_rays(pos, SCATTERED_N, seed=5)
    edge, ao = edge_rays(), scenes.random_rays(300, seed=9, tmax=3.0)
    head = (448, 256, 200, 96)
    parts = (camera, scattered, edge, ao)
    total = sum(p.shape[0] for p in parts)
    target = (21000 - 37) // 64 * 64 + 37
    keep_camera = camera.shape[0] - (total - target)
    mixed = np.concatenate([p[:h] for p, h in zip(parts, head)] + [camera[head[0]:keep_camera]] + [p[h:] for p, h in zip(parts[1:], head[1:])])
    assert mixed.shape[0] == target and sum(head) == SMALL_N
    return camera, scattered, mixed


def check_launches(tree, batch, kernel, any_hit, what):
    """One launch with bvhFlags = 0 and REPEATS with the validated flags, each on a fresh 0xAB prefill: status word zero, guard untouched,
    records equal to the oracle's."""
    import torch
    from gpu_util import assert_parity
    stream = torch.cuda.current_stream().cuda_stream
    ref = batch.refs[tree.name, bool(any_hit)][0]
    for i, flags in enumerate([0] + [None] * REPEATS):
        if i < 2:
            nt.stream_release(stream)      # a fresh automatic hint: the first launch of a batch, whatever was traced before
        batch.d_res.fill_(0xAB)
        tree.dev.view.trace(kernel, batch.n, any_hit, batch.d_rays.data_ptr(), batch.d_res.data_ptr(), stream, False, flags)
        where = "%s: %s anyHit=%d %s/%s launch %d flags=%s" % (what, kernel, any_hit, tree.name, batch.name, i, flags)
        assert nt.trace_status(stream) == 0, where
        raw = batch.d_res.cpu().numpy()
        assert (raw[batch.n * 16:] == 0xAB).all(), where + ": bytes past the records were written"
        got = raw[:batch.n * 16].view(nt.RESULT_DTYPE)
        if not (np.array_equal(got["id"], ref["id"]) and np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))):
            assert_parity(got, ref, where)


def test_the_device_calls_the_camera_batch_coherent_and_the_scattered_one_incoherent(world):
    """A condition on the batches, not a measurement: under the sweep's thresholds a routed closest-hit launch (coherentRoute 1) of the camera
    batch is traced by its per-ray side and one of the scattered batch by its persistent side.  tests/np_sched.py says the same beforehand."""
    import torch
    import np_sched
    trees, batches = world
    sah = trees["sah"]
    ts.apply(ts.DEFAULTS)
    sah.revalidate()
    out = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
    table = np_sched.top_table(sah.host.nodes, sah.host.nodes.nbytes, ts.DEFAULTS["NTR_TRACE_PREDICT_DEPTH"])
    for name, coherent in (("camera", True), ("scattered", False)):
        b = batches[name]
        nt.predict_batch_coherence(b.n, b.d_rays.data_ptr(), sah.dev.nodes.data_ptr(), sah.host.nodes.nbytes, out.data_ptr())
        torch.cuda.synchronize()
        words = out.cpu().tolist()
        assert words == np_sched.coherence_words(b.rays, table, (b.n + 255) // 256, 2), name
        k, divergent = words[2] & 0xFFFF, words[2] >> 16
        assert (k == 1 and not divergent) if coherent else k > 1, (name, words)
        assert nt.trace_plan("kepler_dynamic_fetch", b.n, False, sah.host.nodes.nbytes, sah.host.woop.nbytes).coherentRoute == 1


@pytest.mark.parametrize("row", range(len(PAIRWISE)), ids=["pair%02d:%s" % (i, ts.row_id(r)) for i, r in enumerate(PAIRWISE)])
def test_pairwise_row_changes_no_record(world, row):
    trees, batches = world
    config = PAIRWISE[row]
    what = "row %d (%s)" % (row, ts.row_id(config))
    ts.apply(config)
    loop_row = any(config[n] != ts.DEFAULTS[n] for n in ts.LOOP_FACTORS)
    cases = [(trees[t], batches[b]) for t in ("sah", "lbvh") for b in ("mixed", "small")]
    if loop_row:
        cases += [(trees[c], batches[c]) for c in ("comb0", "comb1")]
    for tree in {id(t): t for t, _ in cases}.values():
        tree.revalidate()
    nt.trace_status()
    for tree, batch in cases:
        for kernel in nt.KERNELS:
            for any_hit in (False, True):
                check_launches(tree, batch, kernel, any_hit, what)
    if row == 0:      # the defaults: the instrumented kernel's counters equal the oracle's as well
        assert not ts.non_default(config)
        for tree, batch in cases:
            for any_hit in (False, True):
                ref = batch.refs[tree.name, any_hit][0]
                # (the counters are defined over the rays with tmin < tmax: the kernels answer the others without traversal)
                live = batch.rays[batch.rays["tmin"] < batch.rays["tmax"]]
                assert 0 < live.shape[0] < batch.n
                rst = oracle.trace(tree.host.nodes, tree.host.woop, tree.host.tri_index, live, any_hit=any_hit, threads=8)[1]
                want = dict({k: v for k, v in rst.as_dict().items() if k != "maxStackDepth"}, numRays=batch.n)
                batch.d_res.fill_(0xAB)
                st = tree.dev.view.trace_stats("kepler_dynamic_fetch", batch.n, any_hit, batch.d_rays.data_ptr(), batch.d_res.data_ptr())
                assert st.as_dict() == want, (tree.name, batch.name, any_hit)
                raw = batch.d_res.cpu().numpy()
                assert (raw[batch.n * 16:] == 0xAB).all() and np.array_equal(raw[:batch.n * 16].view(nt.RESULT_DTYPE)["id"], ref["id"])


def shape_id(i):
    (kernel, any_hit, n), config = SHAPES[i][0][:3], SHAPES[i][1]
    return "shape%03d:%s,anyHit=%d,n=%d:%s" % (i, SHORT[kernel], any_hit, n, ts.row_id(config))


@pytest.mark.parametrize("row", range(len(SHAPES)), ids=[shape_id(i) for i in range(len(SHAPES))])
def test_launch_shape_changes_no_record(world, row):
    import torch
    trees, batches = world
    key, config = SHAPES[row]
    kernel, any_hit, n = key[:3]
    sah = trees["sah"]
    batch = batches[{CAMERA_N: "camera", SCATTERED_N: "scattered", SMALL_N: "small"}[n]]
    assert batch.n == n
    ts.apply(config)
    # the launch of this batch on this device has the shape the row stands for
    plan = nt.trace_plan(kernel, n, any_hit, sah.host.nodes.nbytes, sah.host.woop.nbytes, nodes_addr=sah.dev.nodes.data_ptr(),
                         woop_addr=sah.dev.woop.data_ptr(), bvh_flags=sah.flags, num_cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert ts.shape_key(kernel, any_hit, n, plan) == key
    nt.trace_status()
    check_launches(sah, batch, kernel, any_hit, shape_id(row))


def test_a_sweep_leaves_no_state_behind(world):
    """After the last row: tunables back to the defaults, everything captured launches or the stream hold returned, and a default launch
    still equals the oracle."""
    import torch
    trees, batches = world
    ts.clear()
    nt.set_tunables()
    nt.trace_graph_release_all()
    nt.stream_release(torch.cuda.current_stream().cuda_stream)
    for t in (trees["sah"], trees["lbvh"]):
        t.revalidate()
    base = nt.trace_plan("kepler_dynamic_fetch", batches["mixed"].n, False, 64 * 3000, 64 * 3000)
    assert not base.predictable and not base.useAutoHint and base.coherentRoute == 0      # (the library's own thresholds again)
    for kernel in nt.KERNELS:
        for any_hit in (False, True):
            check_launches(trees["lbvh"], batches["mixed"], kernel, any_hit, "after the sweep")
            check_launches(trees["sah"], batches["small"], kernel, any_hit, "after the sweep")
