"""The scheduling layer against its exact numpy restatements (np_sched.py): per-block costs (ntr_predict_block_costs), the dispatch
order and batch word of the prediction (ntr_predict_dispatch_order), the coherence words (ntr_predict_batch_coherence), the order a
predicted hint gets (ntr_sched_hint_predict) and the life of a hint over real launches (ntr_sched_hint_inspect after every launch).
Records alone cannot see this layer: any permutation of the blocks gives the same records."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt
import np_sched as S
from gpu_util import DeviceBvh, assert_parity, up
from kat_vectors import two_leaf_bvh
from ntrace_amd import scenes
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = [1, 99, 100, 101, 227, 228, 255, 256, 257, 256 * 63 + 1, 256 * 64, 256 * 64 + 1, 70001]


def device_lbvh(tri, pos):
    n = tri.shape[0]
    capn, capw, capi = nt.lbvh_capacity(n)
    d_tri, d_pos = up(tri), up(pos)
    bufs = [torch.zeros(c, dtype=torch.uint8, device=DEV) for c in (capn, capw, capi)]
    mn, mx = oracle.scene_bbox(pos)
    res = nt.lbvh_build(n, d_tri.data_ptr(), pos.shape[0], d_pos.data_ptr(), mn, mx, 8, 0.001, bufs[0].data_ptr(), capn, bufs[1].data_ptr(), capw,
                        bufs[2].data_ptr(), capi)
    torch.cuda.synchronize()
    return nt.HostBvh(bufs[0].cpu().numpy()[:res.nodesBytes].copy(), bufs[1].cpu().numpy()[:res.triWoopBytes].copy(),
                      bufs[2].cpu().numpy()[:res.triIndexBytes].view(np.int32).copy())


@pytest.fixture(scope="module")
def soup():
    tri, pos, cam = scenes.random_soup(20000, seed=11)
    return DeviceBvh(nt.sah_build(tri, pos)), tri, pos, cam


@pytest.fixture(scope="module")
def trees(soup):
    out = {"sah soup": soup[0]}
    tri, pos, _ = scenes.atrium()
    out["atrium, leaves of 1"] = DeviceBvh(nt.sah_build(tri, pos, 1, 1))
    t2, p2 = scenes.random_soup(30000, seed=53)[:2]
    out["device lbvh"] = DeviceBvh(device_lbvh(t2, p2))
    two_t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    two_p = np.array([[-5, -5, 0], [-4, -5, 0], [-5, -4, 0], [4, 4, 1], [5, 4, 1], [4, 5, 1]], np.float32)
    out["two triangles"] = DeviceBvh(nt.sah_build(two_t, two_p, 1, 1))
    kn, kw, ki = two_leaf_bvh((-2, -1, -1, 1, -1, 1), (1, 2, -1, 1, -1, 1), [(0, 0, 0, 0)] * 3, [(0, 0, 0, 0)] * 3, 0, 1)
    out["kat two leaves"] = DeviceBvh(nt.HostBvh(kn, kw, ki))
    return out


def special_rays(cam):
    """Rays with +-0 direction components, zero-length directions, tmin >= tmax, NaN components, tmax = inf, subnormal components."""
    r = []
    nan, inf, sub = float("nan"), float("inf"), 1e-41
    for o in ((1.0, 2.0, -14.0), (0.0, 0.0, 0.0), (-0.0, 3.0, 0.5)):
        for d in ((0.0, 0.0, 1.0), (-0.0, 0.0, 1.0), (0.0, -0.0, -1.0), (0.3, -0.0, 0.4), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0),
                  (nan, 0.5, 0.5), (0.5, nan, 0.1), (sub, 1.0, -sub), (-sub, sub, 1.0), (1e-30, 1.0, 1e-38), (0.2, 0.3, 0.9)):
            for t0, t1 in ((0.0, 1e30), (0.0, inf), (3.0, 3.0), (5.0, 4.0), (0.0, nan), (nan, 10.0), (-inf, inf), (0.0, 2.0)):
                r.append(o + (t0,) + d + (t1,))
    r.append((nan, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1e30))
    r.append((inf, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 1e30))
    return np.array(r, np.float32).view(nt.RAY_DTYPE).reshape(-1)


def ao_rays(pos, n, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, nt.RAY_DTYPE)
    p = pos[rng.integers(0, pos.shape[0], n)]
    d = rng.standard_normal((n, 3)).astype(np.float32)
    for k, v in zip(("ox", "oy", "oz", "dx", "dy", "dz"), (p[:, 0], p[:, 1], p[:, 2], d[:, 0], d[:, 1], d[:, 2])):
        rays[k] = v
    rays["tmin"], rays["tmax"] = 1e-3, 0.5
    return rays


def mixed_batch(cam, pos, n_total=70001, seed=5):
    """Primary, random and AO rays, with the special rays placed where the kernels look: the sample lanes 100 (and 227) of the blocks
    and the last ray of every count in COUNTS (the sample of a short last block)."""
    prim = scenes.primary_rays(cam, 320, 240)[0]
    pool = np.concatenate([prim, scenes.random_rays(40000, seed=seed), ao_rays(pos, 20000, seed)])
    rng = np.random.default_rng(seed)
    rays = pool[rng.integers(0, pool.shape[0], n_total)]
    m = min(prim.shape[0] // 2, n_total)
    rays[:m] = prim[:m]                                        # a run of camera rays (coherent blocks)
    sp = special_rays(cam)
    nb = (n_total + 255) // 256
    pick = np.arange(0, nb, 2)                                 # every other block's sample ray is special
    rays[np.minimum(pick * 256 + 100, n_total - 1)] = sp[np.arange(pick.size) % sp.size]
    for k, n in enumerate(COUNTS):
        if n <= n_total:
            rays[n - 1] = sp[(7 * k + 3) % sp.size]
    return rays


def device_costs(dbvh, d_rays, n):
    out = torch.full(((n + 255) // 256,), 0x7777, dtype=torch.int32, device=DEV)
    nt.predict_block_costs(n, d_rays.data_ptr(), dbvh.nodes.data_ptr(), dbvh.host.nodes.nbytes, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def set_depth(monkeypatch, trees, depth):
    monkeypatch.setenv("NTR_TRACE_PREDICT_DEPTH", str(depth))
    nt.set_tunables()
    for d in trees.values():
        d.view.validate()          # the cached top-of-tree table is rebuilt here only


def first_mismatch(got, want):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (int(bad.size), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


# ---- A: block costs ---------------------------------------------------------------------------------------------------------------------
def test_block_costs_equal_the_restatement_bit_for_bit(soup, trees, monkeypatch):
    _, _, pos, cam = soup
    rays = mixed_batch(cam, pos)
    d_rays = up(rays)
    try:
        for depth in (0, 1, 9, 10, 11):
            set_depth(monkeypatch, trees, depth)
            for name, dbvh in trees.items():
                table = S.top_table(dbvh.host.nodes, dbvh.host.nodes.nbytes, depth)
                if name in ("two triangles", "kat two leaves"):
                    assert table.shape[0] == 2
                counts = COUNTS if depth == 9 else [70001, 257, 1]
                for n in counts:
                    want = S.block_costs(rays[:n], table)
                    got = device_costs(dbvh, d_rays, n)
                    assert first_mismatch(got, want) is None, (name, depth, n, first_mismatch(got, want))
                    if n == 70001 and name != "kat two leaves":
                        assert want.max() > 0, (name, depth)
    finally:
        monkeypatch.delenv("NTR_TRACE_PREDICT_DEPTH")
        nt.set_tunables()
        for d in trees.values():
            d.view.validate()


# ---- B: the dispatch order of the prediction -------------------------------------------------------------------------------------------
def dispatch_order(dbvh, d_rays, n):
    order = torch.full(((n + 255) // 256,), -1, dtype=torch.int32, device=DEV)
    word = torch.full((1,), 0x5A5A, dtype=torch.int32, device=DEV)
    nt.predict_dispatch_order(n, d_rays.data_ptr(), dbvh.nodes.data_ptr(), dbvh.host.nodes.nbytes, order.data_ptr(), word.data_ptr())
    return order.cpu().numpy().view(np.uint32).astype(np.int64), int(word.cpu().numpy().view(np.uint32)[0])


def pool_k_wide(nodes_bytes, n):
    return nt.trace_plan("fermi_speculative_while_while", n, False, nodes_bytes, 1 << 20).minipoolWide


@pytest.mark.parametrize("blocks", [63, 64, 65, 1023, 1024, 1025, 8193])
def test_dispatch_order_and_word_equal_the_restatement(soup, blocks):
    dbvh, _, pos, cam = soup
    table = S.top_table(dbvh.host.nodes, dbvh.host.nodes.nbytes, 9)
    n = blocks * 256 - 37
    rays = mixed_batch(cam, pos, n, seed=blocks) if n <= 400000 else np.concatenate(
        [scenes.random_rays(n // 2, seed=blocks), np.resize(scenes.primary_rays(cam, 320, 240)[0], n - n // 2)])
    d_rays = up(rays)
    cls = S.dispatch_class(S.block_costs(rays, table))
    want_word = S.coherence_words(rays, table, blocks, pool_k_wide(dbvh.host.nodes.nbytes, n))[2]
    words = []
    for rep in range(2):       # twice through the same scratch: its class counters are zero again after each prediction
        order, word = dispatch_order(dbvh, d_rays, n)
        assert S.check_flatten_order(order, cls) is None, (blocks, rep, S.check_flatten_order(order, cls))
        assert word == want_word, (blocks, rep, hex(word), hex(want_word))
        words.append(word)
    assert words[0] == words[1]
    assert np.unique(cls).size > 1


# ---- C: the coherence words ------------------------------------------------------------------------------------------------------------
def typed_batch(types, table, last=None):
    """One 256-ray block per entry of `types` (the block_incoherence value it is built to have), samples at lanes 100 and 227."""
    ext = float(np.max(np.maximum(table[0, 1::2], table[1, 1::2]) - np.minimum(table[0, 0::2], table[1, 0::2])))
    rays = np.zeros(256 * len(types), nt.RAY_DTYPE)
    rays["dx"], rays["tmax"] = 1.0, 100.0 * ext
    for b, t in enumerate(types):
        i1, i2 = 256 * b + 100, 256 * b + 227
        if t == 8:
            rays["tmin"][i1] = rays["tmax"][i1]
        elif t == 1:
            rays["ox"][i2] = 0.5 * ext
        elif t in (2, 6):
            rays["dx"][i2], rays["dy"][i2] = -0.5, 0.5
            if t == 2:
                rays["tmax"][i1] = 0.1 * ext
    return rays if last is None else rays[:last]


def coherence(dbvh, rays):
    out = torch.full((3,), 77, dtype=torch.int32, device=DEV)
    d = up(rays) if rays.shape[0] else torch.zeros(32, dtype=torch.uint8, device=DEV)
    nt.predict_batch_coherence(rays.shape[0], d.data_ptr(), dbvh.nodes.data_ptr(), dbvh.host.nodes.nbytes, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("wide", [None, "2", "4"])
def test_coherence_words_equal_the_restatement(soup, monkeypatch, wide):
    dbvh, _, pos, cam = soup
    if wide:
        monkeypatch.setenv("NTR_TRACE_MINIPOOL_WIDE", wide)
    nt.set_tunables()
    table = S.top_table(dbvh.host.nodes, dbvh.host.nodes.nbytes, 9)
    rng = np.random.default_rng(int(wide or 0))
    batches = []
    for nb in (64, 65):
        for apart in sorted({(nb - 1) // 2, nb // 2, (nb + 1) // 2, nb // 2 + 1}):    # 2 * apart around nb
            batches.append([1] * apart + [0] * (nb - apart))
        for total in (nb - 1, nb, nb + 1):                                              # 4 * apart + score around nb
            for apart, n6 in ((0, total // 4), (total // 8, (total - 4 * (total // 8)) // 4), (1, 0)):
                n8 = total - 4 * apart - 4 * n6
                if n8 < 0 or apart + n6 + n8 > nb:
                    continue
                batches.append([1] * apart + [6] * n6 + [8] * n8 + [2] * ((nb - apart - n6 - n8) // 2))
                batches[-1] += [0] * (nb - len(batches[-1]))
    for types in batches:
        types = list(rng.permutation(types))
        rays = typed_batch(types, table)
        assert S.block_incoherence(rays, table).tolist() == types
        want = S.coherence_words(rays, table, len(types), pool_k_wide(dbvh.host.nodes.nbytes, rays.shape[0]))
        assert coherence(dbvh, rays) == want, (types, want)
    for types, last in (([1], 99), ([1], 226), ([1], 228), ([6], 150), ([8], 101), ([1, 6], 256 + 99), ([6, 1], 256 + 228)):
        rays = typed_batch(types, table, last)
        want = S.coherence_words(rays, table, (last + 255) // 256, pool_k_wide(dbvh.host.nodes.nbytes, last))
        assert coherence(dbvh, rays) == want, (types, last, want)
    prim = scenes.primary_rays(cam, 320, 200)[0]
    rnd = scenes.random_rays(64000, seed=3)
    fan = rnd.copy()
    for k in ("ox", "oy", "oz"):
        fan[k] = prim[k][0]
    short = fan.copy()
    short["tmin"], short["tmax"] = 0.0, 1e-3
    for rays in (prim, rnd, fan, short, mixed_batch(cam, pos, 30001)):
        want = S.coherence_words(rays, table, (rays.shape[0] + 255) // 256, pool_k_wide(dbvh.host.nodes.nbytes, rays.shape[0]))
        assert coherence(dbvh, rays) == want
    assert coherence(dbvh, prim[:0]) == [0, 0, 1]


# ---- D: a predicted hint's order -------------------------------------------------------------------------------------------------------
def test_predicted_hint_order_equals_the_restatement(monkeypatch):
    rng = np.random.default_rng(4)
    for classes in (0, 1, 2, 31, 32, 33, 64, 1000):
        monkeypatch.setenv("NTR_SCHED_CLASSES", str(classes))
        nt.set_tunables()
        hint = nt.SchedHint()
        for nb in (1, 255, 256, 257, 511, 8192, 70001):
            small = rng.integers(0, 50, nb).astype(np.uint32)
            spike = small.copy()
            spike[nb // 3] = 0xFFFFFFFF
            for what, cost in (("zero", np.zeros(nb, np.uint32)), ("equal", np.full(nb, 12, np.uint32)), ("ramp", np.arange(nb, dtype=np.uint32)),
                               ("random", rng.integers(0, 1 << 20, nb).astype(np.uint32)), ("spike", spike),
                               ("2^24", (np.uint32(1 << 24) + rng.integers(-3, 4, nb)).astype(np.uint32))):
                d_cost = torch.from_numpy(cost.view(np.int32)).to(DEV)
                hint.predict(d_cost.data_ptr(), nb)
                st = hint.inspect()
                assert (st["numBlocks"], st["valid"], st["predicted"], st["uses"]) == (nb, 1, 1, 0)
                assert st["words"].tolist() == [0, 0, 0]
                assert np.array_equal(st["cost"], cost)
                want = S.sched_order(cost, classes)
                assert first_mismatch(st["order"], want) is None, (classes, nb, what, first_mismatch(st["order"], want))
        hint.close()


# ---- E / F: the hint over real launches ------------------------------------------------------------------------------------------------
def hinted_launch(dbvh, kernel, d_rays, n, hint):
    d_res = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device=DEV)
    dbvh.view.trace(kernel, n, False, d_rays.data_ptr(), d_res.data_ptr(), hint=hint)
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(nt.RESULT_DTYPE)


def lower_thresholds(monkeypatch, **more):
    monkeypatch.setenv("NTR_TRACE_PREDICT_MIN_RAYS", "1")
    monkeypatch.setenv("NTR_TRACE_PREDICT_MIN_NODES", "1")
    monkeypatch.setenv("NTR_SCHED_REFRESH_EVERY", "4")
    for k, v in more.items():
        monkeypatch.setenv(k, v)
    nt.set_tunables()


@pytest.mark.parametrize("kernel,route", [("fermi_speculative_while_while", None), ("kepler_dynamic_fetch", "0")])
def test_hint_life_cycle_over_real_launches(soup, monkeypatch, kernel, route):
    dbvh, _, pos, cam = soup
    lower_thresholds(monkeypatch, **({"NTR_TRACE_ROUTE": route} if route else {}))
    rays = np.concatenate([scenes.primary_rays(cam, 320, 240)[0], scenes.primary_rays(cam, 200, 100)[0]])   # coherent
    n = rays.shape[0]
    nb = (n + 255) // 256
    ref, _ = oracle.trace(dbvh.host.nodes, dbvh.host.woop, dbvh.host.tri_index, rays, any_hit=False, threads=8)
    d_rays = up(rays)
    plan = nt.trace_plan(kernel, n, False, dbvh.host.nodes.nbytes, dbvh.host.woop.nbytes, flags=nt._capi.PLAN_FLAG_CALLER_HINT).as_dict()
    assert plan["hintable"] and plan["predictable"]
    _, b_word = dispatch_order(dbvh, d_rays, n)
    classes = 32
    for start in ("fresh", "predicted"):
        hint = nt.SchedHint()
        if start == "predicted":
            pred = np.random.default_rng(1).integers(0, 100, nb).astype(np.uint32)
            d_pred = torch.from_numpy(pred.view(np.int32)).to(DEV)
            hint.predict(d_pred.data_ptr(), nb)
        prev = hint.inspect()
        for launch in range(12):
            step = nt.trace_plan_hint_step(prev["valid"], prev["predicted"], prev["uses"])
            zero_k, refresh = step["zeroK"], step["refresh"]
            predicts = plan["predictable"] and not prev["valid"]
            got = hinted_launch(dbvh, kernel, d_rays, n, hint)
            assert_parity(got, ref, "%s %s launch %d" % (kernel, start, launch))
            st = hint.inspect()
            what = (kernel, start, launch, prev["uses"])
            assert st["numBlocks"] == nb and st["uses"] == prev["uses"] + 1 and st["predicted"] == 0 and st["valid"] == 1, what
            if start == "predicted" and launch == 0:
                assert not refresh, what              # the first launch of a predicted order runs it without refreshing
            if refresh:
                assert st["cost"].max() > 0, what
                assert np.array_equal(st["order"], S.sched_order(st["cost"], classes)), what
            else:
                assert np.array_equal(st["order"], prev["order"]) and np.array_equal(st["cost"], prev["cost"]), what
            if predicts:
                assert st["words"][2] == b_word, (what, hex(st["words"][2]), hex(b_word))
            elif refresh and plan["probeOnRefresh"]:
                assert st["words"].tolist() == coherence(dbvh, rays), what
            elif not zero_k:
                assert np.array_equal(st["words"], prev["words"]), what
            prev = st
        hint.close()


def incoherent_rays(pos, n, seed):
    return scenes.box_rays(pos, n, seed=seed)


@pytest.mark.parametrize("setting", ["incoherent batch", "coherent batch, NTR_TRACE_WHOLE_WAVE=0, NTR_TRACE_ROUTE=0", "NTR_TRACE_UNIFIED=0"])
def test_a_launch_that_records_no_cost_keeps_a_predicted_order(soup, monkeypatch, setting):
    """kepler_dynamic_fetch in dynamic-fetch mode records no block cost.  Its refresh launches must not leave the hint valid on the
    identity order (derived from all-zero costs): the next launch would then skip the heavy-first prediction for good."""
    dbvh, _, pos, cam = soup
    kernel = "kepler_dynamic_fetch"
    if setting.startswith("coherent"):
        lower_thresholds(monkeypatch, NTR_TRACE_WHOLE_WAVE="0", NTR_TRACE_ROUTE="0")   # (routed, a coherent batch is the per-ray body's)
        rays = np.concatenate([scenes.primary_rays(cam, 320, 240)[0], scenes.random_rays(6000, seed=2)])
    else:
        lower_thresholds(monkeypatch, **({"NTR_TRACE_UNIFIED": "0"} if "UNIFIED" in setting else {}))
        rays = incoherent_rays(pos, 80000, seed=8)
    n = rays.shape[0]
    nb = (n + 255) // 256
    ref, _ = oracle.trace(dbvh.host.nodes, dbvh.host.woop, dbvh.host.tri_index, rays, any_hit=False, threads=8)
    d_rays = up(rays)
    table = S.top_table(dbvh.host.nodes, dbvh.host.nodes.nbytes, 9)
    cls = S.dispatch_class(S.block_costs(rays, table))
    b_order, _ = dispatch_order(dbvh, d_rays, n)
    identity = np.arange(nb)
    assert S.check_flatten_order(b_order, cls) is None and not np.array_equal(b_order, identity)   # precondition: a real prediction
    hint = nt.SchedHint()
    prev = hint.inspect()
    zero_refreshes = 0
    for launch in range(8):
        refresh = nt.trace_plan_hint_step(prev["valid"], prev["predicted"], prev["uses"])["refresh"]
        got = hinted_launch(dbvh, kernel, d_rays, n, hint)
        assert_parity(got, ref, "%s launch %d" % (setting, launch))
        st = hint.inspect()
        assert np.array_equal(np.sort(st["order"]), identity), (setting, launch, "the hint's order is not a permutation")
        if refresh and st["cost"].max() == 0:
            zero_refreshes += 1
            assert not (st["valid"] and np.array_equal(st["order"], identity)), (
                "%s, launch %d: a refresh that recorded no cost left the hint valid=1 on the identity order" % (setting, launch))
            if st["valid"]:
                assert S.check_flatten_order(st["order"], cls) is None, (setting, launch, S.check_flatten_order(st["order"], cls))
        prev = st
    hint.close()
    assert zero_refreshes > 0, "%s: every refresh recorded costs (the case under test did not occur)" % setting
