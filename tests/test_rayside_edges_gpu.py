"""The kernels on either side of the tracer at their edges (raygen_kernels.hip, rayops_kernels.hip): count_hits over every record kind
and past its grid-stride cap, the primary generator's jitter, the AO generator's frame branches and missed inputs, the shadow generator
past 32 samples, reconstruct around its 256-thread block, and the ray sort around its 2 048-key tile on the batches a frame gives it.
References are numpy restatements (np_raygen.py, np_rayops.py; pinned in test_rayside_restatements_cpu.py): exact where the kernel's
result is integer work or a plain float32 sequence, float64 within test_raygen_gpu's tolerances where the reference itself builds with
-use_fast_math."""
import math

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes
import np_raygen
from np_rayops import np_ray_sort_order, np_reconstruct_vec

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-5                                  # test_raygen_gpu.TOL
INT_MIN = -2 ** 31
CD = np.array([0xCDCDCDCD], dtype=np.uint32).view(np.int32)[0]     # a 0xCD byte prefill read as an id
EDGE_FRAMES = ((1, 1), (7, 7), (8, 8), (9, 17), (1, 1000), (1000, 1), (63, 65))
SEEDS = (0x2545F491, 0xFFFFFFF0)            # the second wraps: seed + taskIdx passes 2^32 at taskIdx 16


def _dev():
    import torch
    return torch.device("cuda:0")


def _zeros(n, dtype):
    import torch
    return torch.zeros(max(n, 1), dtype=dtype, device=_dev())


# ---- count_hits ----------------------------------------------------------------------------------------------------------------------

COUNT_SIZES = (1, 63, 64, 65, 255, 256, 257, 65_537, 524_287, 524_288, 524_289, 3_000_000)


def _records(ids):
    r = np.zeros(ids.shape[0], dtype=nt.RESULT_DTYPE)
    r["id"] = ids
    r["t"] = 1.0
    return r


def test_count_hits_counts_nonnegative_ids():
    """countHitsKernel counts records with id >= 0 (RendererKernels.cu:193): -2, INT_MIN and a 0xCD prefill are not hits.  Sizes around
    the 256-thread block and past the 2 048-block cap (524 288 records), where the grid-stride loop runs."""
    import torch
    from gpu_util import up
    top = COUNT_SIZES[-1]
    rng = np.random.default_rng(1)
    mix = rng.choice(np.array([-1, -2, INT_MIN, CD, 0, 1, 2 ** 31 - 1], dtype=np.int32), top)
    pos = rng.random(top) < 0.3
    mix[pos] = rng.integers(0, 2 ** 31 - 1, int(pos.sum()), dtype=np.int32)
    kinds = {"all -1": np.full(top, -1, np.int32), "all hits": np.arange(top, dtype=np.int32) % 1000, "mix": mix}
    for name, ids in kinds.items():
        d_res = up(_records(ids))
        torch.cuda.synchronize()
        for n in COUNT_SIZES:
            assert nt.count_hits(d_res.data_ptr(), n) == int((ids[:n] >= 0).sum()), (name, n)
        del d_res
    assert (mix == -2).any() and (mix == INT_MIN).any() and (mix == CD).any() and (mix == 0).any()


def test_count_hits_offset_pointer_stream_and_empty():
    """a pointer into the buffer as bench.py passes it (d_res + first * 16, first not a multiple of 256), a non-default stream, and
    numRays = 0"""
    import torch
    from gpu_util import up
    rng = np.random.default_rng(2)
    n_all = 700_000
    ids = rng.choice(np.array([-1, -2, INT_MIN, CD, 0, 5, 77], dtype=np.int32), n_all)
    d_res = up(_records(ids))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for first, cnt in ((37, 1), (37, 300), (1001, 65_537), (129, 524_289), (5, n_all - 5)):
        exp = int((ids[first:first + cnt] >= 0).sum())
        assert nt.count_hits(d_res.data_ptr() + first * 16, cnt) == exp, (first, cnt)
        assert nt.count_hits(d_res.data_ptr() + first * 16, cnt, s.cuda_stream) == exp, (first, cnt, "stream")
    assert nt.count_hits(d_res.data_ptr(), 0) == 0
    assert nt.count_hits(d_res.data_ptr() + 16, 0, s.cuda_stream) == 0
    assert nt.count_hits(0, 0) == 0


# ---- pixel table and primary rays ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", EDGE_FRAMES)
def test_pixel_table_and_primary_rays_edge_frames(w, h):
    """PixelTable (PixelTable.cpp:57-143) at frames with only edge stripes or one block; rayGenPrimaryKernel (RayGenKernels.cu:77-125)
    with seed 0 and two seeds, one wrapping seed + taskIdx past 2^32: the jitter restated within TOL, and far from the seed-0 rays"""
    import torch
    cam = np_raygen.NEAR_ORIGIN_CAM
    n = w * h
    d_tab = _zeros(n, torch.int32)
    d_inv = _zeros(n, torch.int32)
    nt.pixel_table(w, h, d_tab.data_ptr(), d_inv.data_ptr())
    tab = d_tab.cpu().numpy()[:n]
    assert np.array_equal(tab, scenes.pixel_table(w, h))
    assert np.array_equal(d_inv.cpu().numpy()[tab], np.arange(n))
    assert np.array_equal(tab[d_inv.cpu().numpy()[:n]], np.arange(n))
    m = scenes.nscreen_to_world(cam, w, h)
    eye = np.asarray(cam["eye"], dtype=F)
    _, d0, _ = np_raygen.primary_rays(tab, cam["eye"], m, w, h, cam["far"])
    for seed in (0,) + SEEDS:
        d_rays = torch.full((n * 8,), float("nan"), dtype=torch.float32, device=_dev())
        d_i2s = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        d_s2i = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        nt.raygen_primary(d_rays.data_ptr(), d_i2s.data_ptr(), d_s2i.data_ptr(), d_tab.data_ptr(), cam["eye"], m, w, h, cam["far"], seed)
        torch.cuda.synchronize()
        got = d_rays.cpu().numpy().reshape(-1, 8)
        assert np.array_equal(got[:, :3], np.repeat(eye[None, :], n, 0)) and (got[:, 3] == 0).all(), seed
        assert (got[:, 7] == F(cam["far"])).all(), seed
        s2i = d_s2i.cpu().numpy()
        assert np.array_equal(s2i, tab) and np.array_equal(d_i2s.cpu().numpy()[s2i], np.arange(n)), seed
        _, d, _ = np_raygen.primary_rays(tab, cam["eye"], m, w, h, cam["far"], seed)
        assert np.abs(got[:, 4:7] - d).max() < TOL, seed
        assert np.allclose(np.linalg.norm(got[:, 4:7], axis=1), 1.0, atol=1e-5)
        if seed:
            assert np.abs(got[:, 4:7] - d0).max() > 10 * TOL, ("the kernel ignored seed", seed)


# ---- AO rays -------------------------------------------------------------------------------------------------------------------------

def _ao_inputs(count, seed=0):
    """a hand-built AO input batch: normals +-x, +-y, +-z, tied largest components, -0.0 components; input rays facing each normal,
    leaving it, and perpendicular to it (float32 sum of products exactly 0); every fifth input missed"""
    r2, r3 = 1.0 / math.sqrt(2.0), 1.0 / math.sqrt(3.0)
    table = [((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0)),
             ((0, 0, 1), (1, 0, 0)), ((0, 0, -1), (0, 1, 0)),
             ((r2, r2, 0), (0.5, -0.5, 0)), ((0, r2, r2), (0, 0.5, -0.5)), ((r2, 0, r2), (0.5, 0, -0.5)), ((r3, r3, r3), (0.5, -0.5, 0)),
             ((-r2, -r2, 0), (0, 0, 1)), ((r2, -r2, 0), (0.5, 0.5, 0)), ((-r3, r3, -r3), (0.5, 0.5, 0)),
             ((-0.0, 1, -0.0), (1, 0, 0)), ((-0.0, -0.0, -1), (0, 1, 0)), ((1, -0.0, 0), (0, -0.0, 1))]
    normals = np.array([t[0] for t in table], dtype=F)
    perp = np.array([t[1] for t in table], dtype=F)
    assert (((normals * perp).astype(F)).sum(1) == 0).all()
    rng = np.random.default_rng(seed)
    tri = np.arange(count) % len(table)
    mode = (np.arange(count) // len(table)) % 3          # 0 facing, 1 leaving, 2 perpendicular
    d = np.where((mode == 0)[:, None], -normals[tri], np.where((mode == 1)[:, None], normals[tri], perp[tri]))
    miss = np.arange(count) % 5 == 4
    d[miss] = rng.normal(size=(int(miss.sum()), 3))
    d[miss] /= np.linalg.norm(d[miss], axis=1, keepdims=True)
    rays = np.zeros(count, dtype=nt.RAY_DTYPE)
    o = rng.uniform(-3, 3, size=(count, 3))
    rays["ox"], rays["oy"], rays["oz"] = o.T.astype(F)
    rays["dx"], rays["dy"], rays["dz"] = d.T.astype(F)
    rays["tmax"] = 50.0
    res = np.zeros(count, dtype=nt.RESULT_DTYPE)
    res["id"] = np.where(miss, -1, tri)
    res["t"] = rng.uniform(0.5, 4.0, count).astype(F)
    res["t"][::7] = 5e-5                    # backs off to the origin itself
    return rays, res, normals


def test_ao_rays_branches_and_missed_inputs():
    """rayGenAOKernel (RayGenKernels.cu:129-236): exact tmax (-1 for missed inputs), tmin and id maps; origins and directions against
    the float64 restatement; unit directions in the hemisphere of the (flipped) normal, independently of the restatement"""
    import torch
    from gpu_util import up
    rays, res, normals = _ao_inputs(300)
    d_rays, d_res, d_nrm = up(rays), up(res), up(normals)
    maxd = 3.5
    for seed in (0, 0x5EED1234):
        for first in (0, 37):
            for count in (1, 255, 256, 257):
                n_in = np_raygen.ao_normals(rays, res, normals, first, count)
                for ns in (1, 2, 3, 8, 17, 64):
                    n = count * ns
                    d_out = torch.full((n * 8,), float("nan"), dtype=torch.float32, device=_dev())
                    d_a = torch.full((n,), -7, dtype=torch.int32, device=_dev())
                    d_b = torch.full((n,), -7, dtype=torch.int32, device=_dev())
                    nt.raygen_ao(d_out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(),
                                 first, count, ns, maxd, seed)
                    torch.cuda.synchronize()
                    got = d_out.cpu().numpy().reshape(-1, 8)
                    what = (seed, first, count, ns)
                    ro, rd, rt = np_raygen.ao_rays(rays, res, normals, ns, maxd, seed, first, count)
                    assert np.array_equal(got[:, 7], rt.astype(F)), what
                    assert (got[:, 7] == -1).sum() == (res["id"][first:first + count] == -1).sum() * ns, what
                    assert (got[:, 3] == 0).all(), what
                    assert np.array_equal(d_a.cpu().numpy(), np.arange(n)) and np.array_equal(d_b.cpu().numpy(), np.arange(n)), what
                    assert np.abs(got[:, :3] - ro).max() < 1e-4 * max(1.0, np.abs(ro).max()), what
                    assert np.abs(got[:, 4:7] - rd).max() < 5e-5, what
                    gd = got[:, 4:7].astype(np.float64)
                    assert np.allclose(np.linalg.norm(gd, axis=1), 1.0, atol=1e-5), what
                    assert ((gd * np.repeat(n_in, ns, axis=0)).sum(1) >= -1e-6).all(), what


# ---- shadow rays ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup_frame():
    from gpu_util import DeviceBvh, gpu_trace
    tri, pos, cam = scenes.random_soup(5000, seed=3)
    dbvh = DeviceBvh(nt.sah_build(tri, pos))
    rays, _ = scenes.primary_rays(cam, 48, 32)
    res, _ = gpu_trace("fermi_speculative_while_while", dbvh, rays, False)
    return tri, pos, dbvh, rays, res


@pytest.mark.parametrize("ns,radius", [(1, 0.75), (33, 0.75), (33, 0.0)])
def test_shadow_rays_edges(soup_frame, ns, radius):
    """rayGenShadowKernel (RayGenKernels.cu:240-301) with one sample, past the 32 samples of one Sobol word, with a point light, and
    with inputs hit closer than the 1e-2 back-off (the origin stays the input's): the checks of test_raygen_gpu's shadow test"""
    import torch
    from gpu_util import assert_parity, gpu_trace, up
    from oracle import oracle
    tri, pos, dbvh, rays, res = soup_frame
    first, count, seed = 100, 1000, 0x13579BDF
    res = res.copy()
    res["id"][first + 5::7] = -1
    hit = np.nonzero(res["id"] >= 0)[0]
    hit = hit[(hit >= first) & (hit < first + count)]
    near_in = np.zeros(res.shape[0], dtype=bool)
    for k, t in enumerate((0.005, 0.0, 0.01)):          # hit closer than the back-off: the origin is the input ray's own
        res["t"][hit[k::9]] = t
        near_in[hit[k::9]] = True
    light = (float(pos[:, 0].mean()), float(pos[:, 1].max()) * 0.9, float(pos[:, 2].mean()))
    n = count * ns
    d_out = torch.full((n * 8,), float("nan"), dtype=torch.float32, device=_dev())
    d_a = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    d_b = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    d_rays, d_res = up(rays), up(res)
    nt.raygen_shadow(d_out.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_rays.data_ptr(), d_res.data_ptr(), first, count, ns, light, radius, seed)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().reshape(-1, 8)
    ro, rd, rt = np_raygen.shadow_rays(rays, res, ns, light, radius, seed, first, count, f32_wrap=True)
    scale = max(1.0, np.abs(ro).max())
    assert np.abs(got[:, :3] - ro).max() < 1e-4 * scale
    near = np.repeat(near_in[first:first + count], ns)
    assert near.any()
    o_in = np.repeat(np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)[first:first + count], ns, axis=0)
    assert np.array_equal(got[near, :3], o_in[near])
    assert np.abs(got[:, 4:7] - rd).max() < 5e-5
    miss = rt < 0
    assert miss.any() and (~miss).any()
    assert np.array_equal(got[miss, 7], np.full(int(miss.sum()), -1.0, dtype=F))
    assert np.abs(got[~miss, 7] - rt[~miss]).max() < 1e-4 * scale
    assert (got[:, 3] == 0).all() and np.allclose(np.linalg.norm(got[:, 4:7], axis=1), 1.0, atol=1e-5)
    assert np.array_equal(d_a.cpu().numpy(), np.arange(n)) and np.array_equal(d_b.cpu().numpy(), np.arange(n))
    srays = d_out.cpu().numpy().view(nt.RAY_DTYPE).reshape(-1)
    ref, _ = oracle.trace(dbvh.host.nodes, dbvh.host.woop, dbvh.host.tri_index, srays, any_hit=True, threads=8)
    for kernel in nt.KERNELS:
        g, _ = gpu_trace(kernel, dbvh, srays, True)
        assert_parity(g, ref, "shadow batch ns=%d radius=%g, %s" % (ns, radius, kernel))


# ---- reconstruct ---------------------------------------------------------------------------------------------------------------------

# colours on the conversion's edges: 0, all ones, and channels whose n-sample average is exactly k / 255 in exact arithmetic
COLOURS = np.array([0x00000000, 0xFFFFFFFF, 0x01010101, 0x80808080, 0x7F7F7F7F, 0xFEFEFEFE, 0x00FF00FF, 0xFF00FF00, 0x33333333,
                    0xCCCCCCCC, 0x03020100, 0xFFFEFDFC, 0x55AA55AA], dtype=np.uint32)


@pytest.mark.parametrize("ray_type", [0, 1, 2])
def test_reconstruct_ragged_sizes_and_colour_edges(ray_type):
    """reconstructKernel (RendererKernels.cu:59-172) for numPrimary around the 256-thread block, an offset first primary slot, and
    1, 2, 3 and 16 rays per primary; every pixel equals the float32 restatement, the ones the batch does not write keep their prefill"""
    import torch
    from gpu_util import up
    rng = np.random.default_rng(40 + ray_type)
    w, h = 40, 33
    npix = w * h
    ntri = COLOURS.size
    slot_to_id = scenes.pixel_table(w, h)
    mat = COLOURS.copy()
    shaded = np.roll(COLOURS, 3)
    d_s2i, d_mat, d_sh = up(slot_to_id), up(mat), up(shaded)
    prefill = 0x11223344
    for num in (1, 255, 256, 257, 1000):
        for first in (0, 1, 300):
            for n_per in ((1,) if ray_type == 0 else (1, 2, 3, 16)):
                p_res = np.zeros(npix, dtype=nt.RESULT_DTYPE)
                p_res["id"] = rng.integers(-1, ntri, npix)
                nb = npix if ray_type == 0 else num * n_per
                b_ids = rng.integers(-1, ntri, nb)
                if ray_type != 0:               # a third of the primaries: every sample hits the same triangle (uniform average)
                    same = rng.integers(-1, ntri, num)
                    uni = np.arange(num) % 3 == 0
                    b_ids.reshape(num, n_per)[uni] = same[uni, None]
                b_i2s = rng.permutation(nb).astype(np.int32)
                b_res = np.zeros(nb, dtype=nt.RESULT_DTYPE)
                b_res["id"] = b_ids if ray_type == 0 else b_ids[np.argsort(b_i2s)]    # slot b_i2s[r] holds ray r's record
                d_pix = torch.full((npix,), prefill, dtype=torch.int32, device=_dev())
                bufs = [up(p_res), up(b_i2s), up(b_res)]
                nt.reconstruct(ray_type, n_per, first, num, d_s2i.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                               d_mat.data_ptr(), d_sh.data_ptr(), d_pix.data_ptr())
                torch.cuda.synchronize()
                got = d_pix.cpu().numpy().view(np.uint32)
                exp = np_reconstruct_vec(ray_type, n_per, first, num, slot_to_id, p_res, b_i2s, b_res, mat, shaded,
                                         np.full(npix, prefill, dtype=np.uint32))
                what = (num, first, n_per)
                assert np.array_equal(got, exp), (what, int(np.count_nonzero(got != exp)))
                written = np.zeros(npix, dtype=bool)
                written[slot_to_id[first:first + num]] = True
                assert (got[~written] == prefill).all(), what


# ---- ray sort ------------------------------------------------------------------------------------------------------------------------

SORT_SIZES = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 65_537)
SORT_MAX = SORT_SIZES[-1]


@pytest.fixture(scope="module")
def sort_batches():
    """SORT_MAX rays of each batch kind; a test sorts prefixes"""
    import torch
    from gpu_util import up
    out = {"random": scenes.random_rays(SORT_MAX, seed=31, tmax=6.0)}
    # an AO batch as a frame makes it: 4 rays per input, a fifth of the inputs missed (tmax = -1)
    ns = 4
    count = -(-SORT_MAX // ns)
    rays, res, normals = _ao_inputs(count, seed=5)
    d_out = torch.zeros(count * ns * 32, dtype=torch.uint8, device=_dev())
    d_a = torch.zeros(count * ns, dtype=torch.int32, device=_dev())
    d_in, d_res, d_nrm = up(rays), up(res), up(normals)
    nt.raygen_ao(d_out.data_ptr(), d_a.data_ptr(), d_a.data_ptr(), d_in.data_ptr(), d_res.data_ptr(), d_nrm.data_ptr(), 0, count, ns, 2.0,
                 0xFFF2D5E4)
    torch.cuda.synchronize()
    out["ao"] = d_out.cpu().numpy().view(nt.RAY_DTYPE)[:SORT_MAX].copy()
    assert (out["ao"]["tmax"] == -1).any()
    # a primary batch: one eye, PixelTable order
    tri, pos, cam = scenes.cornell_box()
    w, h = 257, 256
    d_tab = _zeros(w * h, torch.int32)
    nt.pixel_table(w, h, d_tab.data_ptr())
    d_p = torch.zeros(w * h * 32, dtype=torch.uint8, device=_dev())
    d_i = _zeros(w * h, torch.int32)
    nt.raygen_primary(d_p.data_ptr(), d_i.data_ptr(), d_i.data_ptr(), d_tab.data_ptr(), cam["eye"], scenes.nscreen_to_world(cam, w, h), w, h,
                      cam["far"], 0)
    torch.cuda.synchronize()
    out["primary"] = d_p.cpu().numpy().view(nt.RAY_DTYPE)[:SORT_MAX].copy()
    # n copies of one ray, with tmax = 0: a zero-extent box, position components 0 / 0
    out["identical"] = np.repeat(scenes.random_rays(1, seed=8, tmax=0.0), SORT_MAX)
    # zero-length directions among ordinary rays
    z = scenes.random_rays(SORT_MAX, seed=9, tmax=3.0)
    zl = np.random.default_rng(9).random(SORT_MAX) < 0.4
    z["dx"][zl] = z["dy"][zl] = z["dz"][zl] = 0.0
    out["zero_dir"] = z
    # axis-parallel directions with tmax = inf: o + 0 * inf is NaN (dropped by the box), o +- inf spans the box to infinity -- here
    # -inf..inf in x, finite..inf in y, finite in z
    rng = np.random.default_rng(10)
    a = scenes.random_rays(SORT_MAX, seed=10, tmax=np.inf)
    axis = rng.integers(0, 2, SORT_MAX)
    sign = np.where(axis == 0, rng.choice(np.array([-1.0, 1.0], dtype=F), SORT_MAX), F(1.0))
    for k, name in enumerate(("dx", "dy", "dz")):
        a[name] = np.where(axis == k, sign, F(0.0))
    out["axis_inf"] = a
    return out


@pytest.mark.parametrize("kind", ["random", "ao", "primary", "identical", "zero_dir", "axis_inf"])
def test_ray_morton_sort_exact_order(sort_batches, kind):
    """ntr_ray_morton_sort at sizes around its 2 048-key tile (OS_THREADS * ITEMS) and at n = 1, 2: the output order is the restated
    one exactly (192-bit key over the batch's own fminf box, ties in slot order), rays and both id maps follow it"""
    import torch
    from gpu_util import up
    rng = np.random.default_rng(len(kind))
    for n in SORT_SIZES:
        rays = sort_batches[kind][:n].copy()
        slot_to_id = rng.permutation(n).astype(np.int32)
        d_in, d_s2i = up(rays), up(slot_to_id)
        d_out = torch.zeros(n * 32, dtype=torch.uint8, device=_dev())
        d_i2s = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        d_s2i_out = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        nt.ray_morton_sort(n, d_in.data_ptr(), d_s2i.data_ptr(), d_out.data_ptr(), d_i2s.data_ptr(), d_s2i_out.data_ptr())
        order = np_ray_sort_order(rays)
        if kind == "identical":
            assert np.array_equal(order, np.arange(n))
        got = d_out.cpu().numpy().view(nt.RAY_DTYPE)
        s2i = d_s2i_out.cpu().numpy()
        first_bad = np.nonzero(s2i != slot_to_id[order])[0]
        assert first_bad.size == 0, (kind, n, int(first_bad.size), int(first_bad[0]) if first_bad.size else None)
        assert np.array_equal(got.view(np.uint32).reshape(n, 8), rays[order].view(np.uint32).reshape(n, 8)), (kind, n)
        assert np.array_equal(d_i2s.cpu().numpy()[s2i], np.arange(n)), (kind, n)
