"""The numpy restatements the ray-side GPU tests (test_rayside_edges_gpu.py) compare the kernels with, pinned on the CPU: the vectorised
ray keys against the object-integer ones, the fminf box on NaN end points, the vectorised reconstruct against the per-task one, the
primary generator against scenes.primary_rays, and the pixel table at frames with only edge stripes."""
import numpy as np

import ntrace_amd as nt
from ntrace_amd import scenes
import np_raygen
from np_rayops import (f32_to_u32, np_ray_box, np_ray_keys, np_ray_keys_vec, np_ray_sort_order, np_reconstruct,
                       np_reconstruct_vec)

F = np.float32
TOL = 1e-5                                  # test_raygen_gpu.TOL
EDGE_FRAMES = ((1, 1), (7, 7), (8, 8), (9, 17), (1, 1000), (1000, 1), (63, 65))
SEEDS = (0x2545F491, 0xFFFFFFF0)            # the second wraps: seed + taskIdx passes 2^32 at taskIdx 16


def _words_to_int(words):
    return [int(a) | (int(b) << 64) | (int(c) << 128) for a, b, c in zip(*words)]


def test_vectorised_keys_equal_object_integer_keys():
    rays = scenes.random_rays(300, seed=5, tmax=4.0)
    rays[40:45] = rays[3]
    rays["tmax"][100:120] = -1.0            # degenerate rays of missed AO inputs: the end point lies behind the origin
    assert _words_to_int(np_ray_keys_vec(rays)) == np_ray_keys(rays)
    box = np_ray_box(scenes.random_rays(2000, seed=6, tmax=9.0))
    assert _words_to_int(np_ray_keys_vec(rays[:50], box)) == np_ray_keys(rays[:50], box)
    # the highest key bit is 149 (RAY_KEY_DIGITS = 19 digits of 8 bits cover it): a* < 2^25, b* < 2^22
    assert max(np_ray_keys(rays)) < 1 << 150


def test_box_drops_nan_end_points_as_fminf_does():
    """tmax = inf and a zero direction component: o + 0 * inf is NaN; fminf / fmaxf (the kernel, and the reference's
    FW_SPECIALIZE_MINMAX(F32, fminf, fmaxf)) drop it, np.minimum / np.maximum would not"""
    rays = np.zeros(3, dtype=nt.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = [1.0, -2.0, 0.5], [3.0, 4.0, -1.0], [0.0, 0.0, 2.0]
    rays["dx"], rays["dy"], rays["dz"] = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]
    rays["tmax"] = np.inf
    with np.errstate(invalid="ignore"):
        e = np.stack([rays["ox"] + rays["dx"] * rays["tmax"], rays["oy"] + rays["dy"] * rays["tmax"],
                      rays["oz"] + rays["dz"] * rays["tmax"]], 1)
    assert np.isnan(e).sum() == 6
    assert np.isnan(np.minimum(e.min(0), 0)).any()
    lo, hi = np_ray_box(rays)
    assert lo.dtype == F and hi.dtype == F
    assert np.array_equal(lo, np.array([-2.0, -1.0, -np.inf], dtype=F))
    assert np.array_equal(hi, np.array([np.inf, np.inf, 2.0], dtype=F))


def test_key_conversion_is_the_device_conversion():
    """(unsigned int)f on the device: truncation, saturating, NaN -> 0 -- what the degenerate batches (0 / 0 over a zero-extent box,
    0 * inf of a zero-length direction) produce"""
    x = np.array([np.nan, -1.5, -0.0, 0.0, 3.7, 16777216.0, 2.0 ** 33, np.inf, -np.inf], dtype=F)
    assert f32_to_u32(x).tolist() == [0, 0, 0, 0, 3, 16777216, 0xFFFFFFFF, 0xFFFFFFFF, 0]


def test_degenerate_batches_sort_as_expected():
    rays = np.repeat(scenes.random_rays(1, seed=2, tmax=0.0), 50)      # zero-extent box: position components 0 / 0
    w = np_ray_keys_vec(rays)
    assert all(np.array_equal(x, np.full(50, x[0])) for x in w)
    assert np.array_equal(np_ray_sort_order(rays), np.arange(50))
    zero = scenes.random_rays(64, seed=3, tmax=2.0)
    zero["dx"][::2] = zero["dy"][::2] = zero["dz"][::2] = 0.0         # 0 * (1 / 0): direction components NaN -> 0
    keys = np_ray_keys_vec(zero)
    mask = np.uint64(sum(1 << (3 + k + 6 * i) for k in range(3) for i in range(32) if 3 + k + 6 * i < 64))
    assert not (keys[0][::2] & mask).any()
    order = np_ray_sort_order(zero)
    assert np.array_equal(np.sort(order), np.arange(64))


def test_vectorised_reconstruct_equals_per_task_restatement():
    rng = np.random.default_rng(11)
    w, h, ntri = 20, 13, 9
    n = w * h
    slot_to_id = scenes.pixel_table(w, h)
    mat = np.array([0, 0xFFFFFFFF, 0x01010101, 0x80808080, 0xFEFDFCFB, 0x7F000080, 0x00FF00FF, 0x33333333, 0xCCCCCCCC], dtype=np.uint32)
    shaded = mat[::-1].copy()
    for ray_type in (0, 1, 2):
        for n_per, first, num in ((1, 0, n), (3, 7, 100), (16, 1, 60)):
            if ray_type == 0 and n_per != 1:
                continue
            p_res = np.zeros(n, dtype=nt.RESULT_DTYPE)
            p_res["id"] = rng.integers(-1, ntri, n)
            nb = n if ray_type == 0 else num * n_per
            b_res = np.zeros(nb, dtype=nt.RESULT_DTYPE)
            b_res["id"] = rng.integers(-1, ntri, nb)
            b_i2s = rng.permutation(nb).astype(np.int32)
            args = (ray_type, n_per, first, num, slot_to_id, p_res, b_i2s, b_res, mat, shaded)
            a = np_reconstruct(*args, np.full(n, 0x11223344, dtype=np.uint32))
            b = np_reconstruct_vec(*args, np.full(n, 0x11223344, dtype=np.uint32))
            assert np.array_equal(a, b), (ray_type, n_per, first, num)


def test_pixel_table_edge_frames():
    """frames where w & ~7 or h & ~7 is 0 have no 8x8 blocks: the table is the edge stripes alone (PixelTable.cpp:118-140)"""
    for w, h in EDGE_FRAMES:
        tab = scenes.pixel_table(w, h)
        assert np.array_equal(np.sort(tab), np.arange(w * h)), (w, h)
        if (w & ~7) == 0 or (h & ~7) == 0:
            assert np.array_equal(tab, np.arange(w * h)), (w, h)
    tab = scenes.pixel_table(9, 17)          # two 8x8 blocks, then the row y = 16 below them, then the column x = 8
    assert (tab[:64] % 9 < 8).all() and (tab[:64] // 9 < 8).all() and (tab[64:128] // 9 >= 8).all()
    assert np.array_equal(tab[128:136], np.arange(8) + 16 * 9)
    assert np.array_equal(tab[136:], np.arange(17) * 9 + 8)


def _screen_tol(w, h):
    """np_raygen.primary_rays takes the kernel's float32 screen position, scenes.primary_rays a float64 one: they differ by an ulp of
    the position (~1.2e-7) times the frame's aspect ratio"""
    return 1e-6 + 1.2e-7 * w / h


def test_primary_restatement_matches_scenes_and_seed_moves_rays():
    """seed 0: the float64 restatement of rayGenPrimaryKernel through the nscreenToWorld matrix is scenes.primary_rays; with a seed the
    jitter moves every frame's rays by far more than the GPU test's tolerance, so a kernel that ignored the seed could not pass it"""
    tri, pos, cam = scenes.cornell_box()
    for w, h in EDGE_FRAMES:
        tab = scenes.pixel_table(w, h)
        m = scenes.nscreen_to_world(cam, w, h)
        o, d, t = np_raygen.primary_rays(tab, cam["eye"], m, w, h, cam["far"])
        ref, _ = scenes.primary_rays(cam, w, h)
        refd = np.stack([ref["dx"], ref["dy"], ref["dz"]], 1).astype(np.float64)
        assert np.abs(d - refd).max() < _screen_tol(w, h), (w, h)
        assert (o == np.array([ref["ox"][0], ref["oy"][0], ref["oz"][0]], dtype=np.float64)).all() and (t == ref["tmax"]).all()
    cam = np_raygen.NEAR_ORIGIN_CAM              # the GPU test's camera
    for w, h in EDGE_FRAMES:
        tab = scenes.pixel_table(w, h)
        m = scenes.nscreen_to_world(cam, w, h)
        _, d, _ = np_raygen.primary_rays(tab, cam["eye"], m, w, h, cam["far"])
        ref, _ = scenes.primary_rays(cam, w, h)
        assert np.abs(d - np.stack([ref["dx"], ref["dy"], ref["dz"]], 1)).max() < _screen_tol(w, h), (w, h)
        for seed in SEEDS:
            _, ds, _ = np_raygen.primary_rays(tab, cam["eye"], m, w, h, cam["far"], seed)
            assert np.allclose(np.linalg.norm(ds, axis=1), 1.0)
            assert np.abs(ds - d).max() > 20 * TOL, (w, h, seed)


def test_ao_normals_decide_the_flip_in_float32():
    """an input ray perpendicular to the normal (float32 sum of products exactly 0) keeps the normal; a missed input takes (1, 0, 0)"""
    normals = np.array([[0.70710677, 0.70710677, 0.0], [-0.0, 1.0, -0.0], [0.0, 0.0, 1.0]], dtype=F)
    rays = np.zeros(6, dtype=nt.RAY_DTYPE)
    dirs = [(0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)]
    rays["dx"], rays["dy"], rays["dz"] = np.array(dirs, dtype=F).T
    res = np.zeros(6, dtype=nt.RESULT_DTYPE)
    res["id"] = [0, 1, 2, 2, -1, -1]
    n = np_raygen.ao_normals(rays, res, normals)
    assert np.array_equal(n, np.array([normals[0], normals[1], -normals[2], normals[2], [-1, 0, 0], [1, 0, 0]], dtype=np.float64))
