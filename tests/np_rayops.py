"""numpy restatements of rayops_kernels.hip: reconstructKernel (src/rt/cuda/RendererKernels.cu:59-172) and the secondary-ray Morton
keys (RayBuffer.cpp:103-165, RayBufferKernels.cu:70-175).  Both are plain IEEE binary32 arithmetic and integer work (the library
builds with -ffp-contract=off), so every function here restates the kernel's float32 sequence and is compared bit for bit."""
import numpy as np

F = np.float32
BG = np.array([0.2, 0.4, 0.8, 1.0], dtype=F)   # RendererKernels.cu:101


def np_from_abgr(c):
    c = c.astype(np.uint32)
    k = F(1.0) / F(255.0)
    return np.stack([(c & 0xFF).astype(F) * k, ((c >> 8) & 0xFF).astype(F) * k, ((c >> 16) & 0xFF).astype(F) * k,
                     (c >> 24).astype(F) * k], -1).astype(F)


def np_to_abgr(v):
    b = (np.minimum(np.maximum(v, F(0)), F(1)) * F(255.0)).astype(np.uint32)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


def np_reconstruct(ray_type, n_per, first, num, p_slot_to_id, p_res, b_id_to_slot, b_res, mat, shaded, pixels):
    """reconstructKernel one task at a time (RendererKernels.cu:59-172)"""
    for task in range(num):
        pslot = first + task
        pid = p_slot_to_id[pslot]
        slots = b_id_to_slot[pid:pid + n_per] if ray_type == 0 else b_id_to_slot[task * n_per:(task + 1) * n_per]
        col = np.zeros(4, dtype=F)
        for s in slots:
            tri = b_res["id"][s]
            if tri == -1:
                add = BG if ray_type == 0 else np.ones(4, dtype=F)
            elif ray_type == 1:
                add = np.array([0, 0, 0, 1], dtype=F)
            else:
                add = np_from_abgr(shaded[tri:tri + 1])[0]
            col = (col + add).astype(F)
        col = (col * (F(1.0) / F(n_per))).astype(F)
        ptri = p_res["id"][pslot]
        if ray_type == 1 and ptri == -1:
            col = BG.copy()
        if ray_type == 2:
            col = (col * (BG if ptri == -1 else np_from_abgr(mat[ptri:ptri + 1])[0])).astype(F)
        pixels[pid] = np_to_abgr(col[None])[0]
    return pixels


def np_reconstruct_vec(ray_type, n_per, first, num, p_slot_to_id, p_res, b_id_to_slot, b_res, mat, shaded, pixels):
    """np_reconstruct vectorised over the tasks: the same float32 sequence (samples summed in order, then * (1 / n), then the
    material), so equal bit for bit; ids must be >= -1, as the kernel reads the colour tables at any other id."""
    task = np.arange(num)
    pslot = first + task
    pid = p_slot_to_id[pslot]
    base = pid if ray_type == 0 else task * n_per
    col = np.zeros((num, 4), dtype=F)
    for i in range(n_per):
        tri = b_res["id"][b_id_to_slot[base + i]]
        miss = (tri == -1)[:, None]
        if ray_type == 1:
            add = np.where(miss, np.ones(4, dtype=F), np.array([0, 0, 0, 1], dtype=F))
        else:
            add = np.where(miss, BG if ray_type == 0 else np.ones(4, dtype=F), np_from_abgr(shaded[np.maximum(tri, 0)]))
        col = (col + add.astype(F)).astype(F)
    col = (col * (F(1.0) / F(n_per))).astype(F)
    ptri = p_res["id"][pslot]
    if ray_type == 1:
        col = np.where((ptri == -1)[:, None], BG, col).astype(F)
    if ray_type == 2:
        m = np.where((ptri == -1)[:, None], BG, np_from_abgr(mat[np.maximum(ptri, 0)]))
        col = (col * m).astype(F)
    pixels[pid] = np_to_abgr(col)
    return pixels


def _parts(rays):
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1).astype(F)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1).astype(F)
    return o, d


def np_ray_box(rays):
    """findAABBKernel (RayBufferKernels.cu:70-136): box of the origins and the end points o + d * tmax, reduced with fminf / fmaxf
    (FW_SPECIALIZE_MINMAX(F32, fminf, fmaxf)), which drop a NaN operand -- np.fmin / np.fmax, not np.minimum / np.maximum."""
    o, d = _parts(rays)
    with np.errstate(all="ignore"):
        e = (o + (d * rays["tmax"][:, None]).astype(F)).astype(F)
    lo = np.fmin(np.fmin.reduce(o, axis=0), np.fmin.reduce(e, axis=0)).astype(F)
    hi = np.fmax(np.fmax.reduce(o, axis=0), np.fmax.reduce(e, axis=0)).astype(F)
    return lo, hi


def _components(rays, box):
    """the six float32 key components of genMortonKeysKernel (RayBufferKernels.cu:140-175) before the conversion to U32"""
    o, d = _parts(rays)
    lo, hi = box if box is not None else np_ray_box(rays)
    with np.errstate(all="ignore"):
        a = ((o - lo) / (hi - lo)).astype(F)
        ln = np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
        inv = (F(1.0) * (F(1.0) / ln)).astype(F)
        b = (((d * inv[:, None]).astype(F) + F(1.0)).astype(F) * F(0.5)).astype(F)
        return [(a[:, k] * F(256.0) * F(65536.0)).astype(F) for k in range(3)] + [(b[:, k] * F(32.0) * F(65536.0)).astype(F) for k in range(3)]


def np_ray_keys(rays, box=None):
    """the 192-bit sort keys (RayBuffer.cpp:103-165) as Python integers; `box`: the (lo, hi) of the batch the rays are a sample of"""
    with np.errstate(all="ignore"):
        comp = [c.astype(np.int64).astype(np.uint64) & 0xFFFFFFFF for c in _components(rays, box)]
    big = [int(0)] * rays.shape[0]
    for k in range(6):
        ck = comp[k]
        for i in range(32):
            bit = ((ck >> np.uint64(i)) & np.uint64(1)).astype(np.uint64)
            pos = k + 6 * i
            for r in np.nonzero(bit)[0]:
                big[r] |= 1 << pos
    return big


def f32_to_u32(x):
    """(unsigned int)x as the device converts it (v_cvt_u32_f32, like the reference's cvt.rzi.u32.f32): truncation, saturating at 0
    and 2^32 - 1, NaN -> 0"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(np.isnan(x), 0.0, x))
    return np.clip(t, 0.0, 4294967295.0).astype(np.uint64)


def np_ray_keys_vec(rays, box=None):
    """the 192-bit keys vectorised: component k's bit i goes to key bit k + 6 i (RayBufferKernels.cu:160-170); returns three uint64
    words, least significant first"""
    comp = [f32_to_u32(c) for c in _components(rays, box)]
    words = [np.zeros(rays.shape[0], dtype=np.uint64) for _ in range(3)]
    for k in range(6):
        for i in range(32):
            pos = k + 6 * i
            words[pos >> 6] |= ((comp[k] >> np.uint64(i)) & np.uint64(1)) << np.uint64(pos & 63)
    return words


def np_ray_sort_order(rays):
    """the order ntr_ray_morton_sort puts the batch in: ascending 192-bit key over the batch's own box, equal keys in slot order"""
    w = np_ray_keys_vec(rays)
    return np.lexsort((np.arange(rays.shape[0]), w[0], w[1], w[2]))
