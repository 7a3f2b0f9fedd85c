"""numpy restatements of the ray generators of src/rt/ray/RayGenKernels.cu (primary :77-125, AO :129-236, shadow :240-301) for
testing the device ray generators to a floating-point tolerance (the reference builds these kernels with -use_fast_math, so no
bit-exact target exists for them).  Values are float64; where a kernel branches on a float32 value, the branch is decided on the
float32 value, as the kernel decides it, so that a case on the boundary is not a false mismatch."""
import numpy as np


def _jenkins(a, b, c):
    M = np.uint32
    with np.errstate(over="ignore"):
        a = a - b; a = a - c; a = a ^ (c >> M(13))
        b = b - c; b = b - a; b = b ^ (a << M(8))
        c = c - a; c = c - b; c = c ^ (b >> M(13))
        a = a - b; a = a - c; a = a ^ (c >> M(12))
        b = b - c; b = b - a; b = b ^ (a << M(16))
        c = c - a; c = c - b; c = c ^ (b >> M(5))
        a = a - b; a = a - c; a = a ^ (c >> M(3))
        b = b - c; b = b - a; b = b ^ (a << M(10))
        c = c - a; c = c - b; c = c ^ (b >> M(15))
    return a, b, c


def ao_normals(in_rays, in_results, normals, first=0, count=None):
    """the AO generator's normal per input ray (RayGenKernels.cu:155-162): the hit triangle's normal, (1, 0, 0) for a missed input,
    negated when it faces along the ray; the facing test is the kernel's float32 sum of products (exact 0: no flip)"""
    count = in_rays.shape[0] - first if count is None else count
    r = in_rays[first:first + count]
    tri = in_results["id"][first:first + count]
    n = np.where((tri != -1)[:, None], normals[np.maximum(tri, 0)].astype(np.float32), np.array([1.0, 0.0, 0.0], dtype=np.float32))
    F = np.float32
    dot = ((n[:, 0] * r["dx"]).astype(F) + (n[:, 1] * r["dy"]).astype(F)).astype(F) + (n[:, 2] * r["dz"]).astype(F)
    n = n.astype(np.float64)
    n[dot > 0] = -n[dot > 0]
    return n


# A pinhole camera whose eye is near the origin, looking obliquely: the kernel forms the direction as (world point - eye) in float32,
# which for an eye far from the origin (the Cornell camera sits at |eye| ~ 850) cancels to ~1e-5 and would hide a wrong jitter of that size.
NEAR_ORIGIN_CAM = {"eye": (0.3, -0.2, 0.5), "target": (-1.0, 0.4, 3.0), "up": (0.0, 1.0, 0.0), "fov_deg": 55.0, "far": 100.0}


def primary_rays(index_to_pixel, origin, nscreen_to_world, w, h, max_dist, kernel_seed=0):
    """rayGenPrimaryKernel (RayGenKernels.cu:77-125): (origins, unit directions, tmax) of the w * h rays in slot order.
    kernel_seed != 0 offsets the normalised screen position by (F32)hash * 2^-32 * 0.005 (:95-106).  The normalised screen position is
    the kernel's float32 sequence (2 (x + 0.5) / w - 1 cancels near the centre, and a 1000:1 frame magnifies that 1000-fold); the
    jitter, the transform and the normalisation are float64."""
    n = w * h
    F = np.float32
    pix = np.asarray(index_to_pixel[:n], dtype=np.int64)
    nx = ((F(2.0) * ((pix % w).astype(F) + F(0.5))).astype(F) / F(w) - F(1.0)).astype(F).astype(np.float64)
    ny = ((F(2.0) * ((pix // w).astype(F) + F(0.5))).astype(F) / F(h) - F(1.0)).astype(F).astype(np.float64)
    if kernel_seed != 0:
        with np.errstate(over="ignore"):
            a = (np.uint32(kernel_seed) + np.arange(n, dtype=np.uint32)).astype(np.uint32)
        b = np.full(n, 0x9e3779b9, dtype=np.uint32)
        c = np.full(n, 0x9e3779b9, dtype=np.uint32)
        a, b, c = _jenkins(a, b, c)
        a, b, c = _jenkins(a, b, c)
        nx = nx + a.astype(np.float32).astype(np.float64) * 2.0 ** -32 * 0.005
        ny = ny + b.astype(np.float32).astype(np.float64) * 2.0 ** -32 * 0.005
    m = np.asarray(nscreen_to_world, dtype=np.float32).astype(np.float64).reshape(4, 4)
    world = m[:, 0][None, :] * nx[:, None] + m[:, 1][None, :] * ny[:, None] + m[:, 3][None, :]
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    d = world[:, :3] / world[:, 3:4] - o[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(o[None, :], n, axis=0), d, np.full(n, float(np.float32(max_dist)))


def ao_rays(in_rays, in_results, normals, num_samples, max_dist, kernel_seed, first=0, count=None):
    count = in_rays.shape[0] - first if count is None else count
    r = in_rays[first:first + count]
    res = in_results[first:first + count]
    o = np.stack([r["ox"], r["oy"], r["oz"]], 1).astype(np.float64)
    d = np.stack([r["dx"], r["dy"], r["dz"]], 1).astype(np.float64)
    back = np.maximum(res["t"].astype(np.float64) - 1.0e-4, 0.0)
    origin = o + d * back[:, None]
    tri = res["id"]
    n = ao_normals(in_rays, in_results, normals, first, count)
    na = np.abs(n)          # float32 values held exactly: the ties nm == az, nm == ax are decided as in float32
    nm = na.max(1)
    perp = np.stack([n[:, 1], -n[:, 0], np.zeros(count)], 1)
    zc = nm == na[:, 2]
    xc = ~zc & (nm == na[:, 0])
    perp[zc] = np.stack([np.zeros(count), n[:, 2], -n[:, 1]], 1)[zc]
    perp[xc] = np.stack([-n[:, 2], np.zeros(count), n[:, 0]], 1)[xc]
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    biperp = np.cross(n, perp)
    task = np.arange(count, dtype=np.uint32)
    a, b, c = _jenkins(np.uint32(kernel_seed) + task, np.full(count, 0x9e3779b9, np.uint32), np.full(count, 0x9e3779b9, np.uint32))
    a, b, c = _jenkins(a, b, c)
    angle = 2.0 * np.pi * c.astype(np.float32).astype(np.float64) * 2.0 ** -32
    t0 = perp * np.cos(angle)[:, None] + biperp * np.sin(angle)[:, None]
    t1 = perp * -np.sin(angle)[:, None] + biperp * np.cos(angle)[:, None]
    out_o = np.repeat(origin, num_samples, axis=0)
    out_d = np.zeros((count * num_samples, 3))
    for i in range(num_samples):
        x, xadd, h2 = 0.0, 1.0, i + 1
        while h2:
            xadd *= 0.5
            if h2 & 1:
                x += xadd
            h2 >>= 1
        y, yadd, h3 = 0.0, 1.0, i + 1
        while h3:
            yadd *= 1.0 / 3.0
            y += (h3 % 3) * yadd
            h3 //= 3
        ang = 2.0 * np.pi * y
        rr = np.sqrt(x)
        sx, sy = rr * np.cos(ang), rr * np.sin(ang)
        sz = np.sqrt(max(1.0 - sx * sx - sy * sy, 0.0))
        v = sx * t0 + sy * t1 + sz * n
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        out_d[i::num_samples] = v
    tmax = np.repeat(np.where(tri == -1, -1.0, max_dist), num_samples)
    return out_o, out_d, tmax


def shadow_rays(in_rays, in_results, num_samples, light_pos, light_radius, kernel_seed, first=0, count=None, f32_wrap=False):
    """rayGenShadowKernel (src/rt/ray/RayGenKernels.cu:240-301) in float64: (origins, unit directions, tmax) of count * num_samples rays.
    f32_wrap: decide the `>= 1.0f` wrap of the shifted sample (:281-283) on the kernel's float32 sum, not on the float64 one."""
    count = in_rays.shape[0] - first if count is None else count
    r = in_rays[first:first + count]
    res = in_results[first:first + count]
    o = np.stack([r["ox"], r["oy"], r["oz"]], 1).astype(np.float64)
    d = np.stack([r["dx"], r["dy"], r["dz"]], 1).astype(np.float64)
    back = np.maximum(res["t"].astype(np.float64) - 1.0e-2, 0.0)
    origin = o + d * back[:, None]
    M = np.uint32
    with np.errstate(over="ignore"):
        a = (M(kernel_seed) + np.arange(count, dtype=np.uint32)).astype(np.uint32)
    b = np.full(count, 0x9e3779b9, dtype=np.uint32)
    c = np.full(count, 0x9e3779b9, dtype=np.uint32)
    a, b, c = _jenkins(a, b, c)
    a, b, c = _jenkins(a, b, c)
    off = np.stack([a, b, c], 1).astype(np.float32).astype(np.float64) * 2.0 ** -32    # (F32)hash * exp2(-32)
    ro = np.zeros((count, num_samples, 3))
    rd = np.zeros((count, num_samples, 3))
    rt = np.zeros((count, num_samples))
    lp = np.asarray(light_pos, dtype=np.float64)
    for i in range(num_samples):
        r1, r2, v1, v2, k = 0, 0, 1 << 31, 3 << 30, i
        while k:
            if k & 1:
                r1 ^= v1
                r2 ^= (v2 << 1) & 0xFFFFFFFF
            v1 |= v1 >> 1
            v2 ^= v2 >> 1
            k >>= 1
        pos = np.array([float(np.float32(r1)) * 2.0 ** -32, float(np.float32(r2)) * 2.0 ** -32, (i + 0.5) / num_samples])[None, :] + off
        if f32_wrap:
            F = np.float32
            s32 = np.array([F(r1) * F(2.0 ** -32), F(r2) * F(2.0 ** -32), (F(i) + F(0.5)) / F(num_samples)], dtype=F)[None, :]
            wrap = (s32 + off.astype(F)).astype(F) >= F(1.0)
        else:
            wrap = pos >= 1.0
        pos = np.where(wrap, pos - 1.0, pos)
        pos = pos * 2.0 - 1.0
        direction = lp[None, :] + light_radius * pos - origin
        length = np.linalg.norm(direction, axis=1)
        ro[:, i] = origin
        rd[:, i] = direction / length[:, None]
        rt[:, i] = np.where(res["id"] == -1, -1.0, length)
    return ro.reshape(-1, 3), rd.reshape(-1, 3), rt.reshape(-1)
