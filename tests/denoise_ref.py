"""numpy float32 restatements of the denoiser (include/rsrt_denoise.h, rsrt_aov_render) for the tests: the filter, the camera
rays of a (pixel, sample), and the AOV records built from the checker's closest hits.  Every step is one IEEE binary32 operation
in the order the C code performs it, so the results are compared bit for bit."""
import numpy as np

import oracle

F = np.float32
B3 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)
ALBEDO_EPS = F(1.0e-3)
DEPTH_EPS = F(1.0e-4)
DEPTH_MAX = F(65504.0)  # the largest finite binary16: the packed mean distance saturates here


def fma32(a, b, c):
    """f32 fma (one rounding) from f64: the product of two f32 is exact in f64, the sum is rounded to odd (TwoSum tells whether it
    was exact), and rounding that to f32 is then the correctly rounded fma."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


# -------------------------------------------------------------------------------------------------- filter
def features(aov, aov_total):
    """rsrt_dn_features and their binary16 packing: mean normal xyz, mean distance saturated at DEPTH_MAX -> [H, W, 4] f32."""
    f = np.asarray(aov, np.float32)[..., 4:8] / F(aov_total)
    f[..., 3] = np.where(f[..., 3] > DEPTH_MAX, DEPTH_MAX, f[..., 3])
    return f.astype(np.float16).astype(np.float32)


def denoise(sums, aov, sample_total, aov_total, iterations=5, sigma_color=2.0, sigma_normal=0.5, sigma_depth=0.3, demodulate=True):
    """rsrt_denoise: sums [H, W, 4] (the accumulator), aov [H, W, 8] -> [H, W, 3] f32."""
    S, T = F(sample_total), F(aov_total)
    s = np.ascontiguousarray(sums[..., :3], np.float32)
    c = s / S
    if iterations == 0:
        return c
    aov = np.asarray(aov, np.float32)
    miss = T - aov[..., 3]
    a = (aov[..., :3] + miss[..., None]) / T
    f = features(aov, T)  # the packed binary16 features
    r = c / np.where(a < ALBEDO_EPS, ALBEDO_EPS, a) if demodulate else c
    sc, sn, sz = F(sigma_color), F(sigma_normal), F(sigma_depth)
    kn = F(1.0) / (sn * sn)
    zp = f[..., 3]
    kz = F(1.0) / ((sz * sz) * (zp * zp + DEPTH_EPS))
    H, W = r.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    for lvl in range(iterations):
        k4 = F(1.0)
        for _ in range(lvl):
            k4 = k4 * F(4.0)
        kc = k4 / (sc * sc)
        step = 1 << lvl
        pad = 2 * step
        rp_ = np.pad(r, ((pad, pad), (pad, pad), (0, 0)))
        fp_ = np.pad(f, ((pad, pad), (pad, pad), (0, 0)))
        acc = np.zeros((H, W, 4), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                valid = (ys + oy >= 0) & (ys + oy < H) & (xs + ox >= 0) & (xs + ox < W)
                rq = rp_[pad + oy:pad + oy + H, pad + ox:pad + ox + W]
                fq = fp_[pad + oy:pad + oy + H, pad + ox:pad + ox + W]
                h = B3[dx + 2] * B3[dy + 2]
                cd = rq - r
                nd = fq[..., :3] - f[..., :3]
                zd = fq[..., 3] - f[..., 3]
                dc = F(1.0) + ((cd[..., 0] * cd[..., 0] + cd[..., 1] * cd[..., 1]) + cd[..., 2] * cd[..., 2]) * kc
                dn = F(1.0) + ((nd[..., 0] * nd[..., 0] + nd[..., 1] * nd[..., 1]) + nd[..., 2] * nd[..., 2]) * kn
                dz = F(1.0) + (zd * zd) * kz
                w = h / ((dc * dn) * dz)
                new = np.concatenate([acc[..., :3] + w[..., None] * rq, (acc[..., 3] + w)[..., None]], axis=-1)
                acc = np.where(valid[..., None], new, acc)
        r = acc[..., :3] / acc[..., 3:4]
    return r * a if demodulate else r


# -------------------------------------------------------------------------------------------------- camera rays and AOV records
def _uniform(u):
    return np.array([oracle.lib().orc_u32_to_uniform(int(x)) for x in u], np.float32)


def camera_rays(cam, width, height, px, py, sample):
    """The camera ray of sample `sample` of pixels (px, py) (shader.wgsl:1305-1364, start_path): origins, directions [N, 3] f32.
    cam: a CAMERA record (pos, rot_transform columns, fov_y)."""
    import ctypes as C
    L = oracle.lib()
    px, py = np.asarray(px, np.uint32), np.asarray(py, np.uint32)
    u1, u2 = np.empty(px.size, np.uint32), np.empty(px.size, np.uint32)
    for i, pix in enumerate((py * np.uint32(width) + px).tolist()):
        s = C.c_uint32(oracle.rng_seed(pix, int(sample)))
        u1[i] = L.orc_rng_next_u32(C.byref(s))
        u2[i] = L.orc_rng_next_u32(C.byref(s))
    angle = (_uniform(u1) * F(2.0)) * F(3.1415926)
    cx = np.array([oracle.detmath("cos", float(x)) for x in angle], np.float32)
    cy = np.array([oracle.detmath("sin", float(x)) for x in angle], np.float32)
    rad = np.sqrt(_uniform(u2))
    fx, fy = px.astype(np.float32) + cx * rad, py.astype(np.float32) + cy * rad
    sx = ((fx / F(width)) * F(2.0) - F(1.0)) * F(1.0)
    sy = ((fy / F(height)) * F(2.0) - F(1.0)) * F(-1.0)
    fov = F(np.asarray(cam["fov_y"]).reshape(-1)[0])
    m = F(oracle.detmath("sin", float(fov / F(2.0))))
    aspect = F(width) / F(height)
    v = [(sx * m) * aspect, sy * m, np.full(px.size, F(-1.0))]
    rot = np.asarray(cam["rot_transform"], np.float32).reshape(3, 4)
    d = [fma32(rot[2, i], v[2], fma32(rot[1, i], v[1], rot[0, i] * v[0])) for i in range(3)]  # column-major mat3 * v
    dd = fma32(d[2], d[2], fma32(d[1], d[1], d[0] * d[0]))
    inv = F(1.0) / np.sqrt(dd)
    dirs = np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=-1)
    origins = np.broadcast_to(np.asarray(cam["pos"], np.float32).reshape(3), dirs.shape).copy()
    return origins, dirs


def aov_records(scene, oscene, cam, width, height, sample_begin, sample_count, aov=None):
    """What rsrt_aov_render adds for samples [sample_begin, sample_begin + sample_count): [H, W, 8] f32, starting from `aov`
    (zeros when None).  Hits from the checker's cast_ray (mode 0); material colours from the scene."""
    out = np.zeros((height, width, 8), np.float32) if aov is None else np.array(aov, np.float32)
    py, px = np.mgrid[0:height, 0:width]
    px, py = px.reshape(-1), py.reshape(-1)
    colors = np.asarray(scene.materials["color"], np.float32).reshape(-1, 3)
    flat = out.reshape(-1, 8)
    for k in range(sample_begin, sample_begin + sample_count):
        o, d = camera_rays(cam, width, height, px, py, k)
        hit = oracle.cast_rays(oscene, o, d, mode=0)
        m = hit["did_hit"] != 0
        col = colors[hit["material_id"][m]]
        flat[m, 0:3] = flat[m, 0:3] + col
        flat[m, 3] = flat[m, 3] + F(1.0)
        flat[m, 4:7] = flat[m, 4:7] + hit["normal"][m].astype(np.float32)
        flat[m, 7] = flat[m, 7] + hit["distance"][m].astype(np.float32)
    return out
