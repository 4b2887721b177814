"""numpy float32 restatement of the guided upsampling (include/rsrt_upsample.h, rsrt_upsample) for the tests, and a plain bilinear
baseline.  Every step of `upsample` is one IEEE binary32 operation in the order the C code performs it, so the results are compared
bit for bit."""
import numpy as np

import denoise_ref

F = np.float32
SIGMA_NORMAL, SIGMA_DEPTH = 0.5, 0.3


def coords(low_size, out_size):
    """rsrt_up_coord / rsrt_up_nearest of every output pixel along one axis: the low coordinate (f32) and its nearest low pixel."""
    u = (np.arange(out_size).astype(np.float32) * F(low_size)) / F(out_size)
    return u, np.floor(u + F(0.5)).astype(np.int64)


def low_pass(colour, aov, sample_total, aov_total, demodulate=True):
    """What rt_dn_prepare_kernel writes: r [h, w, 3] f32 (rsrt_dn_prepare) and the packed features [h, w, 4] (as f32)."""
    S, T = F(sample_total), F(aov_total)
    aov = np.asarray(aov, np.float32)
    c = np.ascontiguousarray(np.asarray(colour, np.float32)[..., :3]) / S
    miss = T - aov[..., 3]
    a = (aov[..., :3] + miss[..., None]) / T
    r = c / np.where(a < denoise_ref.ALBEDO_EPS, denoise_ref.ALBEDO_EPS, a) if demodulate else c
    with np.errstate(over="ignore"):
        return r, denoise_ref.features(aov, T)


def upsample(colour, aov, guide, sample_total, aov_total, guide_total, sigma_normal=SIGMA_NORMAL, sigma_depth=SIGMA_DEPTH, demodulate=True,
             return_fallback=False):
    """rsrt_upsample: colour [h, w, >=3] (a sum of sample_total samples), aov [h, w, 8], guide [H, W, 8] -> [H, W, 3] f32 (and, with
    return_fallback, the mask of the pixels that took the nearest low pixel's value)."""
    with np.errstate(over="ignore", invalid="ignore"):
        r, f = low_pass(colour, aov, sample_total, aov_total, demodulate)
        guide = np.asarray(guide, np.float32)
        Tg = F(guide_total)
        h, w = r.shape[:2]
        H, W = guide.shape[:2]
        fp = denoise_ref.features(guide, Tg)
        ap = (guide[..., :3] + (Tg - guide[..., 3])[..., None]) / Tg
        sn, sz = F(sigma_normal), F(sigma_depth)
        kn = F(1.0) / (sn * sn)
        zp = fp[..., 3]
        kz = F(1.0) / ((sz * sz) * (zp * zp + denoise_ref.DEPTH_EPS))
        u, xn = coords(w, W)
        v, yn = coords(h, H)
        acc = np.zeros((H, W, 4), np.float32)
        for dy in (-1, 0, 1):
            qy = yn + dy
            hy = F(1.0) - np.abs(qy.astype(np.float32) - v) * F(0.5)
            for dx in (-1, 0, 1):
                qx = xn + dx
                hx = F(1.0) - np.abs(qx.astype(np.float32) - u) * F(0.5)
                valid = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                iy, ix = np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]
                rq, fq = r[iy, ix], f[iy, ix]
                hs = hx[None, :] * hy[:, None]
                nd = fq[..., :3] - fp[..., :3]
                zd = fq[..., 3] - fp[..., 3]
                dn = F(1.0) + ((nd[..., 0] * nd[..., 0] + nd[..., 1] * nd[..., 1]) + nd[..., 2] * nd[..., 2]) * kn
                dz = F(1.0) + (zd * zd) * kz
                wt = hs / (dn * dz)
                new = np.concatenate([acc[..., :3] + wt[..., None] * rq, (acc[..., 3] + wt)[..., None]], axis=-1)
                acc = np.where(valid[..., None], new, acc)
        ok = acc[..., 3] > 0
        near = r[np.minimum(yn, h - 1)[:, None], np.minimum(xn, w - 1)[None, :]]
        res = np.where(ok[..., None], acc[..., :3] / acc[..., 3:4], near)
        out = res * ap if demodulate else res
    return (out, ~ok) if return_fallback else out


def bilinear(img, out_h, out_w):
    """The plain baseline: f64 bilinear interpolation of img [h, w, C] at u = X * w / W, taps floor(u) and min(floor(u) + 1, w - 1)."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    u, v = np.arange(out_w) * w / out_w, np.arange(out_h) * h / out_h
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = (u - x0)[None, :, None], (v - y0)[:, None, None]
    top = img[y0[:, None], x0[None, :]] * (1 - tx) + img[y0[:, None], x1[None, :]] * tx
    bot = img[y1[:, None], x0[None, :]] * (1 - tx) + img[y1[:, None], x1[None, :]] * tx
    return top * (1 - ty) + bot * ty
