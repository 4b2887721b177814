"""The fog rebuild (include/rsrt_fog_upsample.h, rsrt_fog_apply_upsampled) restated in numpy: the demodulated low records, the output
pixel's transmittance from its first-hit record, the nine-tap tent and the compose step, in float32, operation for operation and in the
header's order.  The coordinates are upsample_ref's, the transmittance and the compose step fog_ref's.  The CPU evaluation of the
header (tests/test_fog_upsample.py, tests/cpp/fog_upsample_host.cpp) and the HIP kernels (tests/test_fog_upsample_gpu.py) equal it bit
for bit.  `tent_raw` is the baseline without the demodulation, in float64."""
import numpy as np

import fog_ref
import upsample_ref

F = np.float32
SOURCE_MAX = F(2.0 ** 120)


def source(rec, n):
    """rsrt_fogup_source: rec [..., 4] of n samples -> s [..., 3]."""
    with np.errstate(all="ignore"):
        m = (np.asarray(rec, F) / F(n)).astype(F)
        one = (F(1) - m[..., 3]).astype(F)
        q = (m[..., :3] / one[..., None]).astype(F)
        q = np.where(q < SOURCE_MAX, q, SOURCE_MAX)
        return np.where((one > 0)[..., None], q, F(0)).astype(F)


def tau(k, g, T):
    """rsrt_fogup_tau: g [..., 8] first-hit records of T samples -> [...]."""
    g, T = np.asarray(g, F), F(T)
    with np.errstate(all="ignore"):
        e_far = fog_ref.transmittance(k, k["max_distance"])
        hits = g[..., 3]
        d = (g[..., 7] / hits).astype(F)
        e_hit = fog_ref.transmittance(k, fog_ref.segment(k, np.ones(hits.shape, bool), d))
        mixed = (((hits * e_hit).astype(F) + ((T - hits).astype(F) * e_far).astype(F)).astype(F) / T).astype(F)
        return np.where(hits > 0, np.where(hits >= T, e_hit, mixed), e_far).astype(F)


def gather(s, H, W):
    """The nine taps: s [h, w, 3] -> acc [H, W, 4] (sums of hs * s_q, sum of hs)."""
    s = np.asarray(s, F)
    h, w = s.shape[:2]
    u, xn = upsample_ref.coords(w, W)
    v, yn = upsample_ref.coords(h, H)
    acc = np.zeros((H, W, 4), F)
    for dy in (-1, 0, 1):
        qy = yn + dy
        hy = (F(1) - (np.abs((qy.astype(F) - v).astype(F)) * F(0.5)).astype(F)).astype(F)
        for dx in (-1, 0, 1):
            qx = xn + dx
            hx = (F(1) - (np.abs((qx.astype(F) - u).astype(F)) * F(0.5)).astype(F)).astype(F)
            valid = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            sq = s[np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]]
            hs = (hx[None, :] * hy[:, None]).astype(F)
            new = np.concatenate([(acc[..., :3] + (hs[..., None] * sq).astype(F)).astype(F), (acc[..., 3] + hs).astype(F)[..., None]], axis=-1)
            acc = np.where(valid[..., None], new, acc).astype(F)
    return acc


def inscatter(acc, t):
    """S * (1 - tau): [H, W, 3]."""
    S = (acc[..., :3] / acc[..., 3:4]).astype(F)
    return (S * (F(1) - np.asarray(t, F)).astype(F)[..., None]).astype(F)


def rebuild(colour, rec, n, g, T, k):
    """rsrt_fog_apply_upsampled: colour [H, W, 3] (already divided by its sample total), rec [h, w, 4] of n fog samples, g [H, W, 8] of T
    samples, k fog_ref.prepare's -> ([H, W, 4] alpha 1, the record (I, tau) [H, W, 4] that was composed)."""
    g = np.asarray(g, F)
    H, W = g.shape[:2]
    t = tau(k, g, T)
    r = np.concatenate([inscatter(gather(source(rec, n), H, W), t), t[..., None]], axis=-1).astype(F)
    return fog_ref.compose(colour, r, 1), r


def tent_raw(rec, n, H, W):
    """The baseline: the same nine-tap tent over the mean records as they are (no demodulation, no first hit), float64 -> [H, W, 4]."""
    m = np.asarray(rec, np.float64) / n
    h, w = m.shape[:2]
    u, xn = upsample_ref.coords(w, W)
    v, yn = upsample_ref.coords(h, H)
    u, v = u.astype(np.float64), v.astype(np.float64)
    acc, wt = np.zeros((H, W, 4)), np.zeros((H, W))
    for dy in (-1, 0, 1):
        qy = yn + dy
        hy = 1 - np.abs(qy - v) / 2
        for dx in (-1, 0, 1):
            qx = xn + dx
            hx = 1 - np.abs(qx - u) / 2
            valid = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            hs = np.where(valid, hx[None, :] * hy[:, None], 0.0)
            acc += hs[..., None] * m[np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]]
            wt += hs
    return acc / wt[..., None]
