"""numpy float32 restatement of the variance guidance for the tests: the temporal pass's luminance moments (include/rsrt_temporal.h,
RSRT_TEMPORAL_MOMENTS) and the variance-guided filter with the firefly clamp (include/rsrt_variance.h, RSRT_DENOISE_VARIANCE /
RSRT_DENOISE_CLAMP).  Every step is one IEEE binary32 operation in the order the C code performs it, so the results are compared bit
for bit.  The camera mapping, the colour's pass and the fixed filter's constants come from temporal_ref and denoise_ref."""
import numpy as np

import denoise_ref
import temporal_ref as T

F = np.float32
MIN_FRAMES = F(4.0)
EPS = F(1.0e-6)
SIGMA_L = 4.0  # sigma_color's default under VARIANCE
RADIUS = 3


def lum(x):
    x = np.asarray(x, np.float32)
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def albedo(aov, aov_total):
    aov = np.asarray(aov, np.float32)
    Tn = F(aov_total)
    return (aov[..., :3] + (Tn - aov[..., 3])[..., None]) / Tn


def prepare(sums, aov, S, Tn, demodulate=True):
    """rsrt_dn_prepare: the filter's input r [H, W, 3]."""
    c = np.asarray(sums, np.float32)[..., :3] / F(S)
    if not demodulate:
        return c
    a = albedo(aov, Tn)
    return c / np.where(a < denoise_ref.ALBEDO_EPS, denoise_ref.ALBEDO_EPS, a)


# -------------------------------------------------------------------------------------------------- temporal moments
def reproject_moments(aov, S, Tn, cam, prev_cam, prev_col, prev_feat, prev_mom, max_history=32, depth_tolerance=0.05, normal_tolerance=0.9):
    """The moment history as rsrt_tp_pixel_m gathers it: the colour's taps, validity and wsum over the previous records.
    -> hm [H, W, 3] (mu1, mu2, frames), nh [H, W], used [H, W]."""
    H, W = np.asarray(aov).shape[:2]
    sums0 = np.zeros((H, W, 4), np.float32)
    _, f, surface = T.current(sums0, aov, S, Tn)
    hm = np.zeros((H, W, 3), np.float32)
    nh = np.zeros((H, W), np.float32)
    used = np.zeros((H, W), bool)
    if prev_cam is None:
        return hm, nh, used
    pc, pf, pm = (np.asarray(x, np.float32) for x in (prev_col, prev_feat, prev_mom))
    if cam.same(prev_cam):
        return pm[..., :3].copy(), pc[..., 3].copy(), np.ones((H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W]
    d = T.center_ray(cam, W, H, xs, ys)
    X = cam.pos + f[..., 3:4] * d
    e = np.where(surface[..., None], X - prev_cam.pos, d)
    fx, fy, front = T.project(prev_cam, W, H, e)
    go = front & (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
    fx, fy = np.where(go, fx, F(0)), np.where(go, fy, F(0))
    flx, fly = np.floor(fx), np.floor(fy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    ax, ay = fx - flx, fy - fly
    one = F(1.0)
    tw = [(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]
    tol = F(depth_tolerance) * f[..., 3]
    wsum = np.zeros((H, W), np.float32)
    acc = np.zeros((H, W, 3), np.float32)
    accn = np.zeros((H, W), np.float32)
    for t in range(4):
        qx, qy = x0 + (t & 1), y0 + (t >> 1)
        inside = go & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        hq, fq, mq = pc[cy, cx], pf[cy, cx], pm[cy, cx]
        ok = inside & (hq[..., 3] > 0) & ((fq[..., 3] >= 0) == surface)
        dq = T.center_ray(prev_cam, W, H, cx, cy)
        eq = (prev_cam.pos + fq[..., 3:4] * dq) - X
        with np.errstate(all="ignore"):
            pd = T.dot(f, eq)
            ok &= ~(surface & ~(np.abs(pd) <= tol))
            ok &= ~(surface & ~(T.dot(f, fq) >= F(normal_tolerance)))
        wsum = np.where(ok, wsum + tw[t], wsum)
        accn = np.where(ok, accn + tw[t] * hq[..., 3], accn)
        acc = np.where(ok[..., None], acc + tw[t][..., None] * mq[..., :3], acc)
    used = go & (wsum >= T.MIN_WEIGHT)
    with np.errstate(all="ignore"):
        hh = acc / wsum[..., None]
        nn = accn / wsum
    nn = np.where(nn > F(max_history), F(max_history), nn)
    return np.where(used[..., None], hh, F(0)), np.where(used, nn, F(0)), used


def blend_moments(l, hm, nh, used, S):
    """The new record (mu1, mu2, frames, scale) [H, W, 4]."""
    Sf = F(S)
    l2 = l * l
    out = np.empty(l.shape + (4,), np.float32)
    with np.errstate(all="ignore"):
        out[..., 0] = np.where(used, (hm[..., 0] * nh + l * Sf) / (nh + Sf), l)
        out[..., 1] = np.where(used, (hm[..., 1] * nh + l2 * Sf) / (nh + Sf), l2)
        out[..., 2] = np.where(used, hm[..., 2] + F(1.0), F(1.0))
        out[..., 3] = np.where(used, Sf / (nh + Sf), F(1.0))
    return out


class MomentSequence:
    """The pass with and without RSRT_TEMPORAL_MOMENTS over frames, as the library keeps it: history, features, moment records, camera
    and whether the last frame carried moments (a toggle drops the history)."""

    def __init__(self, **params):
        self.params = params
        self.reset()

    def reset(self):
        self.cam = self.col = self.feat = self.mom = None
        self.moments = False

    def frame(self, sums, aov, S, Tn, cam, moments=True):
        prev = self.cam if self.cam is not None and self.moments == moments else None
        col, f, code = T.temporal(sums, aov, S, Tn, cam, prev, self.col, self.feat, **self.params)
        mom = None
        if moments:
            l = lum(prepare(sums, aov, S, Tn))
            hm, nh, used = reproject_moments(aov, S, Tn, cam, prev, self.col, self.feat, self.mom, **self.params)
            mom = blend_moments(l, hm, nh, used, S)
        self.cam, self.col, self.feat, self.mom, self.moments = cam, col, f, mom, moments
        return col, mom, code


# -------------------------------------------------------------------------------------------------- filter
def _shift(a, dy, dx, fill=0.0):
    """a[y + dy, x + dx] where that lies inside, `fill` elsewhere; and the mask of inside."""
    H, W = a.shape[:2]
    out = np.full(a.shape, fill, a.dtype)
    m = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m[y0:y1, x0:x1] = True
    return out, m


def clamp(r):
    """The firefly clamp of r [H, W, 3]."""
    l = lum(r)
    lmax = np.zeros(l.shape, np.float32)
    have = np.zeros(l.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            lq, m = _shift(l, dy, dx)
            lmax = np.where(m & (lq > lmax), lq, lmax)
            have |= m
    hit = have & (l > lmax)
    with np.errstate(all="ignore"):
        s = lmax / l
        return np.where(hit[..., None], r * s[..., None], r), hit


def variance(m, f, sigma_n, sigma_z):
    """v [H, W] from the moment records m [H, W, 4] and the packed features f [H, W, 4]."""
    sn, sz = F(sigma_n), F(sigma_z)
    kn = F(1.0) / (sn * sn)
    zp = f[..., 3]
    kz = F(1.0) / ((sz * sz) * (zp * zp + denoise_ref.DEPTH_EPS))
    acc = np.zeros(m.shape[:2] + (3,), np.float32)
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            fq, ok = _shift(f, dy, dx)
            mq, _ = _shift(m, dy, dx)
            nd = fq[..., :3] - f[..., :3]
            zd = fq[..., 3] - f[..., 3]
            dn = F(1.0) + ((nd[..., 0] * nd[..., 0] + nd[..., 1] * nd[..., 1]) + nd[..., 2] * nd[..., 2]) * kn
            dz = F(1.0) + (zd * zd) * kz
            w = F(1.0) / (dn * dz)
            new = np.stack([acc[..., 0] + w * mq[..., 0], acc[..., 1] + w * mq[..., 1], acc[..., 2] + w], axis=-1)
            acc = np.where(ok[..., None], new, acc)
    temporal = m[..., 2] >= MIN_FRAMES
    mu1 = np.where(temporal, m[..., 0], acc[..., 0] / acc[..., 2])
    mu2 = np.where(temporal, m[..., 1], acc[..., 1] / acc[..., 2])
    d = mu2 - mu1 * mu1
    return m[..., 3] * np.where(d > 0, d, F(0.0)), temporal


def _level(r, v, f, lvl, sigma_c, sigma_n, sigma_z, guided):
    """One level: the fixed filter's (rsrt_denoise.h) or the variance-guided one's.  -> r', v'."""
    sc, sn, sz = F(sigma_c), F(sigma_n), F(sigma_z)
    kn = F(1.0) / (sn * sn)
    zp = f[..., 3]
    kz = F(1.0) / ((sz * sz) * (zp * zp + denoise_ref.DEPTH_EPS))
    if guided:
        gs = np.zeros(v.shape, np.float32)
        gk = np.zeros(v.shape, np.float32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(v, dy, dx)
                k = F(2.0 if dx == 0 else 1.0) * F(2.0 if dy == 0 else 1.0)
                gs, gk = np.where(ok, gs + k * vq, gs), np.where(ok, gk + k, gk)
        kl = F(1.0) / ((sc * sc) * (gs / gk) + EPS)
        lp = lum(r)
    else:
        k4 = F(1.0)
        for _ in range(lvl):
            k4 = k4 * F(4.0)
        kc = k4 / (sc * sc)
    step = 1 << lvl
    acc = np.zeros(r.shape[:2] + (5,), np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            rq, ok = _shift(r, dy * step, dx * step)
            fq, _ = _shift(f, dy * step, dx * step)
            vq, _ = _shift(v, dy * step, dx * step)
            h = denoise_ref.B3[dx + 2] * denoise_ref.B3[dy + 2]
            nd = fq[..., :3] - f[..., :3]
            zd = fq[..., 3] - f[..., 3]
            if guided:
                dlum = lum(rq) - lp
                dc = F(1.0) + (dlum * dlum) * kl
            else:
                cd = rq - r
                dc = F(1.0) + ((cd[..., 0] * cd[..., 0] + cd[..., 1] * cd[..., 1]) + cd[..., 2] * cd[..., 2]) * kc
            dn = F(1.0) + ((nd[..., 0] * nd[..., 0] + nd[..., 1] * nd[..., 1]) + nd[..., 2] * nd[..., 2]) * kn
            dz = F(1.0) + (zd * zd) * kz
            w = h / ((dc * dn) * dz)
            new = np.concatenate([acc[..., :3] + w[..., None] * rq, (acc[..., 3] + w)[..., None], (acc[..., 4] + (w * w) * vq)[..., None]], axis=-1)
            acc = np.where(ok[..., None], new, acc)
    return acc[..., :3] / acc[..., 3:4], acc[..., 4] / (acc[..., 3] * acc[..., 3])


def denoise(sums, aov, sample_total, aov_total, iterations=5, sigma_color=None, sigma_normal=0.5, sigma_depth=0.3, demodulate=True,
            variance_guided=True, clamp_input=True, moments=None):
    """rsrt_denoise with RSRT_DENOISE_VARIANCE (variance_guided) and / or RSRT_DENOISE_CLAMP (clamp_input): sums [H, W, 4] (the
    accumulator, or the temporal colour with sample_total 1), aov [H, W, 8], moments [H, W, 4] (the temporal pass's records; None: from
    the input itself) -> [H, W, 3] f32."""
    if sigma_color is None:
        sigma_color = SIGMA_L if variance_guided else 2.0
    c = np.asarray(sums, np.float32)[..., :3] / F(sample_total)
    if iterations == 0:
        return c
    assert demodulate or not variance_guided
    r = prepare(sums, aov, sample_total, aov_total, demodulate)
    f = denoise_ref.features(aov, aov_total)
    l = lum(r)
    if clamp_input:
        r, _ = clamp(r)
    v = np.zeros(r.shape[:2], np.float32)
    if variance_guided:
        m = np.asarray(moments, np.float32) if moments is not None else np.stack([l, l * l, np.ones_like(l), np.ones_like(l)], axis=-1)
        v, _ = variance(m, f, sigma_normal, sigma_depth)
    for lvl in range(iterations):
        r, v = _level(r, v, f, lvl, sigma_color, sigma_normal, sigma_depth, variance_guided)
    return r * albedo(aov, aov_total) if demodulate else r
