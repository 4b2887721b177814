"""The bloom pass and the bloomed display (include/rsrt_bloom.h) restated in numpy, float32 operation for operation and in the
header's order, vectorised with clamped index arrays: the prefilter, the 13-tap downsample in its plain and its Karis form, the tent,
the doubling, the chain and the display pixel.  The CPU evaluation of the header (tests/test_bloom.py) and the GPU kernels
(tests/test_bloom_gpu.py) both equal it bit for bit."""
import numpy as np

F = np.float32
KARIS = 1
MAX_LEVELS = 8
CLAMP = F(65504.0)
DEFAULTS = {"levels": 6, "flags": KARIS, "threshold": 1.0, "intensity": 0.1}


def cl(i, n):
    return np.clip(i, 0, n - 1)


def lum(p):
    return ((F(0.2126) * p[..., 0] + F(0.7152) * p[..., 1]) + F(0.0722) * p[..., 2]).astype(F)


def level_size(n, k):
    for _ in range(k):
        n = (n + 1) // 2
    return n


def params_ok(levels, flags, threshold):
    t = F(threshold)
    return bool(1 <= levels <= MAX_LEVELS and (flags & ~KARIS) == 0 and np.isfinite(t) and t >= 0)


def exposed(sums, total, exposure):
    """p of the prefilter: [h, w, 3] float32, clamped to [0, 65504], NaN and negatives 0."""
    with np.errstate(all="ignore"):
        p = ((np.asarray(sums, F)[..., :3] / F(total)).astype(F) * F(exposure)).astype(F)
        p = np.where(p >= 0, p, F(0))
        return np.where(p > CLAMP, CLAMP, p).astype(F)


def prefilter(sums, total, exposure, threshold):
    """D_0: [h, w, 3] float32 from sums [h, w, >=3]."""
    p = exposed(sums, total, exposure)
    with np.errstate(all="ignore"):
        L = lum(p)
        t = F(threshold)
        s = np.where(L > t, ((L - t) / L).astype(F), F(0)).astype(F)
        return (p * s[..., None]).astype(F)


def box(a, b, c, d):
    return (((a + b) + (c + d)) * F(0.25)).astype(F)


def down(src, karis):
    """D_k [ceil(h/2), ceil(w/2), 3] from D_{k-1} [h, w, 3]."""
    h, w = src.shape[:2]
    x, y = np.arange((w + 1) // 2), np.arange((h + 1) // 2)
    taps = {}

    def tap(ox, oy):
        if (ox, oy) not in taps:
            x0, x1, y0, y1 = cl(2 * x + ox, w), cl(2 * x + ox + 1, w), cl(2 * y + oy, h)[:, None], cl(2 * y + oy + 1, h)[:, None]
            taps[ox, oy] = box(src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1])
        return taps[ox, oy]

    def grp(ox, oy):
        return box(tap(ox, oy), tap(ox + 2, oy), tap(ox, oy + 2), tap(ox + 2, oy + 2))
    gc, g = grp(-1, -1), [grp(-2, -2), grp(0, -2), grp(-2, 0), grp(0, 0)]
    if not karis:
        return (gc * F(0.5) + ((g[0] + g[1]) + (g[2] + g[3])) * F(0.125)).astype(F)
    kw = lambda q: (F(1) / (F(1) + lum(q))).astype(F)[..., None]  # noqa: E731
    wc, wi = kw(gc) * F(0.5), [kw(q) * F(0.125) for q in g]
    num = gc * wc + ((g[0] * wi[0] + g[1] * wi[1]) + (g[2] * wi[2] + g[3] * wi[3]))
    den = wc + ((wi[0] + wi[1]) + (wi[2] + wi[3]))
    return (num / den).astype(F)


def tent(u):
    h, w = u.shape[:2]
    x, y = np.arange(w), np.arange(h)
    c = lambda dx, dy: u[cl(y + dy, h)[:, None], cl(x + dx, w)]  # noqa: E731
    return ((((c(-1, -1) + c(1, -1)) + (c(-1, 1) + c(1, 1))) * F(0.0625) + ((c(0, -1) + c(0, 1)) + (c(-1, 0) + c(1, 0))) * F(0.125))
            + c(0, 0) * F(0.25)).astype(F)


def up(t, H, W):
    """The coarse image t [h, w, 3] doubled to [H, W, 3]."""
    h, w = t.shape[:2]

    def axis(n, m):
        i = np.arange(n)
        i0 = (i + 1) // 2 - 1
        w0 = np.where(i & 1, F(0.75), F(0.25)).astype(F)
        return cl(i0, m), cl(i0 + 1, m), w0, (F(1) - w0).astype(F)
    xa, xb, wx0, wx1 = axis(W, w)
    ya, yb, wy0, wy1 = axis(H, h)
    ya, yb, wx0, wx1 = ya[:, None], yb[:, None], wx0[None, :, None], wx1[None, :, None]
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    return ((t[ya, xa] * wx0 + t[ya, xb] * wx1) * wy0 + (t[yb, xa] * wx0 + t[yb, xb] * wx1) * wy1).astype(F)


def bloom(sums, total, exposure, levels=DEFAULTS["levels"], threshold=DEFAULTS["threshold"], karis=True):
    """B: [ceil(h/2), ceil(w/2), 4] float32 (alpha 1, as rsrt_bloom_download returns it) of sums [h, w, >=3]."""
    assert params_ok(levels, KARIS if karis else 0, threshold)
    with np.errstate(all="ignore"):
        d = [prefilter(sums, total, exposure, threshold)]
        for k in range(1, levels + 1):
            d.append(down(d[-1], karis and k == 1))
        u = d[levels]
        for k in range(levels - 1, 0, -1):
            u = (d[k] + up(tent(u), *d[k].shape[:2])).astype(F)
        b = (tent(u) * (F(1) / F(levels))).astype(F)
    return np.concatenate([b, np.ones(b.shape[:2] + (1,), F)], axis=-1)


def tone_map_encode(hdr):
    """rsrt_aces_tone_map and rsrt_srgb8_encode of hdr [h, w, 3]: [h, w, 4] uint8, alpha 255 (exposure_ref.display's second half)."""
    import test_display
    f = F
    with np.errstate(all="ignore"):
        m1 = np.array([[0.59719, 0.07600, 0.02840], [0.35458, 0.90834, 0.13383], [0.04823, 0.01566, 0.83777]], F)  # columns
        m2 = np.array([[1.60475, -0.10208, -0.00327], [-0.53108, 1.10813, -0.07276], [-0.07367, -0.00605, 1.07602]], F)

        def mul(m, v):
            return (m[0] * v[..., 0:1] + m[1] * v[..., 1:2]) + m[2] * v[..., 2:3]
        v = mul(m1, hdr)
        a = v * (v + f(0.0245786)) - f(0.000090537)
        b = v * (f(0.983729) * v + f(0.4329510)) + f(0.238081)
        r = mul(m2, a / b)
        sdr = np.minimum(np.maximum(r, f(0)), f(1))
        sdr = np.where(np.isnan(r), f(0), sdr)
        sdr[(hdr < 0).any(axis=-1)] = F([1, 0, 1])
    codes = np.searchsorted(test_display.srgb_thresholds(), sdr, side="right").astype(np.uint8)
    return np.concatenate([codes, np.full(codes.shape[:2] + (1,), 255, np.uint8)], axis=-1)


def display(sums, total, exposure, intensity, b):
    """rsrt_display_pixel_bloomed per pixel: [h, w, 4] uint8 from sums [h, w, >=3] and the bloom image b [ceil(h/2), ceil(w/2), >=3]."""
    h, w = sums.shape[:2]
    assert b.shape[:2] == ((h + 1) // 2, (w + 1) // 2)
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / F(total)).astype(np.float16).astype(F)
        hdr = (mean * F(exposure)).astype(F)
        hdr = (hdr + F(intensity) * up(np.asarray(b, F)[..., :3], h, w)).astype(F)
    return tone_map_encode(hdr)


def synthetic(h, w, seed, specials=True):
    """Sums [h, w, 4] float32 as an accumulator holds them (to be read with total 1 or 3): dim lognormal radiance with bright dots, a
    bright vertical edge and, where the frame has room, the special pixels — NaN, +inf, -inf, a negative, -0, a denormal, 3e38 and one
    whose mean rounds to >= 65520 in binary16.  Returns (sums, {name: flat pixel index})."""
    rng = np.random.default_rng(seed)
    s = np.empty((h, w, 4), F)
    s[..., :3] = np.exp(rng.normal(-1.5, 1.0, (h, w, 3))).astype(F)
    s[..., 3] = 1
    if w >= 4:
        s[:, (3 * w) // 4:, :3] *= F(40)  # the edge
    n = h * w
    flat = s.reshape(-1, 4)
    for i in rng.choice(n, size=max(1, n // 40), replace=False):  # the dots
        flat[i, :3] = np.exp(rng.normal(6.0, 2.0, 3)).astype(F)
    special = {}
    if specials and n >= 16:
        names = ["nan", "inf", "neg_inf", "negative", "neg_zero", "denormal", "huge", "f16_overflow"]
        special = {k: int(i) for k, i in zip(names, rng.choice(n, size=len(names), replace=False))}
        flat[special["nan"], 1] = np.nan
        flat[special["inf"], 2] = np.inf
        flat[special["neg_inf"], 0] = -np.inf
        flat[special["negative"], :3] = (-3.0, 0.5, -0.25)
        flat[special["neg_zero"], :3] = -0.0
        flat[special["denormal"], :3] = 1e-41
        flat[special["huge"], :3] = 3e38
        flat[special["f16_overflow"], :3] = (65519.0, 65520.0, 3 * 65530.0)
    return s, special
