"""The auto-exposure meter and the exposed display (include/rsrt_exposure.h) restated in numpy: a pixel's luminance in float32,
operation for operation, its histogram word from the float's bit pattern, the exposure of a histogram in Python integers, and the
exposed display pixel over test_display's restatement of the display transform.  The CPU evaluation of the header
(tests/test_exposure.py) and the GPU kernels (tests/test_exposure_gpu.py) both equal it bit for bit."""
import numpy as np

F = np.float32
LO = 888
BINS = 256
WORDS = 257
DEFAULTS = {"low_permille": 100, "high_permille": 950, "key": 0.18, "min_exposure": 2.0 ** -16, "max_exposure": 2.0 ** 16, "blend": 1.0,
            "previous_exposure": 0.0}


def luminance(sums, total):
    """[...] float32 from sums [..., >=3]: c = sum / total per channel, (0.2126 r + 0.7152 g) + 0.0722 b."""
    with np.errstate(all="ignore"):
        c = np.asarray(sums, F)[..., :3] / F(total)
        return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def words(lum):
    """The histogram word of every luminance: its bin, or 256 for !(L > 0)."""
    lum = np.asarray(lum, F)
    with np.errstate(all="ignore"):
        metered = lum > 0
    b = (lum.view(np.uint32) >> 20).astype(np.int64)
    return np.where(metered, np.clip(b, LO, LO + 255) - LO, BINS)


def histogram(sums, total):
    """257 uint32 words of an image of sums [..., >=3]."""
    return np.bincount(words(luminance(sums, total)).ravel(), minlength=WORDS).astype(np.uint32)


def params_ok(low_permille, high_permille, key, min_exposure, max_exposure, blend, previous_exposure):
    pos = lambda x: bool(np.isfinite(F(x)) and F(x) > 0)  # noqa: E731
    return bool(low_permille < high_permille <= 1000 and pos(key) and pos(min_exposure) and pos(max_exposure)
                and F(min_exposure) <= F(max_exposure) and F(0) <= F(blend) <= F(1) and (F(previous_exposure) == 0 or pos(previous_exposure)))


def from_histogram(hist, **params):
    """rsrt_exposure_from_histogram: dict of exposure, target, average_luminance (float32), metered, skipped."""
    q = dict(DEFAULTS, **params)
    assert params_ok(**q)
    h = [int(x) for x in hist]
    assert len(h) == WORDS
    n = sum(h[:BINS])
    prev, blend = F(q["previous_exposure"]), F(q["blend"])
    out = {"metered": n, "skipped": h[BINS]}
    if n == 0:
        e = prev if prev > 0 else F(1)
        out.update(average_luminance=F(0), target=e, exposure=e)
        return out
    a, b = n * q["low_permille"] // 1000, (n * q["high_permille"] + 999) // 1000
    s = cum = 0
    for i in range(BINS):
        lo, hi = max(cum, a), min(cum + h[i], b)
        if hi > lo:
            s += i * (hi - lo)
        cum += h[i]
    bits_avg = (LO << 20) + (1 << 19) + (s << 20) // (b - a)
    avg = np.array([bits_avg], np.uint32).view(F)[0]
    with np.errstate(all="ignore"):
        target = F(F(q["key"]) / avg)
        lo_e, hi_e = F(q["min_exposure"]), F(q["max_exposure"])
        target = lo_e if target < lo_e else (hi_e if hi_e < target else target)
        exposure = F(prev + F(F(target - prev) * blend)) if prev > 0 else target
    out.update(average_luminance=avg, target=target, exposure=exposure)
    return out


def display(sums, total, exposure):
    """rsrt_display_pixel_exposed per pixel: [H, W, 4] uint8 (alpha 255) from sums [H, W, >=3] — test_display.display_numpy with
    the exposure multiplied in after the binary16 rounding."""
    import test_display
    f = F
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / f(total)).astype(np.float16).astype(F)
        hdr = (mean * f(exposure)).astype(F)
        m1 = np.array([[0.59719, 0.07600, 0.02840], [0.35458, 0.90834, 0.13383], [0.04823, 0.01566, 0.83777]], F)  # columns
        m2 = np.array([[1.60475, -0.10208, -0.00327], [-0.53108, 1.10813, -0.07276], [-0.07367, -0.00605, 1.07602]], F)

        def mul(m, v):  # (c0*v0 + c1*v1) + c2*v2, one rounded f32 op at a time
            return (m[0] * v[..., 0:1] + m[1] * v[..., 1:2]) + m[2] * v[..., 2:3]
        v = mul(m1, hdr)
        a = v * (v + f(0.0245786)) - f(0.000090537)
        b = v * (f(0.983729) * v + f(0.4329510)) + f(0.238081)
        r = mul(m2, a / b)
        sdr = np.minimum(np.maximum(r, f(0)), f(1))
        sdr = np.where(np.isnan(r), f(0), sdr)  # clamp as compare-selects: NaN < 0 false, 1 < NaN false -> NaN -> code 0
        sdr[(hdr < 0).any(axis=-1)] = F([1, 0, 1])
    codes = np.searchsorted(test_display.srgb_thresholds(), sdr, side="right").astype(np.uint8)
    return np.concatenate([codes, np.full(codes.shape[:2] + (1,), 255, np.uint8)], axis=-1)


def synthetic(h, w, seed, sigma=1.5):
    """Sums [h, w, 4] float32 as an accumulator holds them: lognormal radiance with, where the frame has room, the special pixels —
    an exact zero, a negative channel with positive luminance, an all-negative pixel, a NaN, a +inf, 1e-30 and 1e30.  Returns
    (sums, {name: flat pixel index})."""
    rng = np.random.default_rng(seed)
    s = np.empty((h, w, 4), F)
    s[..., :3] = np.exp(rng.normal(-1.0, sigma, (h, w, 3))).astype(F)
    s[..., 3] = 1
    flat = s.reshape(-1, 4)
    n = h * w
    special = {}
    if n >= 16:
        special = {"zero": n // 7, "negative_channel": n // 5, "negative": n // 4, "nan": n // 3, "inf": n // 2, "tiny": n - 2, "huge": n - 1}
        flat[special["zero"], :3] = 0
        flat[special["negative_channel"], :3] = (-0.5, 2.0, 0.25)
        flat[special["negative"], :3] = (-3.0, -0.5, -0.25)
        flat[special["nan"], 1] = np.nan
        flat[special["inf"], 2] = np.inf
        flat[special["tiny"], :3] = 1e-30
        flat[special["huge"], :3] = 1e30
    return s, special
