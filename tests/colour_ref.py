"""The white-balance meter, the colour LUT and the colour display (include/rsrt_colour.h) restated in numpy: a pixel's chroma bin from
its floats' bit patterns in int64, the white point of a histogram in Python integers up to the one float32 division, rsrt_colour_log2,
rsrt_colour_pow and the bake in float32, operation for operation and in the header's order, the tetrahedral interpolation with the
header's three compare-and-swaps, and the colour display pixel over bloom_ref's and local_ref's restatements.  The CPU evaluation of
the header (tests/test_colour.py) and the GPU kernels (tests/test_colour_gpu.py) both equal it bit for bit."""
import numpy as np

import bloom_ref
import local_ref

F = np.float32
AXIS = 64
BINS = 4096
WORDS = 4097
LOG2_K = 22700
WHITE_DEFAULTS = {"gate": 12, "iterations": 3, "min_permille": 50, "strength": 1.0, "max_stops": 2.0, "blend": 1.0, "previous": (0.0, 0.0, 0.0)}
CDL_DEFAULTS = {"slope": 1.0, "offset": 0.0, "power": 1.0, "saturation": 1.0}
LUT_SIZES = (2, 3, 17, 33, 65)
LOG2_L = (F(2.8853900818), F(0.9617966939), F(0.5770780164), F(0.4121985831), F(0.3205988980))
# the CDLs the tests bake: (slope, offset, power, saturation), a number or three a channel
CDLS = {"identity": (1.0, 0.0, 1.0, 1.0),
        "warm": ((1.1, 1.0, 0.85), (0.02, 0.0, -0.03), (0.9, 1.0, 1.2), 1.25),
        "crush": (1.4, -0.08, 2.2, 0.6),
        "lift": ((0.7, 0.8, 16.0), (0.3, 0.1, -1.0), (0.25, 4.0, 0.5), 0.0)}


def ilog2(x):
    """rsrt_colour_ilog2 of float32 x > 0 (of anything else: of its bits): int64, Q16."""
    b = np.asarray(x, F).view(np.uint32).astype(np.int64)
    e, m = (b >> 23) - 127, (b & 0x7fffff) >> 7
    return e * 65536 + m + ((m * (65536 - m) * LOG2_K) >> 32)


def words(sums, total):
    """rsrt_white_word per pixel of sums [..., >=3]: the bin vb * 64 + ub, or 4096."""
    with np.errstate(all="ignore"):
        c = (np.asarray(sums, F)[..., :3] / F(total)).astype(F)
        counted = (c > 0).all(axis=-1)
    lr, lg, lb = ilog2(c[..., 0]), ilog2(c[..., 1]), ilog2(c[..., 2])
    ub = np.clip(((lg - lr) >> 12) + 32, 0, 63)
    vb = np.clip(((lg - lb) >> 12) + 32, 0, 63)
    return np.where(counted, vb * AXIS + ub, BINS)


def histogram(sums, total):
    """4097 uint32 words of an image of sums [..., >=3]."""
    return np.bincount(words(sums, total).ravel(), minlength=WORDS).astype(np.uint32)


def white_params_ok(gate, iterations, min_permille, strength, max_stops, blend, previous, flags=0):
    p = [F(x) for x in previous]
    none, given = all(x == 0 for x in p), all(np.isfinite(x) and x > 0 for x in p)
    return bool(1 <= gate <= 31 and 0 <= iterations <= 8 and 0 <= min_permille <= 1000 and 0 <= F(strength) <= 1 and 0 <= F(max_stops) <= 4
                and 0 <= F(blend) <= 1 and (none or given) and flags == 0)


def window(h2, lo, hi):
    """N, Su, Sv over [lo[0], hi[0]] x [lo[1], hi[1]] of h2[vb][ub] (Python integers)."""
    n = su = sv = 0
    for vb in range(lo[1], hi[1] + 1):
        for ub in range(lo[0], hi[0] + 1):
            c = h2[vb][ub]
            n += c
            su += c * (2 * (ub - 32) + 1)
            sv += c * (2 * (vb - 32) + 1)
    return n, su, sv


def to_f32(i):
    """The correctly rounded float32 of an integer (one rounding, as the C conversion makes it)."""
    return np.array([i], np.int64).astype(F)[0]


def clampf(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def final_window(hist, **params):
    """The mean shift of rsrt_white_from_histogram: (N, Su, Sv) of the final window and its (lo, hi), in Python integers."""
    q = dict(WHITE_DEFAULTS, **params)
    assert white_params_ok(**q)
    h = [int(x) for x in hist]
    assert len(h) == WORDS
    h2 = [h[v * AXIS:(v + 1) * AXIS] for v in range(AXIS)]
    lo, hi = [1, 1], [62, 62]
    for _ in range(q["iterations"]):
        n, su, sv = window(h2, lo, hi)
        if n == 0:
            break
        for a, s in enumerate((su, sv)):
            centre = s // (2 * n) + 32  # (Python's // is a floor)
            lo[a], hi[a] = max(centre - q["gate"], 1), min(centre + q["gate"], 62)
    return window(h2, lo, hi), (tuple(lo), tuple(hi))


def from_histogram(hist, **params):
    """rsrt_white_from_histogram: dict of white, target, illuminant (float32 [3]), eu, ev (float32), gated, counted, skipped,
    estimated."""
    q = dict(WHITE_DEFAULTS, **params)
    (n, su, sv), _ = final_window(hist, **params)
    h = [int(x) for x in hist]
    total = sum(h)
    prev = np.array(q["previous"], F)
    given = bool((prev != 0).any())
    out = {"gated": n, "counted": total - h[BINS], "skipped": h[BINS]}
    if n == 0 or n * 1000 < q["min_permille"] * total:
        w = prev if given else np.ones(3, F)
        out.update(white=w.copy(), target=w.copy(), illuminant=np.ones(3, F), eu=F(0), ev=F(0), estimated=False)
        return out
    den = to_f32(32 * n)
    eu, ev = F(to_f32(su) / den), F(to_f32(sv) / den)
    s, m = F(q["strength"]), F(q["max_stops"])
    gr = local_ref.exp2(clampf(F(s * eu), -m, m))
    gb = local_ref.exp2(clampf(F(s * ev), -m, m))
    norm = F(F(F(F(0.2126) * gr) + F(0.7152)) + F(F(0.0722) * gb))
    target = np.array([gr / norm, F(1) / norm, gb / norm], F)
    blend = F(q["blend"])
    white = (prev + ((target - prev).astype(F) * blend).astype(F)).astype(F) if given else target
    out.update(white=white, target=target, illuminant=np.array([local_ref.exp2(-eu), F(1), local_ref.exp2(-ev)], F), eu=eu, ev=ev, estimated=True)
    return out


def cdl_params_ok(slope, offset, power, saturation, flags=0):
    three = lambda x: np.broadcast_to(np.asarray(x, F), (3,))  # noqa: E731
    with np.errstate(all="ignore"):
        return bool(((three(slope) >= 0) & (three(slope) <= 16)).all() and ((three(offset) >= -1) & (three(offset) <= 1)).all()
                    and ((three(power) >= 0.25) & (three(power) <= 4)).all() and 0 <= F(saturation) <= 4 and flags == 0)


def log2(x):
    """rsrt_colour_log2 of normal float32 x > 0."""
    b = np.asarray(x, F).view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - 127
    f = ((b & np.uint32(0x7fffff)) | np.uint32(0x3f800000)).view(F)
    big = f > F(1.41421354)
    f = np.where(big, (f * F(0.5)).astype(F), f).astype(F)
    e = np.where(big, e + 1, e)
    t = ((f - F(1)).astype(F) / (f + F(1)).astype(F)).astype(F)
    t2 = (t * t).astype(F)
    p = np.full(t.shape, LOG2_L[4], F)
    for c in (LOG2_L[3], LOG2_L[2], LOG2_L[1], LOG2_L[0]):
        p = ((p * t2).astype(F) + c).astype(F)
    return (e.astype(F) + (p * t).astype(F)).astype(F)


def pow_(x, p):
    """rsrt_colour_pow of float32 x in [0, 1] and a power in [0.25, 4]."""
    x = np.asarray(x, F)
    tiny = x < F(1.17549435e-38)
    e = (F(p) * log2(np.where(tiny, F(1), x))).astype(F)
    small = e < F(-64)
    return np.where(tiny | small, F(0), local_ref.exp2(np.where(small, F(0), e))).astype(F)


def clamp01(x):
    return np.where(x < 0, F(0), np.where(x > 1, F(1), x)).astype(F)


def pow_f64(x, p):
    """float64 pow of float32 x and the float32 power, rounded once to float32: what rsrt_colour_pow is measured against."""
    return (np.asarray(x, F).astype(np.float64) ** float(F(p))).astype(F)


def bake(n, slope=1.0, offset=0.0, power=1.0, saturation=1.0, pow_fn=None):
    """The n^3 LUT of a CDL as rsrt_colour_lut_download returns it: [n, n, n, 3] float32, indexed blue, green, red.  pow_fn: what to
    take the power with instead of pow_ (the accuracy test passes pow_f64)."""
    pow_fn = pow_fn or pow_
    assert n in LUT_SIZES and cdl_params_ok(slope, offset, power, saturation)
    three = lambda v: [F(a) for a in np.broadcast_to(np.asarray(v, F), (3,))]  # noqa: E731
    slope, offset, power, sat = three(slope), three(offset), three(power), F(saturation)
    enc = (np.arange(n).astype(F) / F(n - 1)).astype(F)
    lin = (enc * enc).astype(F)
    ib, ig, ir = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    x = []
    for i, idx in enumerate((ir, ig, ib)):
        v = clamp01(((lin[idx] * slope[i]).astype(F) + offset[i]).astype(F))
        x.append(pow_fn(v, power[i]) if power[i] != 1 else v)
    if sat != 1:
        y = (((F(0.2126) * x[0]).astype(F) + (F(0.7152) * x[1]).astype(F)).astype(F) + (F(0.0722) * x[2]).astype(F)).astype(F)
        x = [(y + (sat * (v - y).astype(F)).astype(F)).astype(F) for v in x]
    return np.stack([np.sqrt(clamp01(v)).astype(F) for v in x], axis=-1)


def lut_axis(enc, n):
    p = (enc * F(n - 1)).astype(F)
    i = np.minimum(p.astype(np.int64), n - 2)
    return i, (p - i.astype(F)).astype(F)


def lut_at(lut, enc):
    """rsrt_colour_lut_at: lut [n, n, n, >=3] (blue, green, red index) at encoded rgb enc [..., 3] in [0, 1]."""
    n = lut.shape[0]
    flat = np.asarray(lut, F)[..., :3].reshape(-1, 3)
    ir, ta = lut_axis(enc[..., 0], n)
    ig, tb = lut_axis(enc[..., 1], n)
    ib, tc = lut_axis(enc[..., 2], n)
    sa, sb, sc = np.full(ta.shape, 1, np.int64), np.full(ta.shape, n, np.int64), np.full(ta.shape, n * n, np.int64)

    def swap(t0, s0, t1, s1):
        c = t0 < t1
        return np.where(c, t1, t0), np.where(c, s1, s0), np.where(c, t0, t1), np.where(c, s0, s1)
    ta, sa, tb, sb = swap(ta, sa, tb, sb)
    tb, sb, tc, sc = swap(tb, sb, tc, sc)
    ta, sa, tb, sb = swap(ta, sa, tb, sb)
    w = [(F(1) - ta).astype(F), (ta - tb).astype(F), (tb - tc).astype(F), tc.astype(F)]
    n0 = (ib * n + ig) * n + ir
    at = [n0, n0 + sa, n0 + sa + sb, n0 + sa + sb + sc]
    term = [(w[k][..., None] * flat[at[k]]).astype(F) for k in range(4)]
    return (((term[0] + term[1]).astype(F) + term[2]).astype(F) + term[3]).astype(F)


def grade(sdr, lut, strength):
    """rsrt_colour_grade: tone-mapped sdr [..., 3] through the LUT at a strength > 0."""
    with np.errstate(all="ignore"):
        enc = np.sqrt(np.where(np.isnan(sdr), F(0), sdr).astype(F)).astype(F)
        g = lut_at(lut, enc)
        o = clamp01((enc + (F(strength) * (g - enc).astype(F)).astype(F)).astype(F))
        return (o * o).astype(F)


def tone_map(hdr):
    """rsrt_aces_tone_map of hdr [h, w, 3]: float32 sdr, NaN where the header leaves one (bloom_ref.tone_map_encode's first half)."""
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
        sdr = np.where(np.isnan(r), f(np.nan), sdr).astype(F)
        sdr[(hdr < 0).any(axis=-1)] = F([1, 0, 1])
    return sdr


def encode(sdr):
    """rsrt_srgb8_encode per channel (NaN -> 0): [h, w, 4] uint8, alpha 255."""
    import test_display
    codes = np.searchsorted(test_display.srgb_thresholds(), np.where(np.isnan(sdr), F(0), sdr), side="right").astype(np.uint8)
    return np.concatenate([codes, np.full(codes.shape[:2] + (1,), 255, np.uint8)], axis=-1)


def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None):
    """rsrt_display_pixel_colour per pixel: [h, w, 4] uint8 from sums [h, w, >=3], the local gains [h, w] (None: 1), with
    intensity > 0 the bloom image b [ceil(h/2), ceil(w/2), >=3], the white point and, with strength > 0, the LUT."""
    h, w = sums.shape[:2]
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / F(total)).astype(np.float16).astype(F)
        hdr = (mean * F(exposure)).astype(F)
        up = bloom_ref.up(np.asarray(b, F)[..., :3], h, w) if intensity > 0 else np.zeros((h, w, 3), F)
        hdr = (hdr + (F(intensity) * up).astype(F)).astype(F)
        hdr = (hdr * (np.ones((h, w), F) if gain is None else np.asarray(gain, F))[..., None]).astype(F)
        hdr = (hdr * np.asarray(white, F)).astype(F)
    sdr = tone_map(hdr)
    if strength > 0:
        sdr = grade(sdr, lut, strength)
    return encode(sdr)


def chroma_frame(h, w, seed, specials=True):
    """Sums [h, w, 4] float32 as an accumulator holds them (to be read with total 1 or 3): lognormal luminance with chroma
    log-uniform over +-3 octaves in both G/R and G/B, so that the edge bins fill, and, where the frame has room, the special pixels —
    a zero, a -1, a NaN, a +inf and a denormal in one channel each, an all-zero pixel and a -0.  Returns (sums, {name: flat index})."""
    rng = np.random.default_rng(seed)
    s = np.empty((h, w, 4), F)
    g = np.exp(rng.normal(-1.0, 1.0, (h, w)))
    s[..., 1] = g
    s[..., 0] = g * 2.0 ** -rng.uniform(-3, 3, (h, w))
    s[..., 2] = g * 2.0 ** -rng.uniform(-3, 3, (h, w))
    s[..., 3] = 1
    n = h * w
    flat = s.reshape(-1, 4)
    special = {}
    if specials and n >= 16:
        names = ["zero_channel", "minus_one", "nan", "inf", "denormal", "black", "neg_zero"]
        special = {k: int(i) for k, i in zip(names, rng.choice(n, size=len(names), replace=False))}
        flat[special["zero_channel"], 0] = 0
        flat[special["minus_one"], 2] = -1
        flat[special["nan"], 1] = np.nan
        flat[special["inf"], 2] = np.inf
        flat[special["denormal"], 0] = 1e-41
        flat[special["black"], :3] = 0
        flat[special["neg_zero"], :3] = -0.0
    return s, special


def near_grey_frame(h, w, seed, tint=(1.0, 1.0, 1.0), saturated=0.35):
    """Sums [h, w, 4] float32: near-grey surfaces (chroma within +-0.2 octave) with a share `saturated` of strongly coloured pixels
    (one channel 2 to 3 octaves down), everything multiplied by `tint`."""
    rng = np.random.default_rng(seed)
    lum = np.exp(rng.normal(-1.0, 0.8, (h, w, 1)))
    c = lum * 2.0 ** rng.uniform(-0.2, 0.2, (h, w, 3))
    sat = rng.random((h, w)) < saturated
    ch = rng.integers(0, 3, (h, w))
    drop = 2.0 ** -rng.uniform(2, 3, (h, w))
    for k in range(3):
        c[..., k] = np.where(sat & (ch == k), c[..., k] * drop, c[..., k])
    s = np.ones((h, w, 4), F)
    s[..., :3] = (c * np.asarray(tint, np.float64)).astype(F)
    return s
