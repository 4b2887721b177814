"""The video pass (include/rsrt_video.h) restated in numpy, step for step: the display colour of a pixel over colour_ref's and hdr_ref's
restatements (the colour display's chain through its tone map and LUT, or the HDR display's up to its Rec.2020 nits), the continuous
transfer code over thresholds computed from the standards' formulas in float64 (not read from the headers), the Y'CbCr matrix, the
chroma reduction at the three sitings with clamped taps, the dithered quantiser over finish_ref's hash, and the four layouts.  The CPU
evaluation of the header (tests/test_video.py) and the GPU kernels (tests/test_video_gpu.py) both equal it byte for byte."""
import numpy as np

import colour_ref
import finish_ref
import hdr_ref

F = np.float32
BT709, HDR10 = 0, 1
SEMIPLANAR, PLANAR = 0, 1
LIMITED, FULL = 0, 1
LEFT, CENTRE, TOPLEFT = 0, 1, 2
STANDARDS = {"bt709": BT709, "hdr10": HDR10}
RANGES = {"limited": LIMITED, "full": FULL}
SITINGS = {"left": LEFT, "centre": CENTRE, "topleft": TOPLEFT}
LAYOUTS = {"nv12": (SEMIPLANAR, 8), "i420": (PLANAR, 8), "p010": (SEMIPLANAR, 10), "i420p10": (PLANAR, 10)}
DEFAULTS = {"standard": BT709, "depth": 8, "layout": SEMIPLANAR, "range": LIMITED, "siting": LEFT, "dither": 0.0, "seed": 0, "flags": 0}
# Kr, Kg, Kb and the two divisors 2 (1 - Kb), 2 (1 - Kr) as the standards print them: BT.709, BT.2020 non-constant luminance
MATRIX = {BT709: (0.2126, 0.7152, 0.0722, 1.8556, 1.5748), HDR10: (0.2627, 0.6780, 0.0593, 1.8814, 1.4746)}


def params_ok(standard, depth, layout, range, siting, dither, seed=0, flags=0):
    with np.errstate(all="ignore"):
        return bool(standard in (BT709, HDR10) and (depth == 10 or (depth == 8 and standard == BT709)) and layout in (SEMIPLANAR, PLANAR)
                    and range in (LIMITED, FULL) and siting in (LEFT, CENTRE, TOPLEFT) and 0 <= F(dither) <= 1 and flags == 0)


def table(standard):
    """(thresholds, N, end) of a standard's transfer."""
    import test_display
    return (hdr_ref.thresholds(), 1023, F(10000)) if standard == HDR10 else (test_display.srgb_thresholds(), 255, F(1))


def code(x, standard):
    """rsrt_video_code_srgb / _pq per element: the continuous code, float32."""
    t, n, end = table(standard)
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        b = np.searchsorted(t, np.where(np.isnan(x), F(0), x), side="right")
        lo, hi = t[np.clip(b - 1, 0, n - 1)], t[np.clip(b, 0, n - 1)]
        mid = ((b.astype(F) - F(0.5)).astype(F) + ((x - lo).astype(F) / (hi - lo).astype(F)).astype(F)).astype(F)
        first = np.where(x > 0, (F(0.5) * (x / t[0]).astype(F)).astype(F), F(0))
        last = np.where(x >= end, F(n), (F(n - 0.5) + (F(0.5) * ((x - t[n - 1]).astype(F) / F(end - t[n - 1])).astype(F)).astype(F)).astype(F))
        return np.where(b == 0, first, np.where(b == n, last, mid)).astype(F)


def signal(x, standard):
    """Step 2: E' of step 1's channels."""
    return (code(x, standard) / F(table(standard)[1])).astype(F)


def ycc(e, standard):
    """Step 3 on E' [..., 3]: Y', Cb', Cr' [..., 3]."""
    kr, kg, kb, db, dr = (F(v) for v in MATRIX[standard])
    e = np.asarray(e, F)
    y = (((kr * e[..., 0]).astype(F) + (kg * e[..., 1]).astype(F)).astype(F) + (kb * e[..., 2]).astype(F)).astype(F)
    return np.stack([y, ((e[..., 2] - y).astype(F) / db).astype(F), ((e[..., 0] - y).astype(F) / dr).astype(F)], axis=-1)


def reduce(c, siting):
    """Step 4 on one plane [h, w]: [ceil(h / 2), ceil(w / 2)] float32."""
    c = np.asarray(c, F)
    h, w = c.shape
    cy, cx = np.arange((h + 1) // 2), np.arange((w + 1) // 2)

    def at(y, x):
        return c[np.clip(y, 0, h - 1)[:, None], np.clip(x, 0, w - 1)[None, :]]

    def h121(y):
        return (((at(y, 2 * cx - 1) + at(y, 2 * cx + 1)).astype(F) + (F(2) * at(y, 2 * cx)).astype(F)).astype(F) * F(0.25)).astype(F)
    if siting == CENTRE:
        return (((at(2 * cy, 2 * cx) + at(2 * cy, 2 * cx + 1)).astype(F) + (at(2 * cy + 1, 2 * cx) + at(2 * cy + 1, 2 * cx + 1)).astype(F)).astype(F) * F(0.25)).astype(F)
    if siting == LEFT:
        return ((h121(2 * cy) + h121(2 * cy + 1)).astype(F) * F(0.5)).astype(F)
    return (((h121(2 * cy - 1) + h121(2 * cy + 1)).astype(F) + (F(2) * h121(2 * cy)).astype(F)).astype(F) * F(0.25)).astype(F)


def value(v, depth, range, chroma):
    """Step 5: (the value before the quantiser, lo, hi)."""
    m, peak = (F(4), F(1023)) if depth == 10 else (F(1), F(255))
    v = np.asarray(v, F)
    if range == FULL:
        return ((F(128) * m + (peak * v).astype(F)).astype(F) if chroma else (peak * v).astype(F)), F(0), peak
    return (m * (F(128 if chroma else 16) + (F(224 if chroma else 219) * v).astype(F)).astype(F)).astype(F), F(16) * m, F(240 if chroma else 235) * m


def quantise(v, lo, hi, t):
    v = np.clip(np.asarray(v, F), lo, hi)
    return np.clip(np.floor(((v + F(0.5)).astype(F) + t).astype(F)), lo, hi).astype(np.uint32)


def dither_of(h, w, dither, seed, k):
    """t of step 5 over an h x w plane from draws k and k + 1."""
    if not dither > 0:
        return F(0)
    base = finish_ref.frame_base(h, w, seed & 0xFFFFFFFF)
    u1, u2 = finish_ref.uniform(finish_ref.pcg(base + np.uint64(k))), finish_ref.uniform(finish_ref.pcg(base + np.uint64(k + 1)))
    return (F(dither) * ((u1 + u2).astype(F) - F(1)).astype(F)).astype(F)


def codes_of(yc, depth=8, range=LIMITED, siting=LEFT, dither=0.0, seed=0, **_):
    """Steps 4 and 5 of a frame of Y', Cb', Cr' [h, w, 3]: the codes y [h, w], cb, cr [ceil(h / 2), ceil(w / 2)], uint16."""
    h, w = yc.shape[:2]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = quantise(*value(yc[..., 0], depth, range, False), dither_of(h, w, dither, seed, 1))
    cb = quantise(*value(reduce(yc[..., 1], siting), depth, range, True), dither_of(ch, cw, dither, seed, 3))
    cr = quantise(*value(reduce(yc[..., 2], siting), depth, range, True), dither_of(ch, cw, dither, seed, 5))
    return y.astype(np.uint16), cb.astype(np.uint16), cr.astype(np.uint16)


def pack(y, cb, cr, depth=8, layout=SEMIPLANAR, **_):
    """Step 6: the frame's bytes, uint8 [n]."""
    t = np.dtype("<u2") if depth == 10 else np.uint8
    shift = 6 if depth == 10 and layout == SEMIPLANAR else 0
    planes = [y, np.stack([cb, cr], axis=-1)] if layout == SEMIPLANAR else [y, cb, cr]
    return np.concatenate([np.ascontiguousarray((p.astype(np.uint32) << shift).astype(t)).view(np.uint8).ravel() for p in planes])


def unpack(data, h, w, depth=8, layout=SEMIPLANAR, **_):
    """The codes (y, cb, cr) of a frame's bytes."""
    t = np.dtype("<u2") if depth == 10 else np.uint8
    v = np.frombuffer(np.ascontiguousarray(data, np.uint8).tobytes(), t).astype(np.uint16)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    assert v.size == h * w + 2 * ch * cw
    y, c = v[:h * w].reshape(h, w), v[h * w:]
    if layout == SEMIPLANAR:
        c = c.reshape(ch, cw, 2)
        cb, cr = c[..., 0], c[..., 1]
    else:
        cb, cr = c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
    if depth == 10 and layout == SEMIPLANAR:
        assert not ((y & 63).any() or (cb & 63).any() or (cr & 63).any())
        y, cb, cr = y >> 6, cb >> 6, cr >> 6
    return y, cb, cr


def frame_bytes(h, w, depth=8, **_):
    return (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)) * (2 if depth == 10 else 1)


def frame(e, **video):
    """Steps 3 to 6 of a frame of E' [h, w, 3]: (bytes, (y, cb, cr))."""
    q = dict(DEFAULTS, **video)
    assert params_ok(**q)
    c = codes_of(ycc(e, q["standard"]), **q)
    return pack(*c, **q), c


def source(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, hdr=None):
    """Step 1 of a frame: the sdr [h, w, 3] (hdr None) or the Rec.2020 nits with hdr = dict(paper_white, peak, knee)."""
    lin = hdr_ref.linear(sums, total, exposure, white, gain, intensity, b)
    if hdr is not None:
        return hdr_ref.nits_of(lin, hdr.get("paper_white", 203.0), hdr.get("peak", 1000.0), hdr.get("knee", 0.5), hdr_ref.PQ10)
    sdr = colour_ref.tone_map(lin)
    return colour_ref.grade(sdr, lut, strength) if strength > 0 else sdr


def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, hdr=None, **video):
    """rsrt_display_video on the host: (bytes, (y, cb, cr), the levels or None)."""
    q = dict(DEFAULTS, **video)
    assert (q["standard"] == HDR10) == (hdr is not None)
    x = source(sums, total, exposure, white, lut, strength, gain, intensity, b, hdr)
    data, c = frame(signal(x, q["standard"]), **q)
    return data, c, (hdr_ref.levels(x) if hdr is not None else None)
