"""The finished display (include/rsrt_finish.h) restated in numpy, step for step and in the header's order: the sdr of a pixel over
colour_ref's, bloom_ref's and local_ref's restatements, the records, the sharpener over a cross clamped at the picture's border (min and
max as the header's selects), the hash in 64-bit integers masked to 32, the grain, the way back to linear and the dithered quantiser.
The CPU evaluation of the header (tests/test_finish.py) and the GPU kernels (tests/test_finish_gpu.py) both equal it bit for bit."""
import numpy as np

import bloom_ref
import colour_ref

F = np.float32
NOISE_AWARE = 1
DEFAULTS = {"sharpness": 0.5, "grain": 0.0, "dither": 1.0, "seed": 0, "flags": 0}
LOBE_LIMIT = F(0.1875)
M32 = np.uint64(0xffffffff)


def params_ok(sharpness, grain, dither, seed=0, flags=0):
    with np.errstate(all="ignore"):
        return bool(all(0 <= F(v) <= 1 for v in (sharpness, grain, dither)) and (flags & ~NOISE_AWARE) == 0)


def thresholds():
    import test_display
    return np.asarray(test_display.srgb_thresholds(), F)


def fmin(a, b):
    return np.where(a < b, a, b).astype(F)


def fmax(a, b):
    return np.where(a > b, a, b).astype(F)


def sdr_of(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None):
    """rsrt_finish_sdr per pixel: colour_ref.display up to, and not including, the encode.  [h, w, 3] float32."""
    h, w = sums.shape[:2]
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / F(total)).astype(np.float16).astype(F)
        hdr = (mean * F(exposure)).astype(F)
        up = bloom_ref.up(np.asarray(b, F)[..., :3], h, w) if intensity > 0 else np.zeros((h, w, 3), F)
        hdr = (hdr + (F(intensity) * up).astype(F)).astype(F)
        hdr = (hdr * (np.ones((h, w), F) if gain is None else np.asarray(gain, F))[..., None]).astype(F)
        hdr = (hdr * np.asarray(white, F)).astype(F)
    sdr = colour_ref.tone_map(hdr)
    if strength > 0:
        sdr = colour_ref.grade(sdr, lut, strength)
    return sdr


def record(sdr):
    """rsrt_finish_record: [..., 3] sdr -> [..., 4] enc rgb and luma."""
    sdr = np.asarray(sdr, F)
    with np.errstate(all="ignore"):
        s = np.where(sdr > 0, np.where(sdr > 1, F(1), sdr), F(0)).astype(F)
    enc = np.sqrt(s).astype(F)
    luma = (((F(0.5) * enc[..., 0]).astype(F) + enc[..., 1]).astype(F) + (F(0.5) * enc[..., 2]).astype(F)).astype(F)
    return np.concatenate([enc, luma[..., None]], axis=-1)


def cross(rec):
    """b, d, f, h of every pixel of rec [h, w, 4], coordinates clamped to the picture."""
    p = np.pad(rec, ((1, 1), (1, 1), (0, 0)), mode="edge")
    return p[:-2, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[2:, 1:-1]


def sharpen(rec, sharpness, flags=0):
    """rsrt_finish_sharpen over a frame of records [h, w, 4]: [h, w, 3] encoded rgb."""
    b4, d4, f4, h4 = cross(rec)
    b, d, e, f, h = b4[..., :3], d4[..., :3], rec[..., :3], f4[..., :3], h4[..., :3]
    with np.errstate(all="ignore"):
        mn4 = fmin(fmin(b, d), fmin(f, h))
        mx4 = fmax(fmax(b, d), fmax(f, h))
        none = (mx4 == 0) | (mn4 == 1)
        hit_min = (mn4 / (F(4) * mx4).astype(F)).astype(F)
        hit_max = ((F(1) - mx4).astype(F) / ((F(4) * mn4).astype(F) - F(4)).astype(F)).astype(F)
        lobe_c = np.where(none, F(0), fmax(-hit_min, hit_max)).astype(F)
        lobe = (fmax(-LOBE_LIMIT, fmin(fmax(fmax(lobe_c[..., 0], lobe_c[..., 1]), lobe_c[..., 2]), F(0))) * F(sharpness)).astype(F)
        if flags & NOISE_AWARE:
            bl, dl, el, fl, hl = b4[..., 3], d4[..., 3], rec[..., 3], f4[..., 3], h4[..., 3]
            mx5 = fmax(fmax(fmax(fmax(bl, dl), el), fl), hl)
            mn5 = fmin(fmin(fmin(fmin(bl, dl), el), fl), hl)
            rng = (mx5 - mn5).astype(F)
            a = ((F(0.25) * ((bl + dl).astype(F) + (fl + hl).astype(F)).astype(F)).astype(F) - el).astype(F)
            a = np.where(a < 0, -a, a).astype(F)
            factor = (F(1) - (F(0.5) * fmin((a / rng).astype(F), F(1))).astype(F)).astype(F)
            lobe = (lobe * np.where(rng > 0, factor, F(1)).astype(F)).astype(F)
        den = ((F(4) * lobe).astype(F) + F(1)).astype(F)[..., None]
        diff = (((b + d).astype(F) + (f + h).astype(F)).astype(F) - (F(4) * e).astype(F)).astype(F)
        o = (e + ((lobe[..., None] * diff).astype(F) / den).astype(F)).astype(F)
    return colour_ref.clamp01(o)


def pcg(v):
    v = np.asarray(v).astype(np.uint64) & M32
    s = (v * np.uint64(747796405) + np.uint64(2891336453)) & M32
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & M32
    return ((w >> np.uint64(22)) ^ w) & M32


def hash_base(x, y, seed):
    return pcg(pcg(pcg(x) + np.asarray(y).astype(np.uint64)) + np.uint64(seed))


def hash_(x, y, seed, k):
    """rsrt_finish_hash: uint32 words (as uint64 below 2^32)."""
    return pcg(hash_base(x, y, seed) + np.uint64(k))


def uniform(word):
    return ((np.asarray(word).astype(np.uint64) >> np.uint64(8)).astype(F) * F(2.0 ** -24)).astype(F)


def frame_base(h, w, seed):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return hash_base(x, y, seed)


def shape(sdr, sharpness=0.5, grain=0.0, dither=1.0, seed=0, flags=0):
    """Steps 2, 3 and 5 of a frame of sdr [h, w, 3]: (the records' enc, the sharpened and grained enc), both [h, w, 3]."""
    assert params_ok(sharpness, grain, dither, seed, flags)
    rec = record(sdr)
    o = sharpen(rec, sharpness, flags) if sharpness > 0 else rec[..., :3].copy()
    if grain > 0:
        u0 = uniform(pcg(frame_base(sdr.shape[0], sdr.shape[1], seed)))
        t = (F(grain) * ((F(2) * u0).astype(F) - F(1)).astype(F)).astype(F)[..., None]
        o = (o + (t * fmin(o, (F(1) - o).astype(F))).astype(F)).astype(F)
    return rec[..., :3], o


def quantise(x, dither, u1, u2):
    """rsrt_finish_quantise per element: int64 codes."""
    x = np.asarray(x, F)
    t_ = thresholds()
    b = np.searchsorted(t_, np.where(np.isnan(x), F(0), x), side="right").astype(np.int64)
    if not dither > 0:
        return b
    with np.errstate(all="ignore"):
        lo, hi = t_[np.clip(b - 1, 0, 254)], t_[np.clip(b, 0, 254)]
        p = ((x - lo).astype(F) / (hi - lo).astype(F)).astype(F)
        t = (F(dither) * ((u1 + u2).astype(F) - F(1)).astype(F)).astype(F)
        v = (p + t).astype(F)
        moved = b + (v >= 1) - (v < 0)
    return np.where((b == 0) | (b == 255), b, moved)


def frame(sdr, sharpness=0.5, grain=0.0, dither=1.0, seed=0, flags=0):
    """Steps 2 to 7 of a frame of sdr [h, w, 3]: [h, w, 4] uint8, alpha 255."""
    sdr = np.asarray(sdr, F)
    h, w = sdr.shape[:2]
    enc, o = shape(sdr, sharpness, grain, dither, seed, flags)
    with np.errstate(all="ignore"):
        lin = np.where(o == enc, sdr, (o * o).astype(F)).astype(F)
    out = np.full((h, w, 4), 255, np.uint8)
    base = frame_base(h, w, seed)
    for c in range(3):
        u1 = u2 = None
        if dither > 0:
            u1, u2 = uniform(pcg(base + np.uint64(1 + 2 * c))), uniform(pcg(base + np.uint64(2 + 2 * c)))
        out[..., c] = quantise(lin[..., c], dither, u1, u2)
    return out


def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, **finish):
    """rsrt_display_finished_srgb8 on the host: [h, w, 4] uint8."""
    return frame(sdr_of(sums, total, exposure, white, lut, strength, gain, intensity, b), **finish)


def special_sdr(h, w, seed):
    """A frame of tone-mapped values [h, w, 3] float32 in [0, 1] with, where it has room, 0, 1, NaN, +-inf, negatives, denormals and every
    sRGB threshold with the floats one ulp either side of it."""
    rng = np.random.default_rng(seed)
    s = rng.random((h, w, 3)).astype(F) ** 2
    t = thresholds()
    pool = np.concatenate([F([0, -0.0, 1, np.nan, np.inf, -np.inf, -1, -1e-3, 1e-41, 1e-45, 2, 0.5]), t, np.nextafter(t, F(0)), np.nextafter(t, F(2))]).astype(F)
    flat = s.reshape(-1)
    n = pool.size if flat.size >= pool.size + 100 else flat.size // 2  # (33 x 9 and 67 x 5 take the whole pool: 777 values)
    flat[rng.choice(flat.size, size=n, replace=False)] = pool[:n]
    return s
