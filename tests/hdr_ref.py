"""The HDR display (include/rsrt_hdr.h) restated in numpy, step for step and in the header's order: the linear colour of a pixel over
bloom_ref's and local_ref's restatements (colour_ref.display's chain up to its tone map), the sanitiser, the shoulder (min and max as
the header's selects), the scale to nits, BT.2087's matrix in rsrt_mat3_mul's association, the PQ thresholds from ST 2084's formula in
float64, the dithered quantiser over finish_ref's hash, the binary16 words and the integer light levels.  The CPU evaluation of the
header (tests/test_hdr.py) and the GPU kernels (tests/test_hdr_gpu.py) both equal it bit for bit."""
import functools

import numpy as np

import bloom_ref
import finish_ref

F = np.float32
PQ10, SCRGB16F = 0, 1
ENCODINGS = {"pq10": PQ10, "scrgb16f": SCRGB16F}
DEFAULTS = {"paper_white": 203.0, "peak": 1000.0, "knee": 0.5, "dither": 0.0, "seed": 0, "encoding": PQ10, "flags": 0}
CAP = F(2.0 ** 64)
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
# BT.2087: Rec.709 -> Rec.2020, rows
M2020 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]], F)


def eotf(e):
    """ST 2084's EOTF in float64: a signal in [0, 1] -> its share of 10000 cd/m^2."""
    p = float(e) ** (1.0 / M2)
    return (max(p - C1, 0.0) / (C2 - C3 * p)) ** (1.0 / M1)


def oetf(nits):
    """ST 2084's inverse EOTF in float64: cd/m^2 -> the signal in [0, 1]."""
    y = (float(nits) / 10000.0) ** M1
    return ((C1 + C2 * y) / (1.0 + C3 * y)) ** M2


@functools.lru_cache(maxsize=None)
def _thresholds():
    t = np.array([np.float32(10000.0 * eotf((j - 0.5) / 1023.0)) for j in range(1, 1024)], F)
    t.setflags(write=False)
    return t


def thresholds():
    """The 1023 thresholds in nits, from the formula (not from the header)."""
    return _thresholds()


def params_ok(paper_white, peak, knee, dither, seed=0, encoding=PQ10, flags=0):
    with np.errstate(all="ignore"):
        pw, pk, kn, di = F(paper_white), F(peak), F(knee), F(dither)
        return bool(1 <= pw <= 10000 and pw <= pk <= 10000 and 0 <= kn <= F(0.95) and 0 <= di <= 1
                    and (encoding == PQ10 or (encoding == SCRGB16F and not di > 0)) and flags == 0)


def fmax(a, b):
    return np.where(a > b, a, b).astype(F)


def linear(sums, total, exposure, white=(1.0, 1.0, 1.0), gain=None, intensity=0.0, b=None):
    """rsrt_hdr_linear per pixel (step 1): [h, w, 3] float32, what colour_ref.display hands to its tone map."""
    h, w = sums.shape[:2]
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / F(total)).astype(np.float16).astype(F)
        hdr = (mean * F(exposure)).astype(F)
        up = bloom_ref.up(np.asarray(b, F)[..., :3], h, w) if intensity > 0 else np.zeros((h, w, 3), F)
        hdr = (hdr + (F(intensity) * up).astype(F)).astype(F)
        hdr = (hdr * (np.ones((h, w), F) if gain is None else np.asarray(gain, F))[..., None]).astype(F)
        return (hdr * np.asarray(white, F)).astype(F)


def sanitise(x):
    """Step 2."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.where(x > CAP, CAP, x), F(0)).astype(F)


def curve(paper_white, peak, knee):
    """(P, k, d) as float32."""
    P = F(F(peak) / F(paper_white))
    k = F(F(knee) * P)
    return P, k, F(P - k)


def compress(x, paper_white, peak, knee):
    """Step 3 on sanitised x [..., 3]."""
    x = np.asarray(x, F)
    P, k, d = curve(paper_white, peak, knee)
    m = fmax(fmax(x[..., 0], x[..., 1]), x[..., 2])
    with np.errstate(all="ignore"):
        e = (m - k).astype(F)
        c = (k + (d * (e / (d + e).astype(F)).astype(F)).astype(F)).astype(F)
        s = (c / m).astype(F)
        return np.where((m <= k)[..., None], x, (x * s[..., None]).astype(F)).astype(F)


def to_nits(x, paper_white, peak):
    """Step 4."""
    n = (F(paper_white) * np.asarray(x, F)).astype(F)
    return np.where(n > F(peak), F(peak), n).astype(F)


def to_rec2020(nits, peak):
    """Step 5's matrix: (row.r * n.r + row.g * n.g) + row.b * n.b, clamped to the peak."""
    n = np.asarray(nits, F)
    out = np.empty_like(n)
    for i in range(3):
        out[..., i] = ((M2020[i, 0] * n[..., 0]).astype(F) + (M2020[i, 1] * n[..., 1]).astype(F)).astype(F) + (M2020[i, 2] * n[..., 2]).astype(F)
    return np.where(out > F(peak), F(peak), out).astype(F)


def nits_of(lin, paper_white=203.0, peak=1000.0, knee=0.5, encoding=PQ10, **_):
    """rsrt_hdr_nits_of (steps 2 to 5): nits in the encoding's primaries."""
    n = to_nits(compress(sanitise(lin), paper_white, peak, knee), paper_white, peak)
    return to_rec2020(n, peak) if encoding == PQ10 else n


def pq_encode(nits):
    """rsrt_pq10_encode per element (NaN -> 0): int64 codes."""
    nits = np.asarray(nits, F)
    return np.searchsorted(thresholds(), np.where(np.isnan(nits), F(0), nits), side="right").astype(np.int64)


def quantise(nits, dither, u1, u2):
    """rsrt_hdr_quantise per element: int64 codes."""
    nits = np.asarray(nits, F)
    t_ = thresholds()
    b = pq_encode(nits)
    if not dither > 0:
        return b
    with np.errstate(all="ignore"):
        lo, hi = t_[np.clip(b - 1, 0, 1022)], t_[np.clip(b, 0, 1022)]
        p = ((nits - lo).astype(F) / (hi - lo).astype(F)).astype(F)
        t = (F(dither) * ((u1 + u2).astype(F) - F(1)).astype(F)).astype(F)
        v = (p + t).astype(F)
        moved = b + (v >= 1) - (v < 0)
    return np.where((b == 0) | (b == 1023), b, moved)


def pack_pq10(nits, dither=0.0, seed=0):
    """rsrt_hdr_pack_pq10 over a frame of Rec.2020 nits [h, w, 3]: [h, w] uint32."""
    h, w = nits.shape[:2]
    word = np.full((h, w), 3 << 30, np.uint64)
    base = finish_ref.frame_base(h, w, seed & 0xFFFFFFFF)
    for c in range(3):
        u1 = u2 = None
        if dither > 0:
            u1, u2 = finish_ref.uniform(finish_ref.pcg(base + np.uint64(1 + 2 * c))), finish_ref.uniform(finish_ref.pcg(base + np.uint64(2 + 2 * c)))
        word |= quantise(nits[..., c], dither, u1, u2).astype(np.uint64) << np.uint64(10 * c)
    return word.astype(np.uint32)


def f16_bits(v):
    """rsrt_hdr_f16_bits: numpy's float32 -> float16 conversion is round to nearest even."""
    with np.errstate(all="ignore"):
        return np.asarray(v, F).astype(np.float16).view(np.uint16)


def pack_scrgb(nits):
    """rsrt_hdr_pack_scrgb over a frame of Rec.709 nits [h, w, 3]: [h, w, 4] uint16."""
    out = np.full(nits.shape[:2] + (4,), 0x3C00, np.uint16)
    out[..., :3] = f16_bits((np.asarray(nits, F) / F(80)).astype(F))
    return out


def level_q(nits):
    """Step 7 per pixel: uint32."""
    L = fmax(fmax(nits[..., 0], nits[..., 1]), nits[..., 2])
    return (L * F(64)).astype(F).astype(np.uint32)


def levels(nits):
    """The frame's levels from its nits [h, w, 3]: the dict State.display_hdr returns."""
    q = level_q(nits).astype(np.uint64)
    max_q, sum_q = int(q.max()), int(q.sum())
    return {"max_q": max_q, "sum_q": sum_q, "max_cll": float(F(max_q / 64.0)), "max_fall": float(F(sum_q / (64.0 * q.size)))}


def frame(lin, paper_white=203.0, peak=1000.0, knee=0.5, dither=0.0, seed=0, encoding=PQ10, flags=0):
    """Steps 2 to 7 of a frame of linear colour [h, w, 3]: (the words — [h, w] uint32 or [h, w, 4] uint16 —, the levels)."""
    assert params_ok(paper_white, peak, knee, dither, seed, encoding, flags)
    n = nits_of(lin, paper_white, peak, knee, encoding)
    return (pack_pq10(n, dither, seed) if encoding == PQ10 else pack_scrgb(n)), levels(n)


def display(sums, total, exposure, white=(1.0, 1.0, 1.0), gain=None, intensity=0.0, b=None, **hdr):
    """rsrt_display_hdr on the host: (words, levels)."""
    return frame(linear(sums, total, exposure, white, gain, intensity, b), **hdr)


def unpack_pq10(words):
    """[h, w] uint32 -> [h, w, 3] codes."""
    w = np.asarray(words, np.uint32)
    return np.stack([(w >> np.uint32(10 * c)) & np.uint32(1023) for c in range(3)], axis=-1).astype(np.uint16)
