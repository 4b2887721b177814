"""The HDR display without a GPU: the published arithmetic (include/rsrt_hdr.h), compiled for the CPU, against the numpy restatement
the GPU tests hold the kernels to (tests/hdr_ref.py), bit for bit and word for word, special values included; the PQ table against
ST 2084's formula; codes the standard gives; what the shoulder, the dither and the light levels promise, with bounds worked out in the
tests' comments; the parameter checks, the ABI, the kernels' code objects, the C++ State and a sanitizer run of the host program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import bloom_ref
import hdr_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (1, 2), (8, 32), (9, 33), (5, 67)]  # (h, w)
F = np.float32
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "hdr_host.cpp")
PQ10, SCRGB16F = hdr_ref.PQ10, hdr_ref.SCRGB16F
# the defaults and the parameters' corners: knee 0 and 0.95, peak equal to paper white, peak 10000
CORNERS = [dict(paper_white=203.0, peak=1000.0, knee=0.5), dict(paper_white=203.0, peak=1000.0, knee=0.0), dict(paper_white=100.0, peak=100.0, knee=0.95),
           dict(paper_white=1.0, peak=10000.0, knee=0.95), dict(paper_white=10000.0, peak=10000.0, knee=0.0), dict(paper_white=80.0, peak=10000.0, knee=0.25)]
SETTINGS = [dict(k, encoding=e, dither=d, seed=s) for k in CORNERS for e, d, s in ((PQ10, 0.0, 0), (PQ10, 1.0, 0x9e3779b9), (PQ10, 0.5, 3), (SCRGB16F, 0.0, 0))]


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def hdr_params(paper_white=203.0, peak=1000.0, knee=0.5, dither=0.0, seed=0, encoding=PQ10, flags=0):
    return state.HdrParams(paper_white, peak, knee, dither, seed, encoding, flags, 0)


def colour_params(white=(1.0, 1.0, 1.0), strength=0.0, flags=0):
    return state.ColourParams((C.c_float * 3)(*white), strength, flags, (C.c_uint32 * 3)())


def levels_dict(lv):
    return {"max_q": lv.max_q, "sum_q": lv.sum_q, "max_cll": lv.max_cll, "max_fall": lv.max_fall}


def frame_sums(h, w, total=3):
    """local_ref.synthetic's frame (NaN, +-inf, a negative, -0, a denormal and 3e38 in the sums where it has room) with, where it has room,
    a mean of exactly 65504, the largest half, and one of 65520, the first that rounds to infinity."""
    sums, special = local_ref.synthetic(h, w, seed=2000 * h + w)
    if h * w >= 64:
        free = [i for i in range(h * w) if i not in special.values()]
        sums.reshape(-1, 4)[free[5], :3] = F(65504.0 * total)
        sums.reshape(-1, 4)[free[11], :3] = (F(65520.0 * total), 1.0, 2.0)
    return sums


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hdr") / "libhdr.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.hdr_table.argtypes = [C.c_void_p]
    L.hdr_pq_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.hdr_quantise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.hdr_f16_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.hdr_steps.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hdr_curve.argtypes = [C.c_void_p, C.c_void_p]
    L.hdr_nits.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.hdr_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hdr_pack_pq10.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.hdr_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hdr_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hdr_params_ok.argtypes = [C.c_void_p]
    L.hdr_defaults.argtypes = [C.c_void_p]
    L.hdr_layout.argtypes = [C.c_void_p]

    def out_for(shape, encoding):
        return np.zeros(shape + (4,), np.uint16) if encoding == SCRGB16F else np.zeros(shape, np.uint32)

    class Host:
        @staticmethod
        def table():
            t = np.empty(1023, F)
            L.hdr_table(t.ctypes.data)
            return t

        @staticmethod
        def pq_encode(x):
            x = np.ascontiguousarray(x, F)
            out = np.empty(x.shape, np.uint32)
            L.hdr_pq_encode(x.ctypes.data, x.size, out.ctypes.data)
            return out

        @staticmethod
        def quantise(x, dither, u1, u2):
            x, u1, u2 = (np.ascontiguousarray(v, F) for v in (x, u1, u2))
            out = np.empty(x.shape, np.uint32)
            L.hdr_quantise(x.ctypes.data, u1.ctypes.data, u2.ctypes.data, x.size, dither, out.ctypes.data)
            return out

        @staticmethod
        def f16_bits(x):
            x = np.ascontiguousarray(x, F)
            out = np.empty(x.shape, np.uint16)
            L.hdr_f16_bits(x.ctypes.data, x.size, out.ctypes.data)
            return out

        @staticmethod
        def steps(lin, **kw):
            lin = np.ascontiguousarray(lin, F)
            outs = [np.empty_like(lin) for _ in range(3)]
            p = hdr_params(**kw)
            L.hdr_steps(lin.ctypes.data, lin.size // 3, C.byref(p), *(o.ctypes.data for o in outs))
            return outs

        @staticmethod
        def curve(**kw):
            out = np.empty(3, F)
            p = hdr_params(**kw)
            L.hdr_curve(C.byref(p), out.ctypes.data)
            return tuple(out)

        @staticmethod
        def nits(lin, **kw):
            lin = np.ascontiguousarray(lin, F)
            out = np.empty_like(lin)
            p = hdr_params(**kw)
            L.hdr_nits(lin.ctypes.data, lin.size // 3, C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def linear(sums, total, exposure, white=(1.0, 1.0, 1.0), gain=None, intensity=0.0, b=None):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            gain = None if gain is None else np.ascontiguousarray(gain, F)
            b = None if b is None else np.ascontiguousarray(b, F)
            c = colour_params(white)
            out = np.empty((h, w, 3), F)
            L.hdr_linear(sums.ctypes.data, h, w, total, exposure, None if gain is None else gain.ctypes.data, intensity, None if b is None else b.ctypes.data, C.byref(c),
                         out.ctypes.data)
            return out

        @staticmethod
        def pack_pq10(nits, **kw):
            nits = np.ascontiguousarray(nits, F)
            out = np.zeros(nits.shape[:2], np.uint32)
            p = hdr_params(**kw)
            L.hdr_pack_pq10(nits.ctypes.data, nits.shape[0], nits.shape[1], C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def frame(lin, **kw):
            lin = np.ascontiguousarray(lin, F)
            out = out_for(lin.shape[:2], kw.get("encoding", PQ10))
            p, lv = hdr_params(**kw), state.HdrLevels()
            L.hdr_frame(lin.ctypes.data, lin.shape[0], lin.shape[1], C.byref(p), out.ctypes.data, C.byref(lv))
            return out, levels_dict(lv)

        @staticmethod
        def display(sums, total, exposure, white=(1.0, 1.0, 1.0), gain=None, intensity=0.0, b=None, **kw):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            gain = None if gain is None else np.ascontiguousarray(gain, F)
            b = None if b is None else np.ascontiguousarray(b, F)
            out = out_for((h, w), kw.get("encoding", PQ10))
            c, p, lv = colour_params(white), hdr_params(**kw), state.HdrLevels()
            L.hdr_display(sums.ctypes.data, h, w, total, exposure, None if gain is None else gain.ctypes.data, intensity, None if b is None else b.ctypes.data, C.byref(c),
                          C.byref(p), out.ctypes.data, C.byref(lv))
            return out, levels_dict(lv)
    Host.L = L
    return Host


# -- the table, the quantiser, known codes ---------------------------------------------------------------------------------------------
def test_the_table_is_the_formula_in_float64_rounded_to_f32(host):
    """T[j - 1] = f32(10000 * EOTF((j - 0.5) / 1023)), recomputed here; strictly increasing normal floats."""
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32

    def eotf(e):
        p = e ** (1 / m2)
        return (max(p - c1, 0.0) / (c2 - c3 * p)) ** (1 / m1)
    want = np.array([F(10000.0 * eotf((j - 0.5) / 1023.0)) for j in range(1, 1024)], F)
    got = host.table()
    assert same(got, want) and same(got, hdr_ref.thresholds())
    assert (np.diff(got.astype(np.float64)) > 0).all() and got[0] >= np.finfo(F).tiny and np.isfinite(got).all()
    assert got[0] == F(1.2384006e-05) and got[1022] == F(9953.416)


def test_every_threshold_and_its_neighbours_through_the_quantiser(host):
    t = hdr_ref.thresholds()
    below, above = np.nextafter(t, F(0)), np.nextafter(t, F(20000))
    j = np.arange(1, 1024)
    assert np.array_equal(host.pq_encode(t), j) and np.array_equal(host.pq_encode(above), j) and np.array_equal(host.pq_encode(below), j - 1)  # steps at T
    ends = F([0, -0.0, 10000, 20000, np.inf, np.nan, -1, -np.inf, 1e-41])
    assert list(host.pq_encode(ends)) == [0, 0, 1023, 1023, 1023, 0, 0, 0, 0]
    x = np.concatenate([t, below, above, ends]).astype(F)
    assert np.array_equal(host.pq_encode(x), hdr_ref.pq_encode(x))
    rng = np.random.default_rng(5)
    for dither in (0.0, 0.5, 1.0):
        for _ in range(3):
            u1, u2 = (rng.integers(0, 1 << 24, x.size).astype(F) * F(2.0 ** -24) for _ in range(2))
            got = host.quantise(x, dither, u1, u2).astype(np.int64)
            assert np.array_equal(got, hdr_ref.quantise(x, dither, u1, u2)), dither
            hard = hdr_ref.pq_encode(x)
            assert np.abs(got - hard).max() <= (1 if dither else 0)
            assert np.array_equal(got[(hard == 0) | (hard == 1023)], hard[(hard == 0) | (hard == 1023)])  # codes 0 and 1023 never move


def test_known_codes_of_the_standard(host):
    """Full-range 10-bit codes round(1023 * OETF(nits)) from ST 2084's inverse EOTF in float64: none within 0.04 of a code boundary."""
    table = {1: 153, 100: 520, 203: 594, 1000: 769, 10000: 1023}
    for nits, code in table.items():
        v = 1023.0 * hdr_ref.oetf(nits)
        assert int(np.floor(v + 0.5)) == code and (nits == 10000 or abs(v - np.floor(v) - 0.5) >= 0.04), (nits, v)
    assert list(host.pq_encode(F(list(table)))) == list(table.values())
    assert list(hdr_ref.pq_encode(F(list(table)))) == list(table.values())


def test_half_bits_match_numpy(host):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(F),
                        F([0, -0.0, 1, 125, 65504, 65519.99, 65520, 6.1035156e-05, 6.0975552e-05, 5.9604645e-08, 2.9802322e-08, 2.98023226e-08 * 1.0001, np.inf, -np.inf])])
    x = x[~np.isnan(x)]
    assert np.array_equal(host.f16_bits(x), hdr_ref.f16_bits(x))
    # every half's value goes to its own bits, and the midpoints between neighbours go to the even one
    halves = np.arange(0, 0x7c00, dtype=np.uint16)
    assert np.array_equal(host.f16_bits(halves.view(np.float16).astype(F)), halves)
    mid = ((halves[:-1].view(np.float16).astype(np.float64) + halves[1:].view(np.float16).astype(np.float64)) / 2).astype(F)  # (exact in f32)
    assert np.array_equal(host.f16_bits(mid), np.where(halves[:-1] % 2 == 0, halves[:-1], halves[1:]))


# -- bit for bit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_every_step_and_the_whole_pass_match_numpy(host, h, w):
    total, exposure, white = 3, 0.37, (1.3, 0.95, 0.6)
    sums = frame_sums(h, w, total)
    if h * w >= 64:
        flat = sums[..., :3].reshape(-1)
        assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (flat < 0).any() and (np.signbit(flat) & (flat == 0)).any()
        assert ((flat > 0) & (flat < np.finfo(F).tiny)).any() and (flat == F(65504.0 * total)).any()
    b = bloom_ref.bloom(sums, total, exposure, 3)
    gain = local_ref.gains(sums, total, exposure, local_ref.grid_of(sums, total, 8), 8)
    for wh, g, intensity in ((white, gain, 0.5), ((1.0, 1.0, 1.0), None, 0.0), (white, None, 0.5), (white, gain, 0.0)):
        args = (sums, total, exposure, wh, g, intensity, b)
        lin = hdr_ref.linear(*args)
        assert util.same_bits_or_nan(host.linear(*args), lin)
        for kw in SETTINGS:
            curve = {k: kw[k] for k in ("paper_white", "peak", "knee")}
            assert same(host.curve(**curve), hdr_ref.curve(**curve))
            s, c, n = host.steps(lin, **curve)
            assert same(s, hdr_ref.sanitise(lin)) and np.isfinite(s).all() and not np.signbit(s).any()
            assert same(c, hdr_ref.compress(s, **curve)) and same(n, hdr_ref.to_nits(c, kw["paper_white"], kw["peak"]))
            nits = host.nits(lin, **kw)
            assert same(nits, hdr_ref.nits_of(lin, **kw)) and nits.min() >= 0 and nits.max() <= kw["peak"]
            want, want_lv = hdr_ref.frame(lin, **kw)
            got, lv = host.frame(lin, **kw)
            assert np.array_equal(got, want) and lv == want_lv, kw
            got, lv = host.display(*args, **kw)
            assert np.array_equal(got, want) and lv == want_lv, kw
            assert np.array_equal(got, hdr_ref.display(*args, **kw)[0])


# -- properties --------------------------------------------------------------------------------------------------------------------------
def sweep(P, k, d):
    """A dense sweep of m for the curve (P, k, d), dense where the curve moves: 4096 values from 0 to the knee, then the m at which the
    exact curve stands at k + d t, t = j / 2^15, j = 1 .. 2^15 - 1 (m = k + d t / (1 - t): up to 32767 d above the knee, where the
    curve is within d / 2^15 of its asymptote).  Neighbours above the knee lie d / 2^15 >= 0.05 P / 2^15 = 12.8 * 2^-23 P apart on the
    exact curve, which is what a test of monotonicity in f32 needs: the evaluated c carries the roundings of d + e, of the division, of
    the product with d and of the sum with k, and the largest channel m * (c / m) two more, under 6 * 2^-24 P in all, so only samples
    whose exact values differ by more than twice that are ordered by the arithmetic rather than by its rounding.  (Further up the
    asymptote neighbouring floats of m share their c to within that rounding, and the evaluated curve may step back by an ulp or two:
    tail() below holds it to that.)"""
    t = np.arange(1, 1 << 15, dtype=np.float64) / (1 << 15)
    return np.concatenate([np.linspace(0.0, float(k), 4096), float(k) + float(d) * t / (1 - t)]).astype(F)


def tail(P):
    """From 2^15 to 2^40 peaks, 2000 values a decade, then every power of two up to the cap."""
    return np.concatenate([float(P) * np.exp(np.linspace(np.log(2.0 ** 15), np.log(2.0 ** 40), 15000)), 2.0 ** np.arange(54, 65)]).astype(F)


def test_below_the_knee_a_pixel_passes_and_its_nits_are_paper_white_times_x(host):
    rng = np.random.default_rng(3)
    for kw in CORNERS:
        P, k, d = hdr_ref.curve(**kw)
        x = (rng.random((4000, 3)).astype(F) * k).astype(F)
        x[0] = k  # m == k passes
        x[1] = 0
        s, c, n = host.steps(x, **kw)
        assert same(c, x) and same(n, (F(kw["paper_white"]) * x).astype(F)), kw
        far = F(2) * P  # (well above the knee the shoulder is at work: twice the peak comes out below the peak)
        assert k < host.steps(F([[far, far, far]]), **kw)[1][0, 0] < P


def test_no_code_exceeds_the_peaks_and_infinity_gives_the_peaks_code(host):
    inf, nan = np.inf, np.nan
    lin = F([[inf, inf, inf], [inf, 0, 0], [0, inf, 0], [0, 0, inf], [nan, -1, -0.0], [-inf, nan, -3e38], [3e38, 3e38, 3e38], [1e-45, 0, nan]])[None]
    rng = np.random.default_rng(4)
    wild = np.exp(rng.normal(2.0, 6.0, (1, 20000, 3))).astype(F)
    for kw in CORNERS:
        peak_code = int(hdr_ref.pq_encode(F(kw["peak"])))
        codes = hdr_ref.unpack_pq10(host.frame(lin, **kw)[0])[0]
        assert list(codes[0]) == [peak_code] * 3, kw  # a grey infinity: every channel at the peak's code
        assert codes[:4].max() == peak_code and codes.max() <= peak_code
        assert list(codes[4]) == [0, 0, 0] and list(codes[5]) == [0, 0, 0]  # NaN and negatives give 0
        assert list(codes[6]) == [peak_code] * 3 and list(codes[7]) == [0, 0, 0]
        half, lv = host.frame(lin, **dict(kw, encoding=SCRGB16F))
        assert np.array_equal(half[0, 4], [0, 0, 0, 0x3C00]) and np.array_equal(half[0, 5], [0, 0, 0, 0x3C00])
        # scRGB: an infinite channel sits at the peak, to the two roundings of c / m * m and of the division by 80 (1 half ulp)
        top = half[0, :4, :3].view(np.float16).astype(np.float64).max(axis=-1) * 80
        assert np.abs(top / kw["peak"] - 1).max() <= 2.0 ** -10 and lv["max_cll"] <= kw["peak"]
        assert hdr_ref.unpack_pq10(host.frame(wild, **kw)[0]).max() <= peak_code
        assert host.frame(wild, **dict(kw, dither=1.0, seed=9))[0].view(np.uint32).max() >> 30 == 3
        assert hdr_ref.unpack_pq10(host.frame(wild, **dict(kw, dither=1.0, seed=9))[0]).max() <= peak_code + 1  # (the dither's one code)


def test_the_curve_is_non_decreasing_and_keeps_the_channels_ratios(host):
    """Over the sweep, on a grey and on two coloured pixels: the largest channel after the shoulder never falls as m grows, never passes
    P by more than the rounding of k + d, and the channels' ratios stay.  The ratios' bound: x_i' = fl(x_i * s) and x_j' = fl(x_j * s)
    with one factor s, so x_i' / x_j' = (x_i / x_j) (1 + a) / (1 + b) with |a|, |b| <= 2^-24, the two roundings of the two products: a
    relative difference of at most 2 * 2^-24 + O(2^-48); 2.001 * 2^-24 here, in float64.  Up the asymptote (tail) the curve stays
    between its last swept value less the evaluation's rounding (6 * 2^-24 P: sweep's docstring) and P, and the PQ codes and the scRGB
    halves never fall over sweep and tail together."""
    for kw in CORNERS:
        P, k, d = hdr_ref.curve(**kw)
        m, far = sweep(P, k, d), tail(P)
        assert (np.diff(m.astype(np.float64)) >= 0).all() and m[-1] < far[0]
        for ratio in ((1.0, 1.0, 1.0), (1.0, 0.4375, 0.0625), (0.3, 1.0, 0.7)):
            x = (m[:, None] * F(ratio)).astype(F)
            x = x[np.argsort(x.max(axis=-1), kind="stable")]  # (by the largest channel as rounded)
            c = host.steps(x, **kw)[1]
            assert same(c, hdr_ref.compress(x, **kw))
            top = c.max(axis=-1).astype(np.float64)
            assert (np.diff(top) >= 0).all(), (kw, ratio, int(np.argmin(np.diff(top))))
            assert top.max() <= float(P) * (1 + 2.0 ** -23)
            c_far = host.steps((far[:, None] * F(ratio)).astype(F), **kw)[1]
            assert c_far.max(axis=-1).min() >= top[-1] - 6 * 2.0 ** -24 * float(P) and c_far.max() <= float(P) * (1 + 2.0 ** -23)
            for xx, cc in ((x, c), ((far[:, None] * F(ratio)).astype(F), c_far)):
                i, j = int(np.argmax(ratio)), int(np.argmin(ratio))
                ok = cc[:, j] >= F(2.0 ** -100)  # (normal floats: a denormal product has a larger relative rounding)
                before, after = xx[ok, j].astype(np.float64) / xx[ok, i], cc[ok, j].astype(np.float64) / cc[ok, i]
                assert np.abs(after / before - 1).max() <= 2.001 * 2.0 ** -24, (kw, ratio)
        grey = np.repeat(np.concatenate([m, far])[:, None], 3, axis=1)
        assert (np.diff(hdr_ref.pq_encode(host.nits(grey, **kw)[:, 1])) >= 0).all()
        half = host.frame(grey[None], **dict(kw, encoding=SCRGB16F))[0][0, :, 1].view(np.float16).astype(np.float64)
        assert (np.diff(half) >= 0).all()


# -- dither ------------------------------------------------------------------------------------------------------------------------------
def test_dither_is_seeded_and_its_mean_is_the_continuous_code(host):
    """A flat 64 x 64 field at the fractional position p inside code b: a TPDF-dithered quantiser's error has a standard deviation of at
    most half a code, so the mean of 4096 codes lies within 5 * 0.5 / sqrt(4096) = 0.039 of b + p - 0.5."""
    t = hdr_ref.thresholds().astype(np.float64)
    for b, p in ((594, 0.25), (153, 0.7), (769, 0.5), (1, 0.1), (1022, 0.9)):
        value = F(t[b - 1] + p * (t[b] - t[b - 1]))
        pos = (float(value) - t[b - 1]) / (t[b] - t[b - 1])
        nits = np.full((64, 64, 3), value, F)
        ref = hdr_ref.unpack_pq10(hdr_ref.pack_pq10(nits, 1.0, 3))
        got_words = host.pack_pq10(nits, dither=1.0, seed=3)
        got = hdr_ref.unpack_pq10(got_words)
        assert np.array_equal(got, ref) and (got_words >> 30 == 3).all()
        for c in range(3):
            assert abs(got[..., c].astype(np.float64).mean() - (b + pos - 0.5)) <= 5 * 0.5 / np.sqrt(4096), (b, p, c)
            assert set(np.unique(got[..., c])) <= {b - 1, b, b + 1}
        assert not np.array_equal(got[..., 0], got[..., 1])  # the channels take draws of their own
        assert np.array_equal(host.pack_pq10(nits, dither=1.0, seed=3), got_words)  # the same seed: the same words
        assert not np.array_equal(host.pack_pq10(nits, dither=1.0, seed=4), got_words)  # another seed: other words
        hard = host.pack_pq10(nits, dither=0.0, seed=3)
        assert np.array_equal(hdr_ref.unpack_pq10(hard), np.full((64, 64, 3), b)) and np.array_equal(hard, host.pack_pq10(nits, dither=0.0, seed=4))
    ends = np.zeros((16, 16, 3), F)
    ends[:, 8:] = 10000.0
    assert np.array_equal(host.pack_pq10(ends, dither=1.0, seed=5), host.pack_pq10(ends, dither=0.0))  # codes 0 and 1023 are never dithered


# -- levels ------------------------------------------------------------------------------------------------------------------------------
def test_levels_equal_the_integer_definition(host):
    rng = np.random.default_rng(6)
    lin = np.exp(rng.normal(-1.0, 2.0, (37, 53, 3))).astype(F)
    for kw in SETTINGS[::3]:
        nits = host.nits(lin, **kw)
        q = (np.max(nits, axis=-1) * F(64)).astype(F).astype(np.uint64)  # the definition, written out
        want = {"max_q": int(q.max()), "sum_q": int(q.sum()), "max_cll": float(F(int(q.max()) / 64.0)), "max_fall": float(F(int(q.sum()) / (64.0 * q.size)))}
        got = host.frame(lin, **kw)[1]
        assert got == want == hdr_ref.levels(nits), kw
        assert got == host.frame(lin, **dict(kw, dither=0.0 if kw["encoding"] == SCRGB16F else 1.0 - kw["dither"]))[1]  # taken before the dither
    # one bright pixel in a black frame: max_cll is that pixel, max_fall its share of the frame
    lin = np.zeros((12, 20, 3), F)
    lin[7, 3] = (0.5, 1.0, 0.25)
    for enc in (PQ10, SCRGB16F):
        lv = host.frame(lin, encoding=enc)[1]
        pixel = float(host.nits(lin, encoding=enc)[7, 3].max())
        assert lv["max_cll"] == float(F(int(pixel * 64) / 64.0)) and abs(lv["max_cll"] - pixel) <= 1 / 64 and lv["sum_q"] == lv["max_q"]
        assert lv["max_fall"] == float(F(lv["max_q"] / (64.0 * 240))) and abs(lv["max_fall"] - lv["max_cll"] / 240) <= 1e-6 * lv["max_cll"]
    assert host.frame(lin, encoding=SCRGB16F)[1]["max_cll"] == 203.0  # paper white itself, below the knee
    assert host.frame(np.zeros((3, 3, 3), F))[1] == {"max_q": 0, "sum_q": 0, "max_cll": 0.0, "max_fall": 0.0}


# -- parameters, layouts, ABI ------------------------------------------------------------------------------------------------------------
def test_params_ok_accepts_and_refuses_at_each_ranges_ends(host):
    nan, inf = float("nan"), float("inf")
    good = [{}, {"paper_white": 1.0}, {"paper_white": 1000.0}, {"paper_white": 10000.0, "peak": 10000.0}, {"peak": 203.0}, {"peak": 10000.0}, {"knee": 0.0},
            {"knee": 0.95}, {"dither": 1.0}, {"seed": 0xffffffff}, {"encoding": SCRGB16F}, {"encoding": SCRGB16F, "dither": 0.0}]
    bad = [{"paper_white": v} for v in (0.999, 0.0, -1.0, 1000.5, 10001.0, nan, inf)] + [{"peak": v} for v in (202.99, 10000.5, nan, inf, -inf)] + \
          [{"knee": v} for v in (-0.001, 0.9501, 1.0, nan, inf)] + [{"dither": v} for v in (-0.001, 1.001, nan, inf)] + \
          [{"encoding": 2}, {"encoding": 0xffffffff}, {"flags": 1}, {"flags": 0x80000000}, {"encoding": SCRGB16F, "dither": 0.5}, {"encoding": SCRGB16F, "dither": 1.0}]
    for kw in good + bad:
        p = hdr_params(**kw)
        assert bool(host.L.hdr_params_ok(C.byref(p))) == hdr_ref.params_ok(**dict(hdr_ref.DEFAULTS, **kw)) == (kw in good), kw


def test_struct_layout_and_defaults(host):
    lay = np.zeros(14, np.uint32)
    host.L.hdr_layout(lay.ctypes.data)
    P, V = state.HdrParams, state.HdrLevels
    assert list(lay) == [C.sizeof(P), C.sizeof(V), P.peak_nits.offset, P.knee.offset, P.dither.offset, P.seed.offset, P.encoding.offset, P.flags.offset, P._pad.offset,
                         V.max_q.offset, V.max_cll.offset, V.max_fall.offset, state.HDR_PQ10, state.HDR_SCRGB16F]
    assert list(lay) == [32, 24, 4, 8, 12, 16, 20, 24, 28, 8, 12, 16, 0, 1] and (hdr_ref.PQ10, hdr_ref.SCRGB16F) == (0, 1)
    p = P()
    host.L.hdr_defaults(C.byref(p))
    got = {"paper_white": p.paper_white_nits, "peak": p.peak_nits, "knee": p.knee, "dither": p.dither, "seed": p.seed, "encoding": p.encoding, "flags": p.flags}
    assert got == hdr_ref.DEFAULTS == dict(state.HDR_DEFAULTS, encoding=state.HDR_ENCODINGS[state.HDR_DEFAULTS["encoding"]])
    assert got == {"paper_white": 203.0, "peak": 1000.0, "knee": 0.5, "dither": 0.0, "seed": 0, "encoding": 0, "flags": 0}
    sig = inspect.signature(R.State.display_hdr).parameters
    names = ("source", "exposure", "white", "shadows", "highlights", "bloom_intensity", "paper_white", "peak", "knee", "encoding", "dither", "seed", "levels",
             "sample_total")
    assert list(sig)[1:15] == list(names)
    assert [sig[k].default for k in names] == ["mean", None, None, None, None, 0.0, None, None, None, "pq10", None, None, False, None]
    words = np.array([[3 << 30 | 1023 << 20 | 512 << 10 | 1, 3 << 30]], np.uint32)
    assert state.hdr_unpack_pq10(words).tolist() == [[[1, 512, 1023], [0, 0, 0]]] and state.hdr_unpack_pq10(words).dtype == np.uint16


def test_libraries_export_the_hdr_display():
    lib = C.CDLL(_build.build_hip())
    assert hasattr(lib, "rsrt_display_hdr")
    assert hasattr(R.State, "display_hdr") and not hasattr(state.MultiState, "display_hdr")
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "Rust: pub fn rsrt_display_hdr(" in hdr
    assert "rsrt_display_hdr" in open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    cpp = open(os.path.join(util.ROOT, "include", "rsrt_state.hpp")).read()
    assert "display_hdr(" in cpp and "hdr_defaults()" in cpp


def test_hdr_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = sorted(n for n in md if "rt_display_hdr_kernel" in n)
    assert len(names) == 4 and [n[n.index("ILj"):n.index("EEv")] for n in names] == ["ILj0ELb0", "ILj0ELb1", "ILj1ELb0", "ILj1ELb1"], names  # <encoding, levels>
    reduce = [n for n in md if "rt_hdr_levels_kernel" in n]  # the one-workgroup sum of the workgroups' partial levels
    assert len(reduce) == 1
    for n in names + reduce:
        k = md[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k.get("sgpr_spill_count", 0) == 0, (n, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "hdr_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "hdr_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_hdr_compiles(tmp_path):
    build_cpp_demo(tmp_path)


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """hdr_host.cpp as a program of its own (-DHDR_HOST_MAIN) with -fsanitize=address,undefined: frames of special sums of 1 x 1 to 31 x 7
    through the whole pass in both encodings at every corner of the parameters, every threshold with its neighbours through the quantiser,
    the half conversion over every exponent.  On the CPU, outside Python."""
    exe = str(tmp_path / "hdr_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DHDR_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "hdr_host: ok" in r.stdout, r.stdout
