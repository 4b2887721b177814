"""The video pass without a GPU: the published arithmetic (include/rsrt_video.h), compiled for the CPU, against the numpy restatement the
GPU tests hold the kernels to (tests/video_ref.py), bit for bit and byte for byte, special values included; the continuous code against
the true curves; the codes the standards give; neutral greys, the round trip's error, the sitings, the dither and the layouts, with bounds
worked out in the tests' comments; the parameter checks, the ABI, the kernels' code objects, the C++ State, the YUV4MPEG2 writer and a
sanitizer run of the host program."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import colour_ref
import hdr_ref
import local_ref
import util
import video_ref as V
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

F = np.float32
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "video_host.cpp")
FRAMES = [(1, 1), (1, 2), (2, 1), (3, 3), (8, 32), (9, 33), (5, 67)]  # (h, w)
# every standard x depth the pass has, x layout x range x siting
COMBOS = [dict(standard=s, depth=d, layout=l, range=r, siting=g) for (s, d) in ((V.BT709, 8), (V.BT709, 10), (V.HDR10, 10))
          for l in (V.SEMIPLANAR, V.PLANAR) for r in (V.LIMITED, V.FULL) for g in (V.LEFT, V.CENTRE, V.TOPLEFT)]
HDR = dict(paper_white=203.0, peak=1000.0, knee=0.5)


def video_params(standard=V.BT709, depth=8, layout=V.SEMIPLANAR, range=V.LIMITED, siting=V.LEFT, dither=0.0, seed=0, flags=0):
    return state.VideoParams(standard, depth, layout, range, siting, dither, seed, flags)


def hdr_params(paper_white=203.0, peak=1000.0, knee=0.5, dither=0.0, seed=0, encoding=hdr_ref.PQ10, flags=0):
    return state.HdrParams(paper_white, peak, knee, dither, seed, encoding, flags, 0)


def colour_params(white=(1.0, 1.0, 1.0), strength=0.0, flags=0):
    return state.ColourParams((C.c_float * 3)(*white), strength, flags, (C.c_uint32 * 3)())


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def lut4_of(lut):
    """[n, n, n, 3] -> the n^3 nodes of 4 floats the header reads."""
    out = np.ones((lut.shape[0] ** 3, 4), F)
    out[:, :3] = lut.reshape(-1, 3)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("video") / "libvideo.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.video_code.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.video_signal_ycc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
    L.video_ycc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.video_reduce.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.video_frame_ycc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.video_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.video_input.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    L.video_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.video_params_ok.argtypes = [C.c_void_p]
    L.video_defaults.argtypes = [C.c_void_p]
    L.video_planes.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.video_planes.restype = C.c_uint64
    L.video_layout.argtypes = [C.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    class Host:
        @staticmethod
        def code(x, standard):
            x = np.ascontiguousarray(x, F)
            out = np.empty(x.shape, F)
            L.video_code(x.ctypes.data, x.size, standard, out.ctypes.data)
            return out

        @staticmethod
        def signal_ycc(x, standard):
            x = np.ascontiguousarray(x, F)
            e, yc = np.empty_like(x), np.empty_like(x)
            L.video_signal_ycc(x.ctypes.data, x.size // 3, standard, e.ctypes.data, yc.ctypes.data)
            return e, yc

        @staticmethod
        def ycc(e, standard):
            e = np.ascontiguousarray(e, F)
            out = np.empty_like(e)
            L.video_ycc(e.ctypes.data, e.size // 3, standard, out.ctypes.data)
            return out

        @staticmethod
        def reduce(c, siting):
            c = np.ascontiguousarray(c, F)
            h, w = c.shape
            out = np.empty(((h + 1) // 2, (w + 1) // 2), F)
            L.video_reduce(c.ctypes.data, h, w, siting, out.ctypes.data)
            return out

        @staticmethod
        def planes(w, h, **kw):
            out = np.zeros(14, np.uint64)
            p = video_params(**kw)
            n = L.video_planes(w, h, C.byref(p), out.ctypes.data)
            return int(n), [int(v) for v in out]

        @staticmethod
        def frame(e, **kw):
            """Steps 3 to 6 of E' [h, w, 3]: (bytes, (y, cb, cr))."""
            e = np.ascontiguousarray(e, F)
            h, w = e.shape[:2]
            p = video_params(**kw)
            out = np.zeros(Host.planes(w, h, **kw)[0], np.uint8)
            L.video_frame(e.ctypes.data, h, w, C.byref(p), out.ctypes.data)
            return out, V.unpack(out, h, w, p.depth, p.layout)

        @staticmethod
        def frame_ycc(yc, **kw):
            yc = np.ascontiguousarray(yc, F)
            h, w = yc.shape[:2]
            p = video_params(**kw)
            out = np.zeros(Host.planes(w, h, **kw)[0], np.uint8)
            L.video_frame_ycc(yc.ctypes.data, h, w, C.byref(p), out.ctypes.data)
            return out, V.unpack(out, h, w, p.depth, p.layout)

        @staticmethod
        def source(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, hdr=None):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            gain, b = (None if a is None else np.ascontiguousarray(a, F) for a in (gain, b))
            l4 = None if lut is None else lut4_of(lut)
            c, hp, lv = colour_params(white, strength), (None if hdr is None else hdr_params(**hdr)), state.HdrLevels()
            out = np.empty((h, w, 3), F)
            L.video_input(sums.ctypes.data, h, w, total, exposure, ptr(gain), intensity, ptr(b), C.byref(c), ptr(l4), 0 if lut is None else lut.shape[0],
                          None if hp is None else C.byref(hp), out.ctypes.data, C.byref(lv))
            return out, ({"max_q": lv.max_q, "sum_q": lv.sum_q, "max_cll": lv.max_cll, "max_fall": lv.max_fall} if hdr is not None else None)

        @staticmethod
        def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, hdr=None, **kw):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            gain, b = (None if a is None else np.ascontiguousarray(a, F) for a in (gain, b))
            l4 = None if lut is None else lut4_of(lut)
            c, hp, p = colour_params(white, strength), (None if hdr is None else hdr_params(**hdr)), video_params(**kw)
            out = np.zeros(Host.planes(w, h, **kw)[0], np.uint8)
            L.video_display(sums.ctypes.data, h, w, total, exposure, ptr(gain), intensity, ptr(b), C.byref(c), ptr(l4), 0 if lut is None else lut.shape[0],
                            None if hp is None else C.byref(hp), C.byref(p), out.ctypes.data, None)
            return out

    Host.L = L
    return Host


# -- the restatement, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_every_step_and_whole_frames_equal_the_numpy_restatement(host, h, w):
    """Frames of special sums (NaN, +-inf, -0, a negative, a denormal, 3e38 where there is room) with a white point, gains, bloom and, for
    BT.709, a LUT: step 1's channels, the signal, Y'CbCr, the reduced planes and every combination's bytes, with dither 0 and 1."""
    sums, _ = local_ref.synthetic(h, w, seed=3000 * h + w)
    rng = np.random.default_rng(h * 100 + w)
    gain = np.exp(rng.normal(0.0, 0.5, (h, w))).astype(F)
    b = np.exp(rng.normal(-2.0, 1.0, ((h + 1) // 2, (w + 1) // 2, 4))).astype(F)
    lut = colour_ref.bake(3, *colour_ref.CDLS["warm"])
    chain = dict(white=(1.3, 0.95, 0.6), gain=gain, intensity=0.5, b=b)
    for standard in (V.BT709, V.HDR10):
        extra = dict(hdr=HDR) if standard == V.HDR10 else dict(lut=lut, strength=0.75)
        x, lv = host.source(sums, 3, 0.37, **chain, **extra)
        want_x = V.source(sums, 3, 0.37, **chain, **extra)
        assert util.same_bits_or_nan(x, want_x)
        if standard == V.HDR10:
            assert lv == hdr_ref.levels(want_x)
        assert same(host.code(x, standard), V.code(x, standard))
        e, yc = host.signal_ycc(x, standard)
        assert same(e, V.signal(x, standard)) and same(yc, V.ycc(e, standard)) and np.isfinite(yc).all() and e.min() >= 0 and e.max() <= 1
        for siting in (V.LEFT, V.CENTRE, V.TOPLEFT):
            for k in (1, 2):
                assert same(host.reduce(yc[..., k], siting), V.reduce(yc[..., k], siting)), (standard, siting, k)
        for kw in (c for c in COMBOS if c["standard"] == standard):
            for dither, seed in ((0.0, 0), (1.0, 0x9e3779b9)):
                q = dict(kw, dither=dither, seed=seed)
                got = host.display(sums, 3, 0.37, **chain, **extra, **q)
                want, codes, _ = V.display(sums, 3, 0.37, **chain, **extra, **q)
                assert got.size == V.frame_bytes(h, w, **q) and np.array_equal(got, want), q
                for a, c in zip(V.unpack(got, h, w, **q), codes):
                    assert np.array_equal(a, c)


def test_special_values_reach_the_code_as_the_header_says(host):
    nan, inf = np.nan, np.inf
    x = np.array([nan, -inf, -1.0, -0.0, 0.0, 1e-45, 1e-30], F)
    for standard, end, n in ((V.BT709, 1.0, 255), (V.HDR10, 10000.0, 1023)):
        e = host.code(x, standard)
        assert same(e, V.code(x, standard)) and (e[:5] == 0).all() and not np.signbit(e[:5]).any() and (e[5:] >= 0).all() and (e[5:] < 1e-20).all()
        top = host.code(np.array([end, np.nextafter(F(end), F(inf)), 3e38, inf], F), standard)
        assert (top == n).all()
        assert host.code(np.array([np.nextafter(F(end), F(0))], F), standard)[0] <= n


# -- the continuous code --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standard", [V.BT709, V.HDR10])
def test_the_code_at_every_threshold_and_its_neighbours(host, standard):
    t, n, end = V.table(standard)
    below, above = np.nextafter(t, F(0)), np.nextafter(t, F(np.inf))
    x = np.stack([below, t, above], axis=-1).ravel()  # ascending: the thresholds are more than an ulp apart
    assert (np.diff(x) > 0).all()
    e = host.code(x, standard)
    assert same(e, V.code(x, standard))
    assert (np.diff(e) >= 0).all()  # monotone over every threshold
    b = np.searchsorted(t, x, side="right").astype(F)
    assert (e >= b - F(0.5)).all() and (e <= b + F(0.5)).all()
    assert (e.reshape(-1, 3)[:, 1] == np.arange(1, n + 1) - 0.5).all()  # at a threshold itself: the code's lower edge
    # inside each code at p in [1/8, 7/8]: rounding the continuous code gives the displays' own code
    for p in (0.125, 0.25, 0.5, 0.75, 0.875):
        edges = np.concatenate([[F(0)], t, [end]]).astype(np.float64)
        inside = (edges[:-1] + p * (edges[1:] - edges[:-1])).astype(F)
        codes = np.searchsorted(t, inside, side="right")
        assert np.array_equal(codes, np.arange(n + 1))
        assert np.array_equal(np.floor(host.code(inside, standard) + F(0.5)).astype(np.int64), codes), p
    # a dense sweep of the whole range: monotone, finite, inside its code
    sweep = np.sort(np.concatenate([np.linspace(0, float(end) * 1.01, 200001), np.geomspace(1e-8, float(end), 200001)])).astype(F)
    es = host.code(sweep, standard)
    bs = np.searchsorted(t, sweep, side="right").astype(F)
    assert np.isfinite(es).all() and (np.diff(es) >= 0).all() and (es >= bs - F(0.5)).all() and (es <= bs + F(0.5)).all() and es[0] == 0 and es[-1] == n


def test_the_codes_distance_from_the_true_curves(host):
    """Between two thresholds the code is the chord of the true curve g (in codes).  A chord over an interval of one code lies below a
    concave g by at most  max |g''| dx^2 / 8  with dx = 1 / g' the interval's width:  |g''| / (8 g'^2).  For sRGB above the toe,
    g(x) = 255 (1.055 x^(1/2.4) - 0.055):  g' = 255 * 1.055 / 2.4 * x^(1/2.4 - 1),  g'' = g' * (1/2.4 - 1) / x,  so the distance is
    (1 - 1/2.4) / (8 x g'), largest at the toe's end x0 = 0.0031308:  0.0072 of a code.  The toe itself is linear: no distance but f32's.
    The last half code is a piece of its own (half a code over [T[N - 1], end]) where the curve bends less still.  PQ has no closed form
    worth writing down: its bound is the same quantity taken from ST 2084's formula in float64, the largest sag of the true curve under the
    chord between a code's two true edges, over every code and both half codes at the ends; the first codes, where the curve leaves 0
    like x^0.16, holds the largest, 0.10 of a 10-bit code.  f32's share: an ulp of 255 or 1023 and the quotient's roundings, below
    2e-4 and 5e-4 of a code."""
    x0 = 0.0031308
    g1 = 255 * 1.055 / 2.4 * x0 ** (1 / 2.4 - 1)
    bound = (1 - 1 / 2.4) / (8 * x0 * g1)
    assert 0.0071 < bound < 0.0073  # "about 0.007 of an 8-bit code"
    x = np.sort(np.concatenate([np.linspace(0, 1, 400001), np.geomspace(1e-6, 1, 400001)])).astype(F)
    true = np.where(x.astype(np.float64) <= x0, 12.92 * x.astype(np.float64), 1.055 * x.astype(np.float64) ** (1 / 2.4) - 0.055) * 255
    err = np.abs(host.code(x, V.BT709).astype(np.float64) - true)
    print("sRGB: largest distance %.5f codes at x = %.6f (bound %.5f)" % (err.max(), x[err.argmax()], bound))
    assert err.max() <= bound + 2e-4
    assert err[x <= 0.0028].max() <= 2e-4  # the linear toe, below code 10, whose interval holds the toe's end
    edges = np.array([0.0] + [10000.0 * hdr_ref.eotf((j - 0.5) / 1023.0) for j in range(1, 1024)] + [10000.0])  # the codes' true edges
    at = np.array([0.0] + [j - 0.5 for j in range(1, 1024)] + [1023.0])  # ... and the continuous code there
    sag, probes = 0.0, []
    for k in range(1024):
        xs = edges[k] + (edges[k + 1] - edges[k]) * np.linspace(0, 1, 35)[1:-1]
        chord = at[k] + (at[k + 1] - at[k]) * (xs - edges[k]) / (edges[k + 1] - edges[k])
        sag = max(sag, max(abs(1023 * hdr_ref.oetf(v) - c) for v, c in zip(xs[::4] if 8 < k < 1000 else xs, chord[::4] if 8 < k < 1000 else chord)))
        probes.append(xs)
    assert sag < 0.125  # an eighth of a 10-bit step at the worst
    nits = np.concatenate(probes)[::3].astype(F)
    true = np.array([hdr_ref.oetf(v) for v in nits]) * 1023
    err = np.abs(host.code(nits, V.HDR10).astype(np.float64) - true)
    print("PQ: largest distance %.5f codes at %.6f nits (bound %.5f)" % (err.max(), nits[err.argmax()], sag))
    assert err.max() <= sag + 5e-4


# -- codes against the standards ------------------------------------------------------------------------------------------------------------
BARS = {"black": (0, 0, 0), "white": (1, 1, 1), "yellow": (1, 1, 0), "cyan": (0, 1, 1), "green": (0, 1, 0), "magenta": (1, 0, 1), "red": (1, 0, 0), "blue": (0, 0, 1)}


def standard_codes(rgb, standard, depth, rng):
    """BT.709 / BT.2020: E'Y, E'CB, E'CR from the luma coefficients, then the quantised digital representation
    D = INT((219 E'Y + 16) 2^(n - 8) + 0.5), INT((224 E'C + 128) 2^(n - 8) + 0.5), or the full-range INT((2^n - 1) E'Y + 0.5),
    INT((2^n - 1) E'C + 2^(n - 1) + 0.5).  In exact rationals where float64 would do for any other colour: the bars' full-range chroma is
    2^(n - 1) -+ (2^n - 1) / 2, a tie exactly, which float64's rounding of Kr + Kg decides by accident (the result agrees with float64 everywhere else)."""
    from fractions import Fraction
    kr, kb = {V.BT709: (Fraction("0.2126"), Fraction("0.0722")), V.HDR10: (Fraction("0.2627"), Fraction("0.0593"))}[standard]
    r, g, b = (Fraction(int(v)) for v in rgb)
    y = kr * r + (1 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    m, peak = 2 ** (depth - 8), 2 ** depth - 1
    rnd = lambda v: int((v + Fraction(1, 2)) // 1)  # noqa: E731
    if rng == V.LIMITED:
        return rnd((219 * y + 16) * m), rnd((224 * cb + 128) * m), rnd((224 * cr + 128) * m)
    return rnd(peak * y), min(peak, rnd(peak * cb + 2 ** (depth - 1))), min(peak, rnd(peak * cr + 2 ** (depth - 1)))


def test_black_white_and_the_colour_bars_give_the_standards_codes(host):
    assert standard_codes(BARS["red"], V.BT709, 8, V.LIMITED) == (63, 102, 240) and standard_codes(BARS["green"], V.BT709, 8, V.LIMITED) == (173, 42, 26)
    assert standard_codes(BARS["blue"], V.BT709, 8, V.LIMITED) == (32, 240, 118)
    for standard, depth in ((V.BT709, 8), (V.BT709, 10), (V.HDR10, 10)):
        end = 10000.0 if standard == V.HDR10 else 1.0
        for rng in (V.LIMITED, V.FULL):
            for name, rgb in BARS.items():
                x = np.full((2, 2, 3), rgb, F) * F(end)  # a constant picture: display white is the transfer's end, black its 0
                e, _ = host.signal_ycc(x, standard)
                assert np.array_equal(e, np.full((2, 2, 3), rgb, F))
                for siting in (V.LEFT, V.CENTRE, V.TOPLEFT):
                    kw = dict(standard=standard, depth=depth, layout=V.PLANAR, range=rng, siting=siting)
                    _, (y, cb, cr) = host.frame(e, **kw)
                    want = standard_codes(rgb, standard, depth, rng)
                    assert (y == want[0]).all() and (int(cb[0, 0]), int(cr[0, 0])) == want[1:], (name, kw, y[0, 0], cb[0, 0], cr[0, 0], want)
                    assert np.array_equal(V.frame(e, **kw)[0], host.frame(e, **kw)[0])
    _, (y, cb, cr) = host.frame(np.full((2, 2, 3), BARS["red"], F), layout=V.PLANAR)
    assert (int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])) == (63, 102, 240)


@pytest.mark.parametrize("standard,depth", [(V.BT709, 8), (V.BT709, 10), (V.HDR10, 10)])
def test_a_grey_ramp_has_exactly_neutral_chroma(host, standard, depth):
    """2 000 000 signals R' = G' = B' from 0 to 1, each filling a 2 x 1 quad of a one-row picture, so that under the centre siting a chroma
    sample is that one value's: both ranges, dither 0.  Y' misses the channel by a few ulp and the differences are a few 1e-8, four
    orders below half a code."""
    n = 2_000_000
    v = np.linspace(0.0, 1.0, n).astype(F)
    e = np.repeat(np.repeat(v, 2)[None, :, None], 3, axis=2)
    for rng in (V.LIMITED, V.FULL):
        _, (y, cb, cr) = host.frame(e, standard=standard, depth=depth, layout=V.PLANAR, range=rng, siting=V.CENTRE)
        mid = 128 << (depth - 8)
        assert cb.shape == (1, n) and (cb == mid).all() and (cr == mid).all()
        assert (np.diff(y[0].astype(np.int64)) >= 0).all() and y[0, 0] == (0 if rng == V.FULL else 16 << (depth - 8))
        assert y[0, -1] == ((1 << depth) - 1 if rng == V.FULL else 235 << (depth - 8))
    yc = V.ycc(e[0, ::2], standard)  # the numpy model holds the same at every point
    for rng in (V.LIMITED, V.FULL):
        for k in (1, 2):
            assert (V.quantise(*V.value(yc[:, k], depth, rng, True), F(0)) == mid).all()


@pytest.mark.parametrize("standard,depth,rng", [(V.BT709, 8, V.LIMITED), (V.BT709, 8, V.FULL), (V.BT709, 10, V.LIMITED), (V.HDR10, 10, V.LIMITED), (V.HDR10, 10, V.FULL)])
def test_the_round_trips_error_is_the_quantisers(host, standard, depth, rng):
    """Random colours, each constant over its 2 x 2 quad, centre siting, no dither: decoded in float64 by the standard's inverse, a channel
    misses the continuous R'G'B' by at most what half a luma code and half a chroma code make of it:
      R' = Y' + 2 (1 - Kr) Cr'                         ->  sY / 2 + (1 - Kr) sC
      B' = Y' + 2 (1 - Kb) Cb'                         ->  sY / 2 + (1 - Kb) sC
      G' = Y' - (Kr 2 (1 - Kr) Cr' + Kb 2 (1 - Kb) Cb') / Kg  ->  sY / 2 + (sC / 2) (Kr 2 (1 - Kr) + Kb 2 (1 - Kb)) / Kg
    with sY, sC the sizes of one luma and one chroma code in units of R'.  No colour in [0, 1]^3 reaches a clamp."""
    kr, kg, kb, db, dr = V.MATRIX[standard]
    n = 200_000
    rgb = np.random.default_rng(7).random((n, 3)).astype(F)
    rgb[:8] = list(BARS.values())
    e = np.repeat(np.repeat(rgb[None], 2, axis=0), 2, axis=1)  # [2, 2n, 3]
    _, (y, cb, cr) = host.frame(e, standard=standard, depth=depth, layout=V.PLANAR, range=rng, siting=V.CENTRE)
    assert cb.shape == (1, n) and np.array_equal(y[0], y[1]) and np.array_equal(y[0, ::2], y[0, 1::2])
    m, peak = 2 ** (depth - 8), 2 ** depth - 1
    if rng == V.LIMITED:
        sy, sc = 1 / (219 * m), 1 / (224 * m)
        yp, cbp, crp = (y[0, ::2] / m - 16.0) / 219, (cb[0] / m - 128.0) / 224, (cr[0] / m - 128.0) / 224
    else:
        sy = sc = 1 / peak
        yp, cbp, crp = y[0, ::2] / peak, (cb[0] - 128.0 * m) / peak, (cr[0] - 128.0 * m) / peak
    r, b = yp + dr * crp, yp + db * cbp
    g = (yp - kr * r - kb * b) / kg
    bounds = (sy / 2 + (1 - kr) * sc, sy / 2 + (sc / 2) * (kr * 2 * (1 - kr) + kb * 2 * (1 - kb)) / kg, sy / 2 + (1 - kb) * sc)
    errs = [np.abs(c - rgb[:, i].astype(np.float64)).max() for i, c in enumerate((r, g, b))]
    print("round trip, standard %d depth %d range %d: errors %s, bounds %s (8-bit codes)" % (standard, depth, rng, [round(v * 255, 4) for v in errs], [round(v * 255, 4) for v in bounds]))
    if (standard, depth, rng) == (V.BT709, 8, V.LIMITED):
        assert [round(v * 255, 3) for v in bounds] == [1.479, 0.955, 1.638]  # R, G, B in 8-bit codes
    for err, bound in zip(errs, bounds):
        assert err <= bound


# -- siting ---------------------------------------------------------------------------------------------------------------------------------
def test_the_sitings_weights_and_edges(host):
    rng = np.random.default_rng(3)
    for h, w in ((4, 6), (5, 7), (1, 1), (2, 9)):
        ch, cw = (h + 1) // 2, (w + 1) // 2
        flat = np.full((h, w), F(0.123456789))
        for siting in (V.LEFT, V.CENTRE, V.TOPLEFT):
            assert same(host.reduce(flat, siting), np.full((ch, cw), flat[0, 0]))  # a constant picture: the pixel's own value, bit for bit
        rows = np.repeat(rng.random((h, 1)).astype(F), w, axis=1)  # constant along x: LEFT is CENTRE
        assert same(host.reduce(rows, V.LEFT), host.reduce(rows, V.CENTRE))
        assert same(host.reduce(rows, V.CENTRE)[:, 0], ((rows[0::2, 0] + rows[np.minimum(np.arange(1, h + 1, 2), h - 1), 0]) * F(0.5)).astype(F))
    # one coloured column at x = 4 of an 8 x 12 picture: LEFT and TOPLEFT weigh it 1/2 at sample 2 (its own); a column at x = 5: 1/4 at samples 2 and 3
    for x, want in ((4, {2: 0.5}), (5, {2: 0.25, 3: 0.25}), (0, {0: 0.75}), (11, {5: 0.25})):
        c = np.zeros((8, 12), F)
        c[:, x] = 1
        for siting in (V.LEFT, V.TOPLEFT):
            got = host.reduce(c, siting)
            assert (got == np.array([want.get(i, 0.0) for i in range(6)], F)[None, :]).all(), (x, siting, got[0])
        assert (host.reduce(c, V.CENTRE) == np.array([0.5 if i == x // 2 else 0.0 for i in range(6)], F)[None, :]).all()
    # one coloured row: LEFT and CENTRE average the quad's two rows; TOPLEFT weighs 1/4 1/2 1/4 round row 2 cy (the edge row replicated)
    for y, left, top in ((4, {2: 0.5}, {2: 0.5}), (5, {2: 0.5}, {2: 0.25, 3: 0.25}), (0, {0: 0.5}, {0: 0.75}), (7, {3: 0.5}, {3: 0.25})):
        c = np.zeros((8, 12), F)
        c[y, :] = 1
        for siting, want in ((V.LEFT, left), (V.CENTRE, left), (V.TOPLEFT, top)):
            got = host.reduce(c, siting)
            assert (got == np.array([want.get(i, 0.0) for i in range(4)], F)[:, None]).all(), (y, siting, got[:, 0])
    # odd sizes replicate the last column and row: the same planes as the picture padded by its edge
    c = rng.random((5, 7)).astype(F)
    padded = np.pad(c, ((0, 1), (0, 1)), mode="edge")
    for siting in (V.LEFT, V.CENTRE, V.TOPLEFT):
        assert same(host.reduce(c, siting), host.reduce(padded, siting)) and host.reduce(c, siting).shape == (3, 4)
        assert same(host.reduce(c, siting), V.reduce(c, siting))


# -- dither ---------------------------------------------------------------------------------------------------------------------------------
def test_the_dither_is_seeded_stays_in_range_and_keeps_the_mean(host):
    rng = np.random.default_rng(11)
    e = rng.random((9, 33, 3)).astype(F)
    e[0, :8] = list(BARS.values())  # the ranges' ends
    for kw in COMBOS[::5]:
        q = dict(kw, dither=1.0)
        a, codes = host.frame(e, seed=5, **q)
        assert np.array_equal(a, host.frame(e, seed=5, **q)[0]) and not np.array_equal(a, host.frame(e, seed=6, **q)[0])
        hard = host.frame(e, **kw)[1]
        m, full = 1 << (kw["depth"] - 8), kw["range"] == V.FULL
        for i, (c, h0) in enumerate(zip(codes, hard)):
            lo, hi = (0, 256 * m - 1) if full else (16 * m, (235 if i == 0 else 240) * m)
            assert c.min() >= lo and c.max() <= hi and np.abs(c.astype(int) - h0.astype(int)).max() == 1
    # A flat picture over 4096 seeds.  With dither 1 the offset t = (u1 + u2) - 1 is triangular on (-1, 1); floor(v + 0.5 + t) then has the
    # mean v exactly and, whatever v's fraction, the variance 1/4 of a code squared (1/12 + 1/6): a standard error of 0.5 / sqrt(4096).
    seeds = 4096
    bound = 4 * 0.5 / np.sqrt(seeds)
    flat = np.full((2, 2, 3), (0.3137, 0.5519, 0.7321), F)
    yc = host.ycc(flat, V.BT709)
    for depth, rng_ in ((8, V.LIMITED), (10, V.FULL)):
        kw = dict(depth=depth, layout=V.PLANAR, range=rng_, siting=V.CENTRE, dither=1.0)
        total = [np.zeros((2, 2)), np.zeros((1, 1)), np.zeros((1, 1))]
        for seed in range(seeds):
            for t, c in zip(total, host.frame(flat, seed=seed, **kw)[1]):
                t += c
        want = [float(V.value(yc[0, 0, k], depth, rng_, k > 0)[0]) for k in range(3)]
        for t, v in zip(total, want):
            assert np.abs(t / seeds - v).max() <= bound, (depth, t / seeds, v, bound)


# -- layouts --------------------------------------------------------------------------------------------------------------------------------
def test_the_four_layouts_hold_the_same_codes(host):
    e = np.random.default_rng(5).random((9, 33, 3)).astype(F)
    for siting in (V.LEFT, V.CENTRE, V.TOPLEFT):
        for depth in (8, 10):
            semi, c0 = host.frame(e, depth=depth, layout=V.SEMIPLANAR, siting=siting, dither=0.5, seed=3)
            planar, c1 = host.frame(e, depth=depth, layout=V.PLANAR, siting=siting, dither=0.5, seed=3)
            assert all(np.array_equal(a, b) for a, b in zip(c0, c1)) and semi.size == planar.size == (9 * 33 + 2 * 5 * 17) * (2 if depth == 10 else 1)
            t = np.dtype("<u2") if depth == 10 else np.uint8
            words, flat = semi.view(t), planar.view(t)
            shift = 6 if depth == 10 else 0
            assert np.array_equal(words[:297], flat[:297].astype(np.uint32) << shift)  # P010: code << 6; NV12: the code
            assert np.array_equal(words[297::2], flat[297:297 + 85].astype(np.uint32) << shift) and np.array_equal(words[298::2], flat[297 + 85:].astype(np.uint32) << shift)
            assert flat.max() < (1 << depth)
        # 8 and 10 bits are the same picture: a 10-bit limited code is within one of four times the 8-bit code
        y8, y10 = host.frame(e, depth=8, siting=siting)[1][0], host.frame(e, depth=10, siting=siting)[1][0]
        assert np.abs(y10.astype(int) - 4 * y8.astype(int)).max() <= 2


def test_planes_against_sizes_computed_by_hand(host):
    #        w, h, depth, layout: bytes, offsets, pitches, widths, heights
    cases = [(4, 2, 8, V.SEMIPLANAR, 12, [0, 8, 0], [4, 4, 0], [4, 4, 0], [2, 1, 0]),
             (4, 2, 8, V.PLANAR, 12, [0, 8, 10], [4, 2, 2], [4, 2, 2], [2, 1, 1]),
             (5, 3, 8, V.SEMIPLANAR, 27, [0, 15, 0], [5, 6, 0], [5, 6, 0], [3, 2, 0]),
             (5, 3, 8, V.PLANAR, 27, [0, 15, 21], [5, 3, 3], [5, 3, 3], [3, 2, 2]),
             (5, 3, 10, V.SEMIPLANAR, 54, [0, 30, 0], [10, 12, 0], [5, 6, 0], [3, 2, 0]),
             (5, 3, 10, V.PLANAR, 54, [0, 30, 42], [10, 6, 6], [5, 3, 3], [3, 2, 2]),
             (1, 1, 8, V.PLANAR, 3, [0, 1, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1]),
             (1920, 1080, 8, V.SEMIPLANAR, 3110400, [0, 2073600, 0], [1920, 1920, 0], [1920, 1920, 0], [1080, 540, 0]),
             (1920, 1080, 10, V.PLANAR, 6220800, [0, 4147200, 5184000], [3840, 1920, 1920], [1920, 960, 960], [1080, 540, 540])]
    for w, h, depth, layout, n, off, pitch, width, height in cases:
        got, out = host.planes(w, h, depth=depth, layout=layout)
        assert (got, out[:3], out[3:6], out[6:9], out[9:12], out[12], out[13]) == (n, off, pitch, width, height, 2 if layout == V.SEMIPLANAR else 3, 2 if depth == 10 else 1), (w, h)
        assert state.video_planes(w, h, depth, layout) == (n, [(off[i], pitch[i], width[i], height[i]) for i in range(out[12])])
        assert V.frame_bytes(h, w, depth) == n
    assert host.planes(0, 4)[0] == 0 and host.planes(4, 0)[0] == 0 and host.planes(4, 4, depth=9)[0] == 0 and host.planes(4, 4, standard=V.HDR10)[0] == 0
    assert state.video_planes(5, 3, layout="p010")[0] == 54 and state.video_planes(5, 3, layout="i420")[0] == 27


# -- parameters, layouts, ABI ---------------------------------------------------------------------------------------------------------------
def test_params_ok_accepts_and_refuses_at_each_ranges_ends(host):
    nan, inf = float("nan"), float("inf")
    good = [{}, {"depth": 10}, {"standard": V.HDR10, "depth": 10}, {"layout": V.PLANAR}, {"range": V.FULL}, {"siting": V.CENTRE}, {"siting": V.TOPLEFT},
            {"dither": 1.0}, {"dither": 0.0}, {"seed": 0xffffffff}]
    bad = [{"standard": 2}, {"standard": 0xffffffff}, {"standard": V.HDR10}, {"standard": V.HDR10, "depth": 8}, {"depth": 0}, {"depth": 9}, {"depth": 12}, {"depth": 16},
           {"layout": 2}, {"range": 2}, {"siting": 3}, {"siting": 0xffffffff}, {"flags": 1}, {"flags": 0x80000000}] + \
          [{"dither": v} for v in (-0.001, 1.001, nan, inf, -inf)]
    for kw in good + bad:
        p = video_params(**kw)
        assert bool(host.L.video_params_ok(C.byref(p))) == V.params_ok(**dict(V.DEFAULTS, **kw)) == (kw in good), kw


def test_struct_layout_and_defaults(host):
    lay = np.zeros(18, np.uint32)
    host.L.video_layout(lay.ctypes.data)
    P = state.VideoParams
    assert list(lay[:8]) == [C.sizeof(P), P.depth.offset, P.layout.offset, P.range.offset, P.siting.offset, P.dither.offset, P.seed.offset, P.flags.offset]
    assert list(lay[:8]) == [32, 4, 8, 12, 16, 20, 24, 28] and lay[8] == 80
    assert list(lay[9:]) == [state.VIDEO_BT709, state.VIDEO_HDR10, state.VIDEO_SEMIPLANAR, state.VIDEO_PLANAR, state.VIDEO_LIMITED, state.VIDEO_FULL,
                             state.VIDEO_SITING_LEFT, state.VIDEO_SITING_CENTRE, state.VIDEO_SITING_TOPLEFT] == [0, 1, 0, 1, 0, 1, 0, 1, 2]
    assert (V.BT709, V.HDR10, V.SEMIPLANAR, V.PLANAR, V.LIMITED, V.FULL, V.LEFT, V.CENTRE, V.TOPLEFT) == (0, 1, 0, 1, 0, 1, 0, 1, 2)
    p = P()
    host.L.video_defaults(C.byref(p))
    got = {k: getattr(p, k) for k in ("standard", "depth", "layout", "range", "siting", "dither", "seed", "flags")}
    d = state.VIDEO_DEFAULTS
    assert got == V.DEFAULTS == {"standard": 0, "depth": 8, "layout": 0, "range": 0, "siting": 0, "dither": 0.0, "seed": 0, "flags": 0}
    assert got == dict(d, standard=state.VIDEO_STANDARDS[d["standard"]], layout=state.VIDEO_LAYOUTS[d["layout"]][0], range=state.VIDEO_RANGES[d["range"]],
                       siting=state.VIDEO_SITINGS[d["siting"]]) and state.VIDEO_LAYOUTS[d["layout"]][1] == d["depth"]
    assert state.VIDEO_LAYOUTS == V.LAYOUTS and state.VIDEO_STANDARDS == V.STANDARDS and state.VIDEO_RANGES == V.RANGES and state.VIDEO_SITINGS == V.SITINGS
    sig = inspect.signature(R.State.display_video).parameters
    names = ("source", "exposure", "white", "lut_strength", "shadows", "highlights", "bloom_intensity", "standard", "depth", "layout", "range", "siting", "dither", "seed",
             "paper_white", "peak", "knee", "levels", "sample_total")
    assert list(sig)[1:20] == list(names)
    assert [sig[k].default for k in names] == ["mean", None, None, None, None, None, 0.0, "bt709"] + [None] * 9 + [False, None]


def test_video_frame_views():
    for name, (layout, depth) in state.VIDEO_LAYOUTS.items():
        h, w = 3, 5
        rng = np.random.default_rng(depth + layout)
        y, cb, cr = (rng.integers(0, 1 << depth, s).astype(np.uint16) for s in ((h, w), (2, 3), (2, 3)))
        data = V.pack(y, cb, cr, depth, layout)
        f = state.VideoFrame(data, w, h, video_params(depth=depth, layout=layout))
        assert np.array_equal(f.y, y) and np.array_equal(f.cb, cb) and np.array_equal(f.cr, cr) and (f.width, f.height) == (w, h), name
        assert f.data is data and f.params.depth == depth


def test_libraries_export_the_video_pass():
    lib = C.CDLL(_build.build_hip())
    assert hasattr(lib, "rsrt_display_video")
    assert hasattr(C.CDLL(_build.build_host()), "rsrt_y4m_write")
    assert hasattr(R.State, "display_video") and not hasattr(state.MultiState, "display_video")
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "Rust: pub fn rsrt_display_video(" in hdr
    assert "rsrt_display_video" in open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    cpp = open(os.path.join(util.ROOT, "include", "rsrt_state.hpp")).read()
    assert "display_video(" in cpp and "video_defaults()" in cpp


def test_video_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = sorted(n for n in md if "rt_display_video_kernel" in n)
    # <standard, depth, siting, levels>: BT.709 at 8 and 10 bits, HDR10 at 10 with and without the levels, each at three sitings
    want = sorted("ILj%dELj%dELj%dELb%d" % (s, d, g, lv) for (s, d, lvs) in ((0, 8, (0,)), (0, 10, (0,)), (1, 10, (0, 1))) for g in (0, 1, 2) for lv in lvs)
    assert sorted(n[n.index("ILj"):n.index("EEv")] for n in names) == want, names
    for n in names:
        k = md[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k.get("sgpr_spill_count", 0) == 0, (n, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "video_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "video_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_video_compiles(tmp_path):
    build_cpp_demo(tmp_path)


# -- the YUV4MPEG2 writer -------------------------------------------------------------------------------------------------------------------
def read_y4m(path):
    """A parser of its own: (the header's fields, [(y, cb, cr) of every frame])."""
    raw = open(path, "rb").read()
    line, rest = raw.split(b"\n", 1)
    fields = line.decode().split(" ")
    assert fields[0] == "YUV4MPEG2"
    tags = {f[0]: f[1:] for f in fields[1:] if f[0] != "X"}
    w, h = int(tags["W"]), int(tags["H"])
    deep = tags["C"].endswith("p10")
    t = np.dtype("<u2" if deep else "u1")
    ch, cw = (h + 1) // 2, (w + 1) // 2
    n = (w * h + 2 * cw * ch) * t.itemsize
    frames = []
    while rest:
        assert rest[:6] == b"FRAME\n"
        v = np.frombuffer(rest[6:6 + n], t)
        assert v.size == w * h + 2 * cw * ch
        frames.append((v[:w * h].reshape(h, w), v[w * h:w * h + cw * ch].reshape(ch, cw), v[w * h + cw * ch:].reshape(ch, cw)))
        rest = rest[6 + n:]
    return fields, frames


def test_y4m_write_two_frames_and_read_them_back(host, tmp_path):
    rng = np.random.default_rng(9)
    tags = {(8, V.LEFT): "C420mpeg2", (8, V.CENTRE): "C420jpeg", (8, V.TOPLEFT): "C420mpeg2", (10, V.LEFT): "C420p10", (10, V.CENTRE): "C420p10", (10, V.TOPLEFT): "C420p10"}
    for (depth, siting), tag in tags.items():
        for full in (False, True):
            h, w = 7, 13
            kw = dict(depth=depth, layout=V.PLANAR, range=V.FULL if full else V.LIMITED, siting=siting)
            frames = [host.frame(rng.random((h, w, 3)).astype(F), **kw) for _ in range(2)]
            p = video_params(**kw)
            path = str(tmp_path / ("d%d_s%d_%d.y4m" % (depth, siting, full)))
            for i, (data, _) in enumerate(frames):
                f = state.VideoFrame(data, w, h, p)
                R.host.write_y4m(path, f, fps=(30000, 1001), append=i > 0)
            fields, got = read_y4m(path)
            assert fields[:7] == ["YUV4MPEG2", "W13", "H7", "F30000:1001", "Ip", "A1:1", tag], fields
            assert fields[7:] == ["XCOLORRANGE=" + ("FULL" if full else "LIMITED"), "XRSRT_SITING=" + ["LEFT", "CENTRE", "TOPLEFT"][siting], "XRSRT_STANDARD=BT709"]
            assert len(got) == 2
            for (_, codes), planes in zip(frames, got):
                assert all(np.array_equal(a, b) for a, b in zip(codes, planes))
    # refusals: the semi-planar layout, a wrong byte count, a frame rate of 0, an append to a file that is not there
    data, _ = host.frame(rng.random((4, 4, 3)).astype(F))
    L, path = R.host.lib(), os.fsencode(str(tmp_path / "no.y4m"))
    semi, planar = video_params(), video_params(layout=V.PLANAR)
    assert L.rsrt_y4m_write(path, 0, 4, 4, 30, 1, C.byref(semi), data.ctypes.data, data.nbytes) == 1
    assert L.rsrt_y4m_write(path, 0, 4, 4, 30, 1, C.byref(planar), data.ctypes.data, data.nbytes - 1) == 1
    assert L.rsrt_y4m_write(path, 0, 4, 4, 0, 1, C.byref(planar), data.ctypes.data, data.nbytes) == 1
    assert L.rsrt_y4m_write(path, 0, 4, 4, 30, 1, None, data.ctypes.data, data.nbytes) == 1
    assert not os.path.exists(path)
    assert L.rsrt_y4m_write(path, 1, 4, 4, 30, 1, C.byref(planar), data.ctypes.data, data.nbytes) == 2 and not os.path.exists(path)
    with pytest.raises(ValueError):
        R.host.write_y4m(str(tmp_path / "no.y4m"), state.VideoFrame(data, 4, 4, semi))


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """video_host.cpp as a program of its own (-DVIDEO_HOST_MAIN) with -fsanitize=address,undefined: frames of special sums of 1 x 1 to
    31 x 7 through the whole pass at every combination of the parameters.  On the CPU, outside Python."""
    exe = str(tmp_path / "video_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DVIDEO_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "video_host: ok" in r.stdout, r.stdout
