"""White balance and colour grading without a GPU: the published arithmetic (include/rsrt_colour.h), compiled for the CPU, against the
numpy restatement the GPU tests hold the kernels to (tests/colour_ref.py), bit for bit, special pixels included: the chroma histogram,
the white point, baked LUTs, the interpolation and the display bytes; the integer log2's accuracy; the scaling invariances; tint
recovery on rendered frames; an independent float64 reading; rsrt_colour_pow against float64 pow; the display identities; the
parameter checks, the ABI, the kernels' code objects, the C++ State, and a sanitizer run of the host program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_ref
import colour_ref
import exposure_ref
import local_ref
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (5, 7), (4, 64), (37, 70)]
F = np.float32
WHITE_SETS = [{}, {"gate": 1}, {"gate": 31}, {"iterations": 0}, {"iterations": 8}, {"min_permille": 1000}, {"strength": 0.5}, {"max_stops": 0.25},
              {"blend": 0.0, "previous": (1.2, 0.9, 0.7)}, {"blend": 0.25, "previous": (1.2, 0.9, 0.7)}, {"blend": 1.0, "previous": (1.2, 0.9, 0.7)},
              {"min_permille": 1000, "previous": (0.5, 1.0, 2.0)}]
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "colour_host.cpp")


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def seed_of(h, w):
    return 2000 * h + w


def white_params(**kw):
    q = dict(colour_ref.WHITE_DEFAULTS, **kw)
    return state.WhiteParams(q["gate"], q["iterations"], q["min_permille"], q["strength"], q["max_stops"], q["blend"], (C.c_float * 3)(*q["previous"]),
                             q.get("flags", 0))


def colour_params(white=(1.0, 1.0, 1.0), strength=0.0, flags=0):
    return state.ColourParams((C.c_float * 3)(*white), strength, flags, (C.c_uint32 * 3)())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("colour") / "libcolour.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.colour_hist.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.colour_ilog2.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.colour_white.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.colour_log2.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.colour_pow.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.colour_bake.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    L.colour_lut_at.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    L.colour_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    for n in ("colour_white_params_ok", "colour_cdl_params_ok", "colour_params_ok"):
        getattr(L, n).argtypes = [C.c_void_p]
    L.colour_lut_size_ok.argtypes = [C.c_uint32]
    L.colour_defaults.argtypes = [C.c_void_p] * 4
    L.colour_layout.argtypes = [C.c_void_p]

    def lut4(lut):
        """[n, n, n, 3] -> the device's n^3 x 4 floats."""
        return np.ascontiguousarray(np.concatenate([np.asarray(lut, F), np.ones(lut.shape[:3] + (1,), F)], axis=-1))

    class Host:
        @staticmethod
        def histogram(sums, total):
            sums = np.ascontiguousarray(sums, F)
            out = np.full(colour_ref.WORDS, 7, np.uint32)
            L.colour_hist(sums.ctypes.data, sums.size // 4, total, out.ctypes.data)
            return out

        @staticmethod
        def ilog2(x):
            x = np.ascontiguousarray(x, F)
            out = np.empty(x.shape, np.int32)
            L.colour_ilog2(x.ctypes.data, x.size, out.ctypes.data)
            return out

        @staticmethod
        def white(hist, **kw):
            hist = np.ascontiguousarray(hist, np.uint32)
            p, r = white_params(**kw), state.WhiteResult()
            L.colour_white(hist.ctypes.data, C.byref(p), C.byref(r))
            return {"white": F(list(r.white)), "target": F(list(r.target)), "illuminant": F(list(r.illuminant)), "eu": F(r.eu), "ev": F(r.ev),
                    "gated": r.gated, "counted": r.counted, "skipped": r.skipped, "estimated": bool(r.estimated)}

        @staticmethod
        def log2(x):
            x = np.ascontiguousarray(x, F)
            out = np.empty_like(x)
            L.colour_log2(x.ctypes.data, x.size, out.ctypes.data)
            return out

        @staticmethod
        def pow(x, p):
            x = np.ascontiguousarray(x, F)
            out = np.empty_like(x)
            L.colour_pow(x.ctypes.data, x.size, p, out.ctypes.data)
            return out

        @staticmethod
        def bake(n, slope=1.0, offset=0.0, power=1.0, saturation=1.0):
            p = state.CdlParams.of(slope, offset, power, saturation)
            out = np.full((n, n, n, 4), 7, F)
            L.colour_bake(n, C.byref(p), out.ctypes.data)
            assert (out[..., 3] == 1).all()
            return out[..., :3].copy()

        @staticmethod
        def lut_at(lut, enc):
            l4, enc = lut4(lut), np.ascontiguousarray(enc, F)
            out = np.empty_like(enc)
            L.colour_lut_at(l4.ctypes.data, lut.shape[0], enc.ctypes.data, enc.size // 3, out.ctypes.data)
            return out

        @staticmethod
        def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            out = np.zeros((h, w, 4), np.uint8)
            gain = None if gain is None else np.ascontiguousarray(gain, F)
            b = None if b is None else np.ascontiguousarray(b, F)
            l4 = None if lut is None else lut4(lut)
            c = colour_params(white, strength)
            L.colour_display(sums.ctypes.data, h, w, total, exposure, None if gain is None else gain.ctypes.data, intensity, None if b is None else b.ctypes.data,
                             C.byref(c), None if l4 is None else l4.ctypes.data, 0 if lut is None else lut.shape[0], out.ctypes.data)
            return out
    Host.L = L
    return Host


def same_white(a, b):
    return (all(same(a[k], b[k]) for k in ("white", "target", "illuminant", "eu", "ev"))
            and all(a[k] == b[k] for k in ("gated", "counted", "skipped", "estimated")))


# -- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_histogram_and_white_point_match_numpy_bit_for_bit(host, h, w):
    sums, special = colour_ref.chroma_frame(h, w, seed=seed_of(h, w))
    assert bool(special) == (h * w >= 16)
    for total in (1, 3):
        hist = host.histogram(sums, total)
        assert np.array_equal(hist, colour_ref.histogram(sums, total)) and int(hist.sum()) == h * w
        word = colour_ref.words(sums, total).ravel()
        if special:  # skipped or counted as documented
            for name in ("zero_channel", "minus_one", "nan", "black", "neg_zero"):
                assert word[special[name]] == colour_ref.BINS, name
            assert word[special["inf"]] // 64 == 0  # +inf in blue is counted: the lowest v, an edge bin
            assert word[special["denormal"]] % 64 == 63  # a denormal red is counted: the highest u
        if h * w > 1000:  # chroma over +-3 octaves: the edge bins fill
            g = hist[:colour_ref.BINS].reshape(64, 64)
            assert g[0].sum() and g[63].sum() and g[:, 0].sum() and g[:, 63].sum()
        for kw in WHITE_SETS:
            got, want = host.white(hist, **kw), colour_ref.from_histogram(hist, **kw)
            assert same_white(got, want), (total, kw, got, want)
            if kw.get("min_permille") == 1000 and hist[colour_ref.BINS]:  # refuses: the previous white point, or 1
                assert not got["estimated"] and same(got["white"], F(kw.get("previous", (1, 1, 1))))
        base = host.white(hist, previous=(1.2, 0.9, 0.7))
        assert same(host.white(hist, blend=0.0, previous=(1.2, 0.9, 0.7))["white"], F([1.2, 0.9, 0.7]))
        assert np.abs(base["white"] / base["target"] - 1).max() <= 2.0 ** -22  # blend 1: the target, to the rounding of previous + (target - previous)


def test_degenerate_frames(host):
    zeros = np.zeros((9, 13, 4), F)
    hist = host.histogram(zeros, 1)
    assert hist[colour_ref.BINS] == 9 * 13 and hist[:colour_ref.BINS].sum() == 0 and np.array_equal(hist, colour_ref.histogram(zeros, 1))
    for kw in ({}, {"min_permille": 0}, {"iterations": 0, "min_permille": 0}):
        r = host.white(hist, **kw)
        assert not r["estimated"] and same(r["white"], F([1, 1, 1])) and same_white(r, colour_ref.from_histogram(hist, **kw))
    const = np.ones((7, 11, 4), F)
    const[..., :3] = (0.3, 0.2, 0.1)
    hist = host.histogram(const, 1)
    assert np.count_nonzero(hist) == 1 and hist.max() == 77 and np.array_equal(hist, colour_ref.histogram(const, 1))  # exactly one word
    r = host.white(hist)
    assert r["estimated"] and r["gated"] == 77 and same_white(r, colour_ref.from_histogram(hist))
    assert abs(float(r["eu"]) - np.log2(0.2 / 0.3)) <= 1 / 32 + 0.008 and abs(float(r["ev"]) - np.log2(0.2 / 0.1)) <= 1 / 32 + 0.008


def test_ilog2_is_within_0_008_octave_over_every_mantissa(host):
    x = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3f800000)).view(F)
    got = colour_ref.ilog2(x)
    err = np.abs(got / 65536.0 - np.log2(x.astype(np.float64)))
    print("rsrt_colour_ilog2: largest error %.5f octave over 2^23 mantissas" % err.max())
    assert err.max() <= 0.008
    pick = np.concatenate([x[::4099], F([1e-41, 1e-30, 3e38, np.inf, 2.0 ** -126, 0.18, 1.0])])
    assert np.array_equal(host.ilog2(pick), colour_ref.ilog2(pick))
    assert [int(v) for v in colour_ref.ilog2(F([0.25, 1.0, 8.0, np.inf]))] == [-2 * 65536, 0, 3 * 65536, 128 * 65536]  # exact at powers of two


# -- the invariances -----------------------------------------------------------------------------------------------------------------
def test_uniform_power_of_two_scaling_leaves_the_histogram(host):
    sums, _ = colour_ref.chroma_frame(37, 70, seed=5, specials=False)
    want = host.histogram(sums, 1)
    for k in (-9, -1, 1, 6):
        scaled = sums.copy()
        scaled[..., :3] *= F(2.0 ** k)
        assert np.array_equal(host.histogram(scaled, 1), want), k
    assert np.array_equal(host.histogram(sums, 4), want)  # (and so does a power-of-two total)


def test_a_power_of_two_tint_shifts_the_histogram_by_16_bins_an_octave(host):
    sums = colour_ref.near_grey_frame(37, 70, seed=6, saturated=0.0)
    h0 = host.histogram(sums, 1)[:colour_ref.BINS].reshape(64, 64)
    tinted = sums.copy()
    tinted[..., :3] *= F([2, 1, 0.5])
    h1 = host.histogram(tinted, 1)[:colour_ref.BINS].reshape(64, 64)
    assert h0[:, :17].sum() == 0 and h0[48:, :].sum() == 0  # nothing is pushed onto a clamped edge
    assert np.array_equal(h1[16:, :48], h0[:48, 16:])  # u = log2 G/R falls an octave, v = log2 G/B rises one


_rendered = {}


def rendered(name):
    """The oracle's render of a scene at 96 x 54 and 16 spp under the synthetic environment: sums [54, 96, 4]."""
    if name not in _rendered:
        sc = R.Scene.load_toml(util.scene_path(name))
        acc, _ = oracle.render(util.oracle_scene(sc), util.oracle_env(util.small_env()), sc.camera_uniform().view(oracle.CAMERA), 96, 54, 0, 16, 8, fast=True)
        acc.setflags(write=False)
        _rendered[name] = acc
    return _rendered[name]


def estimate(host, sums, total, **kw):
    r = host.white(host.histogram(sums, total), **kw)
    assert r["estimated"]
    return r


@pytest.mark.parametrize("name", ["house", "default"])
def test_tints_are_recovered_on_rendered_frames(host, name):
    """A power-of-two tint moves the estimate by exactly an octave a channel (no counted pixel of the window meets a clamped edge
    bin); any other tint moves (eu, ev) by log2 of it within half a bin, 1 / 32 octave.  The gated share stays above min_permille."""
    acc = rendered(name)
    base = estimate(host, acc, 16)
    assert same_white(base, colour_ref.from_histogram(colour_ref.histogram(acc, 16)))
    share = base["gated"] / (54 * 96)
    print("%s: eu %+.4f ev %+.4f, gated share %.3f, white %s" % (name, base["eu"], base["ev"], share, base["white"]))
    assert share > 0.5
    t = acc.copy()
    t[..., :3] *= F([2, 1, 0.5])
    r = estimate(host, t, 16)
    (n0, su0, sv0), w0 = colour_ref.final_window(colour_ref.histogram(acc, 16))
    (n1, su1, sv1), w1 = colour_ref.final_window(colour_ref.histogram(t, 16))
    assert (n1, su1, sv1) == (n0, su0 - 32 * n0, sv0 + 32 * n0) == (r["gated"], su1, sv1)  # exactly an octave a channel, in the integers
    assert w1 == ((w0[0][0] - 16, w0[0][1] + 16), (w0[1][0] - 16, w0[1][1] + 16))
    assert abs(float(r["eu"]) - (float(base["eu"]) - 1)) <= 2.0 ** -22 and abs(float(r["ev"]) - (float(base["ev"]) + 1)) <= 2.0 ** -22  # (eu is one f32 division)
    for tint in ((1.7, 1, 0.55), (0.6, 1, 1.8)):
        t = acc.copy()
        t[..., :3] *= F(tint)
        r = estimate(host, t, 16)
        du, dv = float(r["eu"]) - float(base["eu"]) + np.log2(tint[0]), float(r["ev"]) - float(base["ev"]) + np.log2(tint[2])
        print("%s tint %s: error %+.4f %+.4f octave, gated share %.3f" % (name, tint, du, dv, r["gated"] / (54 * 96)))
        assert abs(du) <= 1 / 32 and abs(dv) <= 1 / 32 and r["gated"] / (54 * 96) > 0.5
        # ... and the white point takes the tint back out: the balanced frames agree in chroma
        with np.errstate(all="ignore"):
            back = t[..., :3] * r["white"] / (acc[..., :3] * base["white"])
        ok = np.isfinite(back).all(axis=-1)
        ratio = np.median(back[ok], axis=0)
        assert np.abs(np.log2(ratio / ratio[1])).max() <= 1 / 16


def test_the_estimate_agrees_with_an_independent_float64_reading(host):
    """Synthetic near-grey frames with 35 % saturated pixels under tints up to (2.5, 1, 0.4): the estimate against the float64 mean, with
    true log2, of the near-grey pixels' chroma: within 1 / 32 octave (the integer log2 is within 0.0077, a bin's centre within 1 / 32 of
    a pixel but unbiased over a spread of 0.4 octave, and the window's cut of the near-grey cluster's tails is symmetric)."""
    worst = 0.0
    rng = np.random.default_rng(77)
    for seed in range(30):
        tint = (2.0 ** rng.uniform(-1.32, 1.32), 1.0, 2.0 ** rng.uniform(-1.32, 1.32)) if seed else (2.5, 1.0, 0.4)
        sums = colour_ref.near_grey_frame(40, 60, seed=100 + seed, tint=tint)
        r = estimate(host, sums, 1)
        c = sums[..., :3].astype(np.float64)
        u, v = np.log2(c[..., 1] / c[..., 0]), np.log2(c[..., 1] / c[..., 2])
        grey = (np.abs(u + np.log2(tint[0])) <= 0.4) & (np.abs(v + np.log2(tint[2])) <= 0.4)  # the near-grey surfaces: chroma within 0.4 of the tint's
        assert 0.6 < grey.mean() < 0.7
        err = max(abs(float(r["eu"]) - u[grey].mean()), abs(float(r["ev"]) - v[grey].mean()))
        worst = max(worst, err)
        assert err <= 1 / 32, (seed, tint, err)
    print("independent reading: worst |estimate - float64 mean| %.4f octave over 30 frames" % worst)


# -- the LUT -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 17])
def test_baked_luts_match_numpy_bit_for_bit(host, n):
    for name, cdl in colour_ref.CDLS.items():
        got, want = host.bake(n, *cdl), colour_ref.bake(n, *cdl)
        assert same(got, want), name
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
        if name == "identity":  # exactly i / (n - 1)
            ramp = (np.arange(n).astype(F) / F(n - 1)).astype(F)
            assert same(got[..., 0], np.broadcast_to(ramp, (n, n, n))) and same(got[..., 2], np.broadcast_to(ramp[:, None, None], (n, n, n)))
        else:
            assert not same(got, colour_ref.bake(n))


# the worst encoded-domain error of the bake against float64 pow over every node of the 33^3 LUTs of colour_ref.CDLS, measured on the CPU
# (DESIGN.md §20): 2.38e-5 for "warm", at a node near black where the saturation step's Y + s * (x - Y) cancels and the square root of the
# encoding magnifies what is left of rsrt_colour_pow's 4e-6 relative error; 1.3e-6 for the others.  The test asserts twice that
POW_MEASURED = 2.39e-5


def test_colour_pow_against_float64_pow_on_every_node_of_33_cubed(host):
    x = np.concatenate([F([0, 1e-45, 1e-41, 1.17549435e-38, 1e-30, 1e-10, 0.5, 0.99999994, 1.0]), np.linspace(0, 1, 4097).astype(F)])
    for p in (0.25, 0.9, 1.0, 2.2, 4.0):
        assert same(host.pow(x, p), colour_ref.pow_(x, p)), p
    assert same(host.pow(F([1.0, 0.0]), 3.3), F([1, 0]))
    norm = np.linspace(0.001, 1, 5000).astype(F)
    assert same(host.log2(norm), colour_ref.log2(norm)) and np.abs(host.log2(norm) - np.log2(norm.astype(np.float64))).max() <= 2e-6
    worst = 0.0
    n = 33
    for name, (slope, offset, power, sat) in colour_ref.CDLS.items():
        got = host.bake(n, slope, offset, power, sat).astype(np.float64)
        want = colour_ref.bake(n, slope, offset, power, sat, pow_fn=colour_ref.pow_f64).astype(np.float64)  # the same bake, float64 pow in rsrt_colour_pow's place
        err = np.abs(got - want).max()
        print("33^3 bake of %s against float64 pow: largest encoded error %.3g" % (name, err))
        worst = max(worst, err)
    print("rsrt_colour_pow: worst encoded-domain error %.3g" % worst)
    assert worst <= 2 * POW_MEASURED and worst < 1 / 1024


def test_tetrahedral_interpolation(host):
    rng = np.random.default_rng(3)
    for n in (2, 3, 17):
        lut = colour_ref.bake(n, *colour_ref.CDLS["warm"])
        ramp = (np.arange(n).astype(F) / F(n - 1)).astype(F)
        ib, ig, ir = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        nodes = np.stack([ramp[ir], ramp[ig], ramp[ib]], axis=-1).reshape(-1, 3)
        assert same(host.lut_at(lut, nodes), lut.reshape(-1, 3))  # exact at the nodes, 0 and 1 included
        enc = np.concatenate([rng.random((4000, 3)).astype(F), nodes, F([[0, 0, 0], [1, 1, 1], [1, 0, 1], [0.5, 0.5, 0.5], [0.25, 0.5, 0.25], [1e-41, 1, 0.99999994]])])
        enc[:200, 1] = enc[:200, 0]  # ties
        enc[200:400, 2] = enc[200:400, 1]
        got = host.lut_at(lut, enc)
        assert same(got, colour_ref.lut_at(lut, enc))
        # an affine LUT is reproduced to a few ulp everywhere
        m, c = np.array([[0.5, 0.2, 0.1], [0.1, 0.6, 0.05], [0.05, 0.1, 0.7]]), np.array([0.05, 0.02, 0.1])
        affine = (nodes.astype(np.float64) @ m.T + c).astype(F).reshape(n, n, n, 3)
        err = np.abs(host.lut_at(affine, enc).astype(np.float64) - (enc.astype(np.float64) @ m.T + c)).max()
        print("n %d: affine LUT, largest interpolation error %.3g" % (n, err))
        assert err <= 8 * 2.0 ** -24  # the nodes' rounding (half an ulp of 1 each, weights summing to 1) and seven f32 operations
        assert same(host.lut_at(colour_ref.bake(n), nodes), nodes)


# -- the display ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_display_pixels_match_numpy_byte_for_byte(host, h, w):
    sums, _ = local_ref.synthetic(h, w, seed=seed_of(h, w))
    total, exposure = 3, 0.37
    b = bloom_ref.bloom(sums, total, exposure, 3)
    grid = local_ref.grid_of(sums, total, 8)
    gain = local_ref.gains(sums, total, exposure, grid, 8)
    white = (1.3, 0.95, 0.6)
    for n in (2, 3, 17):
        lut = colour_ref.bake(n, *colour_ref.CDLS["warm"])
        for strength in (0.0, 0.5, 1.0):
            for g in (None, gain):
                for intensity in (0.0, 0.5):
                    case = (n, strength, g is not None, intensity)
                    got = host.display(sums, total, exposure, white, lut, strength, g, intensity, b)
                    assert np.array_equal(got, colour_ref.display(sums, total, exposure, white, lut, strength, g, intensity, b)), case
    nan = np.ones((1, 2, 4), F)
    nan[0, 0, 1] = np.nan
    for strength in (0.0, 1.0):  # a NaN channel gives byte 0
        got = host.display(nan, 1, 1.0, (1, 1, 1), colour_ref.bake(2), strength)
        assert list(got[0, 0]) == [0, 0, 0, 255] and got[0, 1, 0] > 0


@pytest.mark.parametrize("h,w", FRAMES)
def test_display_identities(host, h, w):
    sums, _ = local_ref.synthetic(h, w, seed=seed_of(h, w))
    total, exposure = 3, 0.37
    b = bloom_ref.bloom(sums, total, exposure, 2)
    gain = local_ref.gains(sums, total, exposure, local_ref.grid_of(sums, total, 8), 8)
    # white 1 and strength 0: the local, the bloomed and the exposed display
    assert np.array_equal(host.display(sums, total, exposure, gain=gain, intensity=0.5, b=b), local_ref.display(sums, total, exposure, gain, 0.5, b))
    assert np.array_equal(host.display(sums, total, exposure, gain=gain), local_ref.display(sums, total, exposure, gain))
    assert np.array_equal(host.display(sums, total, exposure, intensity=0.5, b=b), bloom_ref.display(sums, total, exposure, 0.5, b))
    plain = exposure_ref.display(sums, total, exposure)
    assert np.array_equal(host.display(sums, total, exposure), plain)
    # an identity LUT moves no byte by more than 1
    for n in (2, 3, 17, 33):
        graded = host.display(sums, total, exposure, lut=colour_ref.bake(n), strength=1.0)
        d = np.abs(graded.astype(int) - plain.astype(int))
        assert d.max() <= 1, n
    # white (2, 1, 0.5) at exposure 1: the exposed display of the frame multiplied by the same exact factors (on a frame whose means
    # are normal binary16 numbers with room for the factor: the binary16 rounding commutes with a power of two only there)
    mid = np.ones((h, w, 4), F)
    mid[..., :3] = np.exp(np.random.default_rng(seed_of(h, w)).normal(-1.0, 1.5, (h, w, 3))).astype(F)
    tinted = mid.copy()
    tinted[..., :3] *= F([2, 1, 0.5])
    assert np.array_equal(host.display(mid, 1, 1.0, (2.0, 1.0, 0.5)), exposure_ref.display(tinted, 1, 1.0))


# -- parameters, layouts, ABI --------------------------------------------------------------------------------------------------------
def test_params_ok_accept_and_reject(host):
    nan, inf = float("nan"), float("inf")
    good = [{}, {"gate": 1}, {"gate": 31}, {"iterations": 0}, {"iterations": 8}, {"min_permille": 0}, {"min_permille": 1000}, {"strength": 0.0}, {"max_stops": 0.0},
            {"max_stops": 4.0}, {"blend": 0.0}, {"previous": (0.5, 1.0, 3e38)}, {"previous": (-0.0, 0.0, 0.0)}]
    bad = [{"gate": 0}, {"gate": 32}, {"iterations": 9}, {"min_permille": 1001}, {"flags": 1}, {"previous": (0.0, 1.0, 1.0)}, {"previous": (1.0, 1.0, -1.0)},
           {"previous": (1.0, nan, 1.0)}, {"previous": (inf, 1.0, 1.0)}]
    bad += [{k: v} for k in ("strength", "blend") for v in (-0.001, 1.001, nan, inf)] + [{"max_stops": v} for v in (-0.5, 4.5, nan, inf)]
    for kw in good:
        p = white_params(**kw)
        assert host.L.colour_white_params_ok(C.byref(p)) and colour_ref.white_params_ok(**dict(colour_ref.WHITE_DEFAULTS, **kw)), kw
    for kw in bad:
        p = white_params(**kw)
        assert not host.L.colour_white_params_ok(C.byref(p)) and not colour_ref.white_params_ok(**dict(colour_ref.WHITE_DEFAULTS, **kw)), kw
    good = [{}, {"slope": 0.0}, {"slope": 16.0}, {"offset": -1.0}, {"offset": 1.0}, {"power": 0.25}, {"power": 4.0}, {"saturation": 0.0}, {"saturation": 4.0},
            {"slope": (0.5, 1.0, 2.0)}]
    bad = [{"slope": v} for v in (-0.1, 16.5, nan, inf, (1.0, 1.0, 17.0))] + [{"offset": v} for v in (-1.5, 1.5, nan, (0.0, nan, 0.0))]
    bad += [{"power": v} for v in (0.2, 4.5, 0.0, nan, inf, (1.0, 0.1, 1.0))] + [{"saturation": v} for v in (-0.1, 4.5, nan, inf)] + [{"flags": 1}]
    for kw in good + bad:
        p = state.CdlParams.of(**kw)
        q = dict(colour_ref.CDL_DEFAULTS, **kw)
        assert bool(host.L.colour_cdl_params_ok(C.byref(p))) == colour_ref.cdl_params_ok(**q) == (kw in good), kw
    for c, ok in [(colour_params(), True), (colour_params((2, 1, 0.5), 1.0), True), (colour_params((1, 1, 1), 1.01), False), (colour_params((1, 1, 1), -0.1), False),
                  (colour_params((1, 1, 1), nan), False), (colour_params((0, 1, 1)), False), (colour_params((1, -1, 1)), False), (colour_params((1, 1, nan)), False),
                  (colour_params((inf, 1, 1)), False), (colour_params(flags=1), False)]:
        assert bool(host.L.colour_params_ok(C.byref(c))) == ok
    for n in range(0, 70):
        assert bool(host.L.colour_lut_size_ok(n)) == (n in colour_ref.LUT_SIZES) == (n in state.COLOUR_LUT_SIZES), n


def test_struct_layouts_and_defaults(host):
    lay = np.zeros(20, np.uint32)
    host.L.colour_layout(lay.ctypes.data)
    W, Rs, Cd, Cp = state.WhiteParams, state.WhiteResult, state.CdlParams, state.ColourParams
    assert list(lay) == [C.sizeof(W), C.sizeof(Rs), C.sizeof(Cd), C.sizeof(Cp), W.strength.offset, W.previous.offset, W.flags.offset, Rs.target.offset,
                         Rs.illuminant.offset, Rs.eu.offset, Rs.gated.offset, Rs.estimated.offset, Cd.offset.offset, Cd.power.offset, Cd.saturation.offset,
                         Cd.flags.offset, Cp.lut_strength.offset, Cp.flags.offset, Cp._pad.offset, state.WHITE_WORDS]
    assert (C.sizeof(W), C.sizeof(Rs), C.sizeof(Cd), C.sizeof(Cp)) == (40, 64, 48, 32) and state.WHITE_WORDS == colour_ref.WORDS == 4097
    w, c, size, strength = W(), Cd(), C.c_uint32(), C.c_float()
    host.L.colour_defaults(C.byref(w), C.byref(c), C.byref(size), C.byref(strength))
    got = {"gate": w.gate, "iterations": w.iterations, "min_permille": w.min_permille, "strength": w.strength, "max_stops": w.max_stops, "blend": w.blend,
           "previous": tuple(w.previous)}
    assert got == colour_ref.WHITE_DEFAULTS == state.WHITE_DEFAULTS == {"gate": 12, "iterations": 3, "min_permille": 50, "strength": 1.0, "max_stops": 2.0,
                                                                        "blend": 1.0, "previous": (0.0, 0.0, 0.0)} and w.flags == 0
    assert (list(c.slope), list(c.offset), list(c.power), c.saturation, c.flags) == ([1, 1, 1], [0, 0, 0], [1, 1, 1], 1, 0)
    assert colour_ref.CDL_DEFAULTS == state.CDL_DEFAULTS == {"slope": 1.0, "offset": 0.0, "power": 1.0, "saturation": 1.0} and (size.value, strength.value) == (33, 1.0)
    import inspect
    sig = inspect.signature(R.State.display_colour_srgb8).parameters
    names = ("source", "exposure", "white", "lut_strength", "shadows", "highlights", "bloom_intensity")
    assert list(sig)[1:8] == list(names) and [sig[k].default for k in names] == ["mean", None, None, None, None, None, 0.0]
    assert inspect.signature(R.State.colour_lut).parameters["size"].default == 33
    assert [inspect.signature(R.State.auto_white_balance).parameters[k].default for k in ("source", "blend")] == ["mean", 1.0]


SYMBOLS = ("rsrt_white_meter", "rsrt_white_download", "rsrt_white_reset", "rsrt_colour_lut_build", "rsrt_colour_lut_upload", "rsrt_colour_lut_download",
           "rsrt_colour_lut_reset", "rsrt_display_colour_srgb8")


def test_libraries_export_white_balance_and_colour_grading():
    lib = C.CDLL(_build.build_hip())
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    for m in ("white_meter", "white_download", "auto_white_balance", "white_reset", "colour_lut", "colour_lut_upload", "colour_lut_download", "colour_lut_reset",
              "display_colour_srgb8"):
        assert hasattr(R.State, m), m
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    for n in SYMBOLS:
        assert "Rust: pub fn %s(" % n in hdr, n  # every entry point carries its Rust signature


KERNELS = ("rt_white_hist_kernel", "rt_colour_lut_kernel", "rt_display_colour_kernel")


def test_colour_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "colour_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "colour_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_colour_compiles(tmp_path):
    build_cpp_demo(tmp_path)


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """colour_host.cpp as a program of its own with -fsanitize=address,undefined: the special pixels through the meter and the display,
    the 2^3 and 3^3 LUTs at their corners, edges and past a NaN (LUT buffers of exactly n^3 nodes).  On the CPU, outside Python."""
    exe = str(tmp_path / "colour_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
           "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "colour_host: ok" in r.stdout, r.stdout
