"""The finished display without a GPU: the published arithmetic (include/rsrt_finish.h), compiled for the CPU, against the numpy
restatement the GPU tests hold the kernels to (tests/finish_ref.py), bit for bit and byte for byte, special values included; the
identities (all three parameters 0: the colour display's bytes; a constant frame; a flat cross); the values RCAS's formulas give on a
step; what the dither and the grain promise, statistically, with bounds worked out in the tests' comments; the parameter checks, the ABI,
the kernels' code objects, the C++ State, a sanitizer run of the host program, and the sharpener's direction on a rendered frame."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import bloom_ref
import colour_ref
import finish_ref
import local_ref
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (1, 2), (3, 1), (9, 33), (5, 67)]  # (h, w): 1 x 1, 2 x 1, 1 x 3, 33 x 9 and 67 x 5 as width x height
F = np.float32
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "finish_host.cpp")
SETTINGS = [dict(sharpness=s, grain=g, dither=d, seed=seed, flags=fl)
            for s in (0.0, 0.5, 1.0) for g in (0.0, 1.0) for d in (0.0, 1.0) for fl in (0, finish_ref.NOISE_AWARE) for seed in (0, 0x9e3779b9)]


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def finish_params(sharpness=0.5, grain=0.0, dither=1.0, seed=0, flags=0):
    return state.FinishParams(sharpness, grain, dither, seed, flags, (C.c_uint32 * 3)())


def colour_params(white=(1.0, 1.0, 1.0), strength=0.0, flags=0):
    return state.ColourParams((C.c_float * 3)(*white), strength, flags, (C.c_uint32 * 3)())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("finish") / "libfinish.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.finish_records.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.finish_shape.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.finish_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.finish_sdr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.finish_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                 C.c_void_p]
    L.finish_hash.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.finish_quantise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.finish_params_ok.argtypes = [C.c_void_p]
    L.finish_defaults.argtypes = [C.c_void_p]
    L.finish_layout.argtypes = [C.c_void_p]

    def lut4(lut):
        return np.ascontiguousarray(np.concatenate([np.asarray(lut, F), np.ones(lut.shape[:3] + (1,), F)], axis=-1))

    class Host:
        @staticmethod
        def records(sdr):
            sdr = np.ascontiguousarray(sdr, F)
            out = np.empty(sdr.shape[:-1] + (4,), F)
            L.finish_records(sdr.ctypes.data, sdr.size // 3, out.ctypes.data)
            return out

        @staticmethod
        def shape(sdr, **kw):
            sdr = np.ascontiguousarray(sdr, F)
            out = np.empty_like(sdr)
            p = finish_params(**kw)
            L.finish_shape(sdr.ctypes.data, sdr.shape[0], sdr.shape[1], C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def frame(sdr, **kw):
            sdr = np.ascontiguousarray(sdr, F)
            out = np.zeros(sdr.shape[:2] + (4,), np.uint8)
            p = finish_params(**kw)
            L.finish_frame(sdr.ctypes.data, sdr.shape[0], sdr.shape[1], C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def _chain(fn, sums, total, exposure, white, lut, strength, gain, intensity, b, tail):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            gain = None if gain is None else np.ascontiguousarray(gain, F)
            b = None if b is None else np.ascontiguousarray(b, F)
            l4 = None if lut is None else lut4(lut)
            c = colour_params(white, strength)
            fn(sums.ctypes.data, h, w, total, exposure, None if gain is None else gain.ctypes.data, intensity, None if b is None else b.ctypes.data, C.byref(c),
               None if l4 is None else l4.ctypes.data, 0 if lut is None else lut.shape[0], *tail)

        @staticmethod
        def sdr(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None):
            out = np.empty(sums.shape[:2] + (3,), F)
            Host._chain(L.finish_sdr, sums, total, exposure, white, lut, strength, gain, intensity, b, (out.ctypes.data,))
            return out

        @staticmethod
        def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, **kw):
            out = np.zeros(sums.shape[:2] + (4,), np.uint8)
            p = finish_params(**kw)
            Host._chain(L.finish_display, sums, total, exposure, white, lut, strength, gain, intensity, b, (C.byref(p), out.ctypes.data))
            return out

        @staticmethod
        def hash(x, y, seed, k):
            x, y = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
            words, uni = np.empty(x.shape, np.uint32), np.empty(x.shape, F)
            L.finish_hash(x.ctypes.data, y.ctypes.data, x.size, seed, k, words.ctypes.data, uni.ctypes.data)
            return words, uni

        @staticmethod
        def quantise(x, dither, u1, u2):
            x, u1, u2 = (np.ascontiguousarray(v, F) for v in (x, u1, u2))
            out = np.empty(x.shape, np.uint8)
            L.finish_quantise(x.ctypes.data, u1.ctypes.data, u2.ctypes.data, x.size, dither, out.ctypes.data)
            return out
    Host.L = L
    return Host


# -- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_every_step_matches_numpy_bit_for_bit(host, h, w):
    sdr = finish_ref.special_sdr(h, w, seed=100 * h + w)
    if h * w >= 64:
        flat = sdr.reshape(-1)
        assert np.isnan(flat).any() and np.isinf(flat).any() and (flat < 0).any() and (flat == 1).any() and ((flat > 0) & (flat < 1e-38)).any()
    assert same(host.records(sdr), finish_ref.record(sdr))
    for kw in SETTINGS:
        _, want = finish_ref.shape(sdr, **kw)
        got = host.shape(sdr, **kw)
        assert same(got, want), kw
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
        assert np.array_equal(host.frame(sdr, **kw), finish_ref.frame(sdr, **kw)), kw


def test_every_threshold_and_its_neighbours_through_the_quantiser(host):
    t = finish_ref.thresholds()
    x = np.concatenate([t, np.nextafter(t, F(0)), np.nextafter(t, F(2)), F([0, 1, np.nan, np.inf, -np.inf, -1, 1e-41, 2])]).astype(F)
    rng = np.random.default_rng(5)
    for dither in (0.0, 0.5, 1.0):
        for _ in range(4):
            u1, u2 = (rng.integers(0, 1 << 24, x.size).astype(F) * F(2.0 ** -24) for _ in range(2))
            got = host.quantise(x, dither, u1, u2)
            assert np.array_equal(got, finish_ref.quantise(x, dither, u1, u2)), dither
            hard = colour_ref.encode(x.reshape(1, -1, 1))[0, :, 0]
            assert np.abs(got.astype(int) - hard.astype(int)).max() <= (1 if dither else 0)
            assert np.array_equal(got[(hard == 0) | (hard == 255)], hard[(hard == 0) | (hard == 255)])  # bytes 0 and 255 never move


def test_hash_matches_numpy_and_is_uniform(host):
    y, x = np.meshgrid(np.arange(64), np.arange(128), indexing="ij")
    x, y = np.concatenate([x.ravel(), [0xffffffff, 0, 70000]]), np.concatenate([y.ravel(), [0, 0xffffffff, 70000]])
    for seed in (0, 1, 0xffffffff):
        for k in (0, 1, 6):
            words, uni = host.hash(x, y, seed, k)
            assert np.array_equal(words.astype(np.uint64), finish_ref.hash_(x, y, seed, k)) and same(uni, finish_ref.uniform(words))
            assert uni.min() >= 0 and uni.max() < 1
            # 8195 uniforms: mean 1 / 2 with standard error 0.0032, a sixteen-cell histogram with 512 a cell, standard deviation 22
            assert abs(float(uni.mean()) - 0.5) <= 6 * 0.0032
            assert np.abs(np.bincount((uni * 16).astype(int), minlength=16) - 512).max() <= 6 * 22
    a, b = host.hash(x, y, 7, 1)[0], host.hash(x, y, 7, 2)[0]
    assert (a != b).mean() > 0.999 and (host.hash(x, y, 8, 1)[0] != a).mean() > 0.999  # draws and seeds are different streams


@pytest.mark.parametrize("h,w", FRAMES)
def test_whole_pass_matches_numpy_byte_for_byte(host, h, w):
    sums, _ = local_ref.synthetic(h, w, seed=2000 * h + w)
    total, exposure, white = 3, 0.37, (1.3, 0.95, 0.6)
    b = bloom_ref.bloom(sums, total, exposure, 3)
    gain = local_ref.gains(sums, total, exposure, local_ref.grid_of(sums, total, 8), 8)
    lut = colour_ref.bake(17, *colour_ref.CDLS["warm"])
    for strength, g, intensity in ((0.0, None, 0.0), (1.0, gain, 0.5), (0.5, None, 0.5)):
        args = (sums, total, exposure, white, lut, strength, g, intensity, b)
        assert util.same_bits_or_nan(host.sdr(*args), finish_ref.sdr_of(*args))
        for kw in SETTINGS[::5] + [SETTINGS[-1]]:
            assert np.array_equal(host.display(*args, **kw), finish_ref.display(*args, **kw)), (strength, intensity, kw)
        # with all three 0: rsrt_display_pixel_colour's bytes, white != 1 and a LUT included
        zero = dict(sharpness=0.0, grain=0.0, dither=0.0)
        assert np.array_equal(host.display(*args, **zero), colour_ref.display(*args))
        assert np.array_equal(host.display(*args, seed=99, flags=finish_ref.NOISE_AWARE, **zero), colour_ref.display(*args))


# -- identities ----------------------------------------------------------------------------------------------------------------------
def test_a_constant_frame_stays_byte_identical_at_any_sharpness(host):
    for value in ((0.3, 0.6, 0.1), (0.0, 1.0, 0.5), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (np.nan, 0.2, 0.7)):
        sdr = np.broadcast_to(F(value), (7, 37, 3)).copy()
        hard = colour_ref.encode(sdr)
        for sharpness in (0.0, 0.25, 1.0):
            for flags in (0, finish_ref.NOISE_AWARE):
                assert np.array_equal(host.frame(sdr, sharpness=sharpness, dither=0.0, flags=flags), hard), (value, sharpness)
                assert same(host.shape(sdr, sharpness=sharpness, dither=0.0, flags=flags), finish_ref.record(sdr)[..., :3])


def test_a_pixel_with_a_flat_cross_is_untouched_whatever_lies_elsewhere(host):
    rng = np.random.default_rng(8)
    sdr = rng.random((20, 45, 3)).astype(F)
    flat = [(0, 0), (19, 44), (7, 9), (12, 30), (0, 20)]
    for y, x in flat:  # the pixel and its clamped cross take one value; the diagonals keep theirs
        for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            sdr[min(max(yy, 0), 19), min(max(xx, 0), 44)] = sdr[y, x]
    hard = colour_ref.encode(sdr)
    for flags in (0, finish_ref.NOISE_AWARE):
        got = host.frame(sdr, sharpness=1.0, grain=0.0, dither=0.0, flags=flags)
        for y, x in flat:
            assert np.array_equal(got[y, x], hard[y, x]), (y, x)
        assert (got != hard).any(axis=-1).mean() > 0.5  # (the sharpener is at work everywhere else)


# -- derived values -------------------------------------------------------------------------------------------------------------------
def test_a_step_between_a_quarter_and_three_quarters_at_sharpness_one(host):
    """enc 0.25 | 0.75.  At the column left of the step the ring is (0.25, 0.25, 0.75, 0.25): mn4 = 0.25, mx4 = 0.75, hitMin = 1 / 12,
    hitMax = 0.25 / -3 = -1 / 12, lobe = max(-1 / 12, -1 / 12) = -1 / 12 (inside the -0.1875 limit), and o = 0.25 + (-1 / 12)(0.5) /
    (1 - 1 / 3) = 0.25 - 0.0625 = 0.1875; by symmetry 0.8125 on the right.  Six f32 roundings: within 2 ulp of 0.1875."""
    enc = np.full((6, 12, 3), 0.25, F)
    enc[:, 6:] = 0.75
    sdr = (enc * enc).astype(F)  # (exact: sqrt gives enc back)
    assert same(host.records(sdr)[..., :3], enc)
    o = host.shape(sdr, sharpness=1.0, dither=0.0)
    assert same(o, finish_ref.shape(sdr, sharpness=1.0, dither=0.0)[1])
    assert np.abs(o[:, 5] - F(0.1875)).max() <= 2 * np.spacing(F(0.1875)) and np.abs(o[:, 6] - F(0.8125)).max() <= 2 * np.spacing(F(0.8125))
    keep = np.ones(12, bool)
    keep[5:7] = False
    assert same(o[:, keep], enc[:, keep])  # every other column unchanged
    assert o.min() >= 0 and o.max() <= 1
    # the limiter: at the step |mean of the ring - e| / range = 0.125 / 0.5 in luma, so the lobe shrinks by 1 - 0.5 * 0.25
    o = host.shape(sdr, sharpness=1.0, dither=0.0, flags=finish_ref.NOISE_AWARE)
    lobe = -(1 / 12) * 0.875
    assert np.abs(o[:, 5] - (0.25 + lobe * 0.5 / (4 * lobe + 1))).max() <= 4 * np.spacing(F(0.25))


def test_rings_of_all_zero_and_all_one_give_finite_results(host):
    for ring in (0.0, 1.0):
        for centre in (0.0, 1e-30, 0.25, 0.5, 1.0):
            sdr = np.full((3, 3, 3), ring, F)
            sdr[1, 1] = centre
            for flags in (0, finish_ref.NOISE_AWARE):
                o = host.shape(sdr, sharpness=1.0, dither=0.0, flags=flags)
                assert np.isfinite(o).all() and o.min() >= 0 and o.max() <= 1
                assert same(o[1, 1], finish_ref.record(sdr)[1, 1, :3])  # the channel's lobe is 0 there: the centre stays
                assert same(o, finish_ref.shape(sdr, sharpness=1.0, dither=0.0, flags=flags)[1])


# -- dither ---------------------------------------------------------------------------------------------------------------------------
def value_at(code, p):
    """The linear value at position p of code's bin."""
    t = finish_ref.thresholds().astype(np.float64)
    return F(t[code - 1] + p * (t[code] - t[code - 1]))


def test_dither_mean_is_the_continuous_code(host):
    """A 256 x 256 frame held at p = 0.25 of bin 128: the byte is 129 with probability p^2 / 2, 127 with (1 - p)^2 / 2, so its mean is
    128 + p - 0.5 = 127.75 and its variance 0.25 (< 0.75); 65536 draws: within 0.02, six standard errors of variance 0.75."""
    sdr = np.full((256, 256, 3), value_at(128, 0.25), F)
    kw = dict(sharpness=0.0, grain=0.0, dither=1.0, seed=3)
    ref = finish_ref.frame(sdr, **kw)[..., :3]
    for c in range(3):  # the restatement alone meets it ...
        assert abs(ref[..., c].astype(np.float64).mean() - 127.75) <= 0.02, c
    got = host.frame(sdr, **kw)[..., :3]
    assert np.array_equal(got, ref)
    for c in range(3):  # ... and so does the header
        assert abs(got[..., c].astype(np.float64).mean() - 127.75) <= 0.02, c
        assert set(np.unique(got[..., c])) == {127, 128, 129}
    assert not np.array_equal(got[..., 0], got[..., 1])  # the channels take draws of their own
    # the same seed gives the same bytes, another changes at least a third of the pixels (two independent draws differ with probability
    # 1 - (0.6875^2 + 0.28125^2 + 0.03125^2) = 0.447)
    assert np.array_equal(host.frame(sdr, **kw), host.frame(sdr, **kw))
    other = host.frame(sdr, **dict(kw, seed=4))[..., :3]
    assert (other != got).mean() >= 1 / 3
    assert np.array_equal(host.frame(sdr, **dict(kw, dither=0.0))[..., :3], np.full((256, 256, 3), 128, np.uint8))


def test_dither_breaks_up_the_bands_of_a_ramp(host):
    """A 1024-wide, 64-high ramp over the four codes 100 .. 103, linear in the continuous code (code - 0.5 + p).  The 16 x 16 box means of
    the dithered bytes stay within 0.25 code of the boxes' mean continuous code (a box mean has standard error 0.5 / 16 = 0.031); the
    undithered ones are off by up to half a code."""
    t = finish_ref.thresholds().astype(np.float64)
    code = np.linspace(99.5, 103.5, 1024, endpoint=False)  # continuous: code k's bin is [k - 0.5, k + 0.5)
    k = np.floor(code + 0.5).astype(int)
    x = (t[k - 1] + (code - (k - 0.5)) * (t[k] - t[k - 1])).astype(F)
    sdr = np.broadcast_to(x[None, :, None], (64, 1024, 3)).copy()
    hard_codes = colour_ref.encode(sdr)[..., 0].astype(np.float64)
    assert np.array_equal(np.unique(hard_codes), [100, 101, 102, 103])
    box = lambda a: a.reshape(4, 16, 64, 16).mean(axis=(1, 3))  # noqa: E731
    want = box(np.broadcast_to(code, (64, 1024)))
    ref = finish_ref.frame(sdr, sharpness=0.0, dither=1.0, seed=1)
    got = host.frame(sdr, sharpness=0.0, dither=1.0, seed=1)
    assert np.array_equal(got, ref)
    for bytes_ in (ref, got):
        for c in range(3):
            assert np.abs(box(bytes_[..., c].astype(np.float64)) - want).max() <= 0.25, c
    hard = host.frame(sdr, sharpness=0.0, dither=0.0)
    assert np.array_equal(hard[..., 0], hard_codes)
    worst = np.abs(box(hard_codes) - want).max()
    # the bands: a pixel is up to half a code off.  At 256 columns a code, the 16 columns of the box beside a threshold are 0.5 - j / 256 off,
    # j = 0 .. 15: a mean of 0.5 - 7.5 / 256 = 0.4707, the most a box mean of this ramp can reach
    assert abs(worst - (0.5 - 7.5 / 256)) < 1e-3
    # bytes 0 and 255 never move
    ends = np.zeros((16, 16, 3), F)
    ends[:, 8:] = 1.0
    ends[0, 0] = np.nan
    assert np.array_equal(host.frame(ends, sharpness=0.0, dither=1.0, seed=5), colour_ref.encode(ends))


# -- grain ----------------------------------------------------------------------------------------------------------------------------
def test_grain_is_shaped_monochrome_and_bounded(host):
    rng = np.random.default_rng(11)
    grey = rng.random((40, 50, 1)).astype(F)
    enc = np.broadcast_to(grey, (40, 50, 3)).copy()
    enc[0, :25], enc[1, :25] = 0.0, 1.0
    sdr = (enc.astype(np.float64) ** 2).astype(F)
    e = host.records(sdr)[..., :3]
    for grain in (0.25, 1.0):
        o = host.shape(sdr, sharpness=0.0, grain=grain, dither=0.0, seed=2)
        assert same(o, finish_ref.shape(sdr, sharpness=0.0, grain=grain, dither=0.0, seed=2)[1])
        assert same(o[:2, :25], e[:2, :25])  # zero at enc 0 and 1
        bound = F(grain) * np.minimum(e, F(1) - e)
        assert (np.abs(o.astype(np.float64) - e) <= bound.astype(np.float64) + np.spacing(F(1))).all() and o.min() >= 0 and o.max() <= 1
        assert same(o[..., 0], o[..., 1]) and same(o[..., 1], o[..., 2])  # a grey pixel stays grey: one draw a pixel
        moved = (o != e).any(axis=-1)
        assert moved[2:].mean() > 0.99 and not same(o, host.shape(sdr, sharpness=0.0, grain=grain, dither=0.0, seed=3))
    # on any colour the three channels share the draw: (o - e) / min(e, 1 - e) is one number a pixel
    colour = rng.random((30, 30, 3)).astype(F) * F(0.8) + F(0.1)
    sdr = (colour * colour).astype(F)
    e = host.records(sdr)[..., :3].astype(np.float64)
    o = host.shape(sdr, sharpness=0.0, grain=1.0, dither=0.0, seed=9).astype(np.float64)
    t = (o - e) / np.minimum(e, 1 - e)
    assert np.abs(t - t[..., :1]).max() <= 1e-5 and np.abs(t).max() <= 1 + 1e-6 and t.min() < -0.9 and t.max() > 0.9


# -- parameters, layouts, ABI --------------------------------------------------------------------------------------------------------
def test_params_ok_accepts_and_refuses(host):
    nan, inf = float("nan"), float("inf")
    good = [{}, {"sharpness": 0.0}, {"sharpness": 1.0}, {"grain": 1.0}, {"dither": 0.0}, {"seed": 0xffffffff}, {"flags": finish_ref.NOISE_AWARE}]
    bad = [{k: v} for k in ("sharpness", "grain", "dither") for v in (-0.001, 1.001, nan, inf, -inf)] + [{"flags": 2}, {"flags": 3}, {"flags": 0x80000000}]
    for kw in good + bad:
        p = finish_params(**kw)
        assert bool(host.L.finish_params_ok(C.byref(p))) == finish_ref.params_ok(**dict(finish_ref.DEFAULTS, **kw)) == (kw in good), kw


def test_struct_layout_and_defaults(host):
    lay = np.zeros(7, np.uint32)
    host.L.finish_layout(lay.ctypes.data)
    P = state.FinishParams
    assert list(lay) == [C.sizeof(P), P.grain.offset, P.dither.offset, P.seed.offset, P.flags.offset, P._pad.offset, state.FINISH_NOISE_AWARE]
    assert list(lay) == [32, 4, 8, 12, 16, 20, 1] and finish_ref.NOISE_AWARE == 1
    p = P()
    host.L.finish_defaults(C.byref(p))
    got = {"sharpness": p.sharpness, "grain": p.grain, "dither": p.dither, "seed": p.seed, "flags": p.flags}
    assert got == finish_ref.DEFAULTS == state.FINISH_DEFAULTS == {"sharpness": 0.5, "grain": 0.0, "dither": 1.0, "seed": 0, "flags": 0}
    sig = inspect.signature(R.State.display_finished_srgb8).parameters
    names = ("source", "exposure", "white", "lut_strength", "shadows", "highlights", "bloom_intensity", "sharpness", "grain", "dither", "seed", "noise_aware",
             "sample_total")
    assert list(sig)[1:14] == list(names)
    assert [sig[k].default for k in names] == ["mean", None, None, None, None, None, 0.0, None, None, None, None, False, None]
    assert list(sig)[1:8] == list(inspect.signature(R.State.display_colour_srgb8).parameters)[1:8]


def test_libraries_export_the_finished_display():
    lib = C.CDLL(_build.build_hip())
    assert hasattr(lib, "rsrt_display_finished_srgb8")
    assert hasattr(R.State, "display_finished_srgb8") and not hasattr(state.MultiState, "display_finished_srgb8")
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "Rust: pub fn rsrt_display_finished_srgb8(" in hdr
    assert "rsrt_display_finished_srgb8" in open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    cpp = open(os.path.join(util.ROOT, "include", "rsrt_state.hpp")).read()
    assert "display_finished(" in cpp and "finish_defaults()" in cpp


def test_finish_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = sorted(n for n in md if "rt_display_finish_kernel" in n)
    assert len(names) == 2 and "ILb0E" in names[0] and "ILb1E" in names[1], names  # <false> and <true>
    for n in names:
        k = md[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "finish_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "finish_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_finish_compiles(tmp_path):
    build_cpp_demo(tmp_path)


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """finish_host.cpp as a program of its own (-DFINISH_HOST_MAIN) with -fsanitize=address,undefined: frames of special sums and special
    sdr values of 1 x 1 to 31 x 7 through every step at every corner of the parameters, the degenerate rings, and every threshold with its
    neighbours through the quantiser.  On the CPU, outside Python."""
    exe = str(tmp_path / "finish_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DFINISH_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "finish_host: ok" in r.stdout, r.stdout


# -- a picture ------------------------------------------------------------------------------------------------------------------------
def laplacian(img):
    g = img[..., :3].astype(np.float64)
    return np.abs(4 * g[1:-1, 1:-1] - g[:-2, 1:-1] - g[2:, 1:-1] - g[1:-1, :-2] - g[1:-1, 2:]).mean()


def test_sharpening_raises_the_laplacian_of_an_over_filtered_render(host):
    """House at 96 x 54 and 4 spp from the CPU path tracer, box-blurred 3 x 3 (a stand-in for an over-filtered picture): the mean absolute
    Laplacian of the finished bytes at sharpness 1 exceeds that at sharpness 0.  The direction only; DESIGN.md §24 quotes the numbers."""
    sc = R.Scene.load_toml(util.scene_path("house"))
    acc, _ = oracle.render(util.oracle_scene(sc), util.oracle_env(util.small_env()), sc.camera_uniform().view(oracle.CAMERA), 96, 54, 0, 4, 8, fast=True)
    p = np.pad(acc.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    blurred = (sum(p[dy:dy + 54, dx:dx + 96] for dy in range(3) for dx in range(3)) / 9).astype(F)
    soft = host.display(blurred, 4, 1.0, sharpness=0.0, dither=0.0)
    sharp = host.display(blurred, 4, 1.0, sharpness=1.0, dither=0.0)
    assert np.array_equal(sharp, finish_ref.display(blurred, 4, 1.0, sharpness=1.0, dither=0.0))
    a, b = laplacian(soft), laplacian(sharp)
    print("house 96 x 54, 4 spp, 3 x 3 box: mean |Laplacian| of the bytes %.3f at sharpness 0, %.3f at sharpness 1" % (a, b))
    assert b > a
