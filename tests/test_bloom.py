"""Bloom without a GPU: its published arithmetic (include/rsrt_bloom.h), compiled for the CPU, against the numpy restatement the GPU
tests hold the kernels to (tests/bloom_ref.py), bit for bit, special pixels included; B finite and >= 0; the constant-image identity;
intensity 0 against the exposed display; threshold 0; symmetry; the parameter check; the ABI and the kernels' code objects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (1, 7), (2, 2), (3, 5), (23, 37), (17, 65)]  # (h, w)
LEVELS = [1, 2, 6, 8]
F = np.float32


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bloom") / "libbloom.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "bloom_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.bloom_prefilter.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.bloom_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    L.bloom_up_tent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.bloom_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
    L.bloom_params_ok.argtypes = [C.c_void_p]
    L.bloom_defaults.argtypes = [C.c_void_p, C.c_void_p]
    L.bloom_level_size.argtypes = [C.c_uint32, C.c_uint32]
    L.bloom_level_size.restype = C.c_uint32
    L.bloom_layout.argtypes = [C.c_void_p]

    class Host:
        @staticmethod
        def prefilter(sums, total, exposure, threshold):
            sums = np.ascontiguousarray(sums, F)
            out = np.full(sums.shape[:-1] + (4,), 7, F)
            L.bloom_prefilter(sums.ctypes.data, sums.size // 4, total, exposure, threshold, out.ctypes.data)
            return out

        @staticmethod
        def bloom(sums, total, exposure, levels=6, threshold=1.0, karis=True):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            out = np.full(((h + 1) // 2, (w + 1) // 2, 4), 7, F)
            L.bloom_image(sums.ctypes.data, h, w, total, exposure, levels, 1 if karis else 0, threshold, out.ctypes.data)
            return out

        @staticmethod
        def up_tent(u, H, W):
            u = np.ascontiguousarray(u, F)
            out = np.full((H, W, 4), 7, F)
            L.bloom_up_tent(u.ctypes.data, u.shape[0], u.shape[1], H, W, out.ctypes.data)
            return out

        @staticmethod
        def display(sums, total, exposure, intensity=None, b=None):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            out = np.zeros((h, w, 4), np.uint8)
            if b is None:
                L.bloom_display(sums.ctypes.data, h, w, total, exposure, 0.0, None, 0, out.ctypes.data)
            else:
                b = np.ascontiguousarray(b, F)
                L.bloom_display(sums.ctypes.data, h, w, total, exposure, intensity, b.ctypes.data, 1, out.ctypes.data)
            return out

        @staticmethod
        def ok(levels=6, flags=1, threshold=1.0):
            p = state.BloomParams(levels, flags, threshold, 0.0)
            return bool(L.bloom_params_ok(C.byref(p)))
    Host.L = L
    return Host


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("karis", [True, False])
def test_header_arithmetic_matches_numpy_bit_for_bit(host, h, w, karis):
    sums, special = bloom_ref.synthetic(h, w, seed=1000 * h + w)
    assert bool(special) == (h * w >= 16)
    for levels in LEVELS:
        for threshold in (0.0, 1.0):
            for total in (1, 3):
                for exposure in (1.0, 0.37):
                    case = (levels, threshold, total, exposure)
                    got = host.bloom(sums, total, exposure, levels, threshold, karis)
                    want = bloom_ref.bloom(sums, total, exposure, levels, threshold, karis)
                    assert got.shape == want.shape == ((h + 1) // 2, (w + 1) // 2, 4) and same(got, want), case
                    # finite and >= 0 on the special frames, alpha 1
                    assert np.isfinite(got).all() and (got >= 0).all() and (got[..., 3] == 1).all(), case
                    for intensity in (0.1, 2.0):
                        assert np.array_equal(host.display(sums, total, exposure, intensity, got),
                                              bloom_ref.display(sums, total, exposure, intensity, want)), (case, intensity)


@pytest.mark.parametrize("h,w", FRAMES)
def test_fused_up_tent_is_the_two_steps(host, h, w):
    """up(tent(u)) evaluated without the tent in memory — the form the up kernel takes — against numpy's two separate steps."""
    u = bloom_ref.prefilter(bloom_ref.synthetic(h, w, seed=h + w)[0], 1, 1.0, 0.0)
    u4 = np.concatenate([u, np.zeros(u.shape[:2] + (1,), F)], axis=-1)
    for H, W in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1), (2 * h, 2 * w - 1)):
        if H < 1 or W < 1:
            continue
        got = host.up_tent(u4, H, W)
        assert same(got[..., :3], bloom_ref.up(bloom_ref.tent(u), H, W)) and (got[..., 3] == 0).all(), (H, W)


def test_special_pixels_go_through_the_prefilter_as_documented(host):
    h, w = 23, 37
    sums, special = bloom_ref.synthetic(h, w, seed=5)
    for total in (1, 3):
        for threshold in (0.0, 1.0):
            got = host.prefilter(sums, total, 1.0, threshold)
            assert same(got[..., :3], bloom_ref.prefilter(sums, total, 1.0, threshold)) and (got[..., 3] == 0).all()
            flat = got.reshape(-1, 4)
            assert np.isfinite(flat).all() and (flat >= 0).all()
            assert flat[special["nan"], 1] == 0  # the NaN channel alone is zeroed
            if threshold == 0:
                assert flat[special["nan"], 0] > 0 and flat[special["nan"], 2] > 0
            assert (flat[special["neg_inf"], 0], flat[special["negative"], 0], flat[special["negative"], 2]) == (0, 0, 0)
            assert (flat[special["neg_zero"], :3] == 0).all() and (flat[special["denormal"], :3] <= F(1e-41)).all()
            if threshold == 0:
                assert flat[special["inf"], 2] == 65504 and (flat[special["huge"], :3] == 65504).all()
                assert flat[special["f16_overflow"], 2] == 65504  # (65530 as a mean of 3 too: above the clamp)
    # threshold 0 keeps q == p, bit for bit, wherever the luminance is positive
    p = bloom_ref.exposed(sums, 3, 0.37)
    q = host.prefilter(sums, 3, 0.37, 0.0)[..., :3]
    pos = bloom_ref.lum(p) > 0
    assert pos.sum() > h * w - 8 and same(q[pos], p[pos]) and (q[~pos] == 0).all()


@pytest.mark.parametrize("levels", [1, 2, 4, 8])
def test_a_constant_image_blooms_to_itself(host, levels):
    """Threshold 0, plain form, a constant c of at most 12 significant bits: the weights are powers of two or 0.75 and every partial
    sum needs at most 12 + 3 + 2 bits, so every level is exact: D_k = c, U_k = (N - k + 1) c, B = (N c) * (1 / N), which is c for N a
    power of two."""
    rng = np.random.default_rng(levels)
    for h, w in FRAMES + [(16, 24)]:
        c = (rng.integers(1, 1 << 12, 3).astype(F) * F(2.0) ** rng.integers(-10, 3, 3).astype(F)).astype(F)
        sums = np.ones((h, w, 4), F)
        sums[..., :3] = c
        got = host.bloom(sums, 1, 1.0, levels, 0.0, karis=False)
        assert same(got, bloom_ref.bloom(sums, 1, 1.0, levels, 0.0, karis=False))
        assert same(got[..., :3], np.broadcast_to(c, got[..., :3].shape)), (h, w, c)


@pytest.mark.parametrize("h,w", FRAMES)
def test_intensity_zero_is_the_exposed_display(host, h, w):
    import exposure_ref
    sums, _ = bloom_ref.synthetic(h, w, seed=1000 * h + w)
    for total in (1, 3):
        for exposure in (1.0, 0.37):
            b = host.bloom(sums, total, exposure)
            plain = host.display(sums, total, exposure)
            assert np.array_equal(plain, exposure_ref.display(sums, total, exposure))
            assert np.array_equal(host.display(sums, total, exposure, 0.0, b), plain)
            assert np.array_equal(bloom_ref.display(sums, total, exposure, 0.0, b), plain)
    if h * w >= 16:
        assert not np.array_equal(host.display(sums, 1, 1.0, 0.5, host.bloom(sums, 1, 1.0)), host.display(sums, 1, 1.0))


@pytest.mark.parametrize("karis", [True, False])
def test_one_bright_texel_blooms_symmetrically(host, karis):
    """On an even-sized frame of sizes divisible by 2^levels the pyramid's geometry is symmetric under both flips; a 2x2 block in the
    exact centre is its own mirror image, so B must be too — bit for bit, since mirrored sums pair the same operands (a + b == b + a)."""
    h, w, levels = 32, 48, 3
    sums = np.zeros((h, w, 4), F)
    sums[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1, :3] = (900.0, 500.0, 100.0)
    b = host.bloom(sums, 1, 1.0, levels, 1.0, karis)
    assert same(b, bloom_ref.bloom(sums, 1, 1.0, levels, 1.0, karis)) and b[..., :3].max() > 0
    assert np.count_nonzero(b[..., 0]) > 100  # it spread
    assert same(b, b[::-1]) and same(b, b[:, ::-1])
    # one texel alone: the flip of the frame gives the flip of B
    one = np.zeros((h, w, 4), F)
    one[11, 30, :3] = (900.0, 500.0, 100.0)
    b1 = host.bloom(one, 1, 1.0, levels, 1.0, karis)
    assert same(host.bloom(one[::-1], 1, 1.0, levels, 1.0, karis), b1[::-1])
    assert same(host.bloom(one[:, ::-1], 1, 1.0, levels, 1.0, karis), b1[:, ::-1])


def test_params_ok_accepts_and_rejects(host):
    good = [{}, {"levels": 1}, {"levels": 8}, {"flags": 0}, {"threshold": 0.0}, {"threshold": 65504.0}]
    bad = [{"levels": 0}, {"levels": 9}, {"levels": 0xffffffff}, {"flags": 2}, {"flags": 3}, {"flags": 0x80000000}]
    bad += [{"threshold": v} for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf"))]
    d = bloom_ref.DEFAULTS
    for kw in good:
        q = dict({"levels": d["levels"], "flags": d["flags"], "threshold": d["threshold"]}, **kw)
        assert host.ok(**kw) and bloom_ref.params_ok(**q), kw
    for kw in bad:
        q = dict({"levels": d["levels"], "flags": d["flags"], "threshold": d["threshold"]}, **kw)
        assert not host.ok(**kw) and not bloom_ref.params_ok(**q), kw
    assert host.ok(threshold=-0.0)


def test_struct_layout_defaults_and_level_sizes(host):
    lay = np.zeros(6, np.uint32)
    host.L.bloom_layout(lay.ctypes.data)
    P = state.BloomParams
    assert list(lay) == [C.sizeof(P), P.flags.offset, P.threshold.offset, P._pad.offset, state.BLOOM_MAX_LEVELS, state.BLOOM_KARIS]
    assert C.sizeof(P) == 16 and [f[0] for f in P._fields_] == ["levels", "flags", "threshold", "_pad"]
    d, intensity = P(), C.c_float()
    host.L.bloom_defaults(C.byref(d), C.byref(intensity))
    got = {"levels": d.levels, "flags": d.flags, "threshold": d.threshold, "intensity": intensity.value}
    want = {k: (v if isinstance(v, int) else float(F(v))) for k, v in bloom_ref.DEFAULTS.items()}
    assert got == want and {k: (v if isinstance(v, int) else float(F(v))) for k, v in state.BLOOM_DEFAULTS.items()} == want
    assert bloom_ref.MAX_LEVELS == state.BLOOM_MAX_LEVELS == 8 and bloom_ref.KARIS == state.BLOOM_KARIS == 1
    for n in (1, 2, 3, 7, 64, 65, 1080, 1920):
        for k in range(9):
            assert host.L.bloom_level_size(n, k) == bloom_ref.level_size(n, k)
    assert [bloom_ref.level_size(1920, k) for k in (1, 4, 8)] == [960, 120, 8] and bloom_ref.level_size(1, 8) == 1
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_BLOOM_KARIS = 1u" in hdr
    import inspect
    sig = inspect.signature(R.State.bloom).parameters
    assert [sig[k].default for k in ("source", "exposure", "levels", "threshold", "karis", "sample_total", "stream")] == ["mean", None, None, None, True, None, None]
    sig = inspect.signature(R.State.display_bloomed_srgb8).parameters
    assert [sig[k].default for k in ("source", "exposure", "intensity", "sample_total")] == ["mean", None, None, None]


def test_library_exports_bloom():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_bloom", "rsrt_bloom_download", "rsrt_bloom_reset", "rsrt_display_bloomed_srgb8"):
        assert hasattr(lib, n), n
    for m in ("bloom", "bloom_download", "bloom_reset", "display_bloomed_srgb8"):
        assert hasattr(R.State, m), m


KERNELS = ("rt_bloom_first_kernel", "rt_bloom_down_kernel", "rt_bloom_up_kernel", "rt_bloom_final_kernel", "rt_display_bloomed_kernel")


def test_bloom_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def tile_constants():
    """RT_BL_TW, RT_BL_TH of the first-level kernel, from the source's #defines."""
    import re
    src = open(os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip", "rt_bloom.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)\b" % n, src).group(1)) for n in ("RT_BL_TW", "RT_BL_TH"))


def test_tile_constants_are_readable():
    tw, th = tile_constants()
    assert tw >= 1 and th >= 1 and tw * th <= 1024


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "bloom_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "bloom_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_bloom_compiles(tmp_path):
    build_cpp_demo(tmp_path)
