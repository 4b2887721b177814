"""Guided upsampling without a GPU: its published per-pixel arithmetic (include/rsrt_upsample.h), compiled for the CPU, against the
numpy restatement the GPU tests hold the kernel to (tests/upsample_ref.py), bit for bit; the fallback for weights that sum to nothing;
the ABI, the parameter defaults and the kernel's code object."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import upsample_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build

# (low h, w) -> (output H, W): odd ratios, one pixel, no magnification in one or both axes, a factor of eight
SHAPES = [((45, 87), (91, 173)), ((1, 1), (1, 1)), ((1, 1), (3, 2)), ((7, 300), (20, 301)), ((33, 65), (33, 65)), ((5, 3), (40, 24))]
SIGMAS = [(0.3, 0.2), (upsample_ref.SIGMA_NORMAL, upsample_ref.SIGMA_DEPTH)]


@pytest.fixture(scope="module")
def host_upsample(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("up") / "libup.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "upsample_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.up_filter.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 7 + [C.c_float] * 2 + [C.c_int, C.c_void_p]
    L.up_filter.restype = C.c_uint32

    def run(colour, aov, guide, S, T, Tg, sn, sz, demod):
        (h, w), (H, W) = colour.shape[:2], guide.shape[:2]
        colour, aov, guide = (np.ascontiguousarray(a, np.float32) for a in (colour, aov, guide))
        out = np.zeros((H, W, 3), np.float32)
        n = L.up_filter(colour.ctypes.data, aov.ctypes.data, guide.ctypes.data, w, h, W, H, S, T, Tg, sn, sz, int(demod), out.ctypes.data)
        return out, n
    return run


def inputs(lo, hi, seed):
    """Low sums + AOV records and guide records of the two sizes, from different seeds (test_denoise.synthetic)."""
    import test_denoise
    sums, aov = test_denoise.synthetic(lo[0], lo[1], 4, 3, seed=seed)
    _, guide = test_denoise.synthetic(hi[0], hi[1], 4, 5, seed=seed + 7919)
    return sums, aov, guide


@pytest.mark.parametrize("lo,hi", SHAPES)
@pytest.mark.parametrize("sn,sz", SIGMAS)
@pytest.mark.parametrize("demod", [True, False])
def test_header_arithmetic_matches_numpy_bit_for_bit(host_upsample, lo, hi, sn, sz, demod):
    sums, aov, guide = inputs(lo, hi, seed=lo[0] * 1000 + lo[1])
    got, n_fallback = host_upsample(sums, aov, guide, 4, 3, 5, sn, sz, demod)
    want, fallback = upsample_ref.upsample(sums, aov, guide, 4, 3, 5, sn, sz, demod, return_fallback=True)
    assert got.shape == (hi[0], hi[1], 3) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert n_fallback == int(fallback.sum()) == 0  # finite features: the nine tent weights are all >= 1 / 16


def test_features_that_pack_to_inf_fall_back_to_the_nearest_low_pixel(host_upsample):
    lo, hi = (45, 87), (91, 173)
    sums, aov, guide = inputs(lo, hi, seed=5)
    aov[10:20, 30:50, 4:7] = 1e9     # low normals -> binary16 inf
    guide[40:70, 20:60, 4:7] = 1e9   # guide normals -> inf; over the low block both: inf - inf = NaN
    got, n_fallback = host_upsample(sums, aov, guide, 4, 3, 5, 0.5, 0.3, True)
    want, fallback = upsample_ref.upsample(sums, aov, guide, 4, 3, 5, 0.5, 0.3, True, return_fallback=True)
    assert np.isfinite(got).all()
    assert n_fallback == int(fallback.sum()) >= 30 * 40  # every pixel of the guide's block at least
    assert fallback[40:70, 20:60].all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a fallback pixel is the nearest low pixel's demodulated colour times the guide's albedo
    r, _ = upsample_ref.low_pass(sums, aov, 4, 3, True)
    Y, X = 50, 33
    yn, xn = upsample_ref.coords(lo[0], hi[0])[1][Y], upsample_ref.coords(lo[1], hi[1])[1][X]
    g = guide[Y, X]
    albedo = (g[:3] + (np.float32(5) - g[3])) / np.float32(5)
    assert np.array_equal(got[Y, X], r[yn, xn] * albedo)


@pytest.mark.parametrize("lo,hi", [((12, 17), (24, 34)), ((5, 3), (40, 24)), ((9, 9), (9, 9))])
def test_a_constant_colour_under_one_albedo_stays_constant(host_upsample, lo, hi):
    rng = np.random.default_rng(3)
    colour = np.float32([0.7, 0.4, 0.2])

    def records(h, w, total):  # one albedo; normals and depths vary, so the weights do
        a = np.zeros((h, w, 8), np.float32)
        a[..., :3], a[..., 3] = 0.5 * total, total
        a[..., 4:7] = rng.normal(0, 1, (h, w, 3)) * total
        a[..., 7] = rng.uniform(1, 5, (h, w)) * total
        return a
    sums = np.ones((lo[0], lo[1], 4), np.float32)
    sums[..., :3] = colour * 4
    aov, guide = records(lo[0], lo[1], 3), records(hi[0], hi[1], 5)
    for demod in (True, False):
        got, _ = host_upsample(sums, aov, guide, 4, 3, 5, 0.5, 0.3, demod)
        assert np.abs(got - colour).max() <= 1e-6, demod
        assert np.abs(upsample_ref.upsample(sums, aov, guide, 4, 3, 5, demodulate=demod) - colour).max() <= 1e-6


def test_bilinear_baseline():
    img = np.arange(12, dtype=np.float64).reshape(3, 4, 1)
    assert np.array_equal(upsample_ref.bilinear(img, 3, 4), img)  # same size: the image
    up = upsample_ref.bilinear(img, 6, 8)
    assert np.array_equal(up[::2, ::2], img)  # X * w / W is whole at even X
    assert up[0, 1, 0] == 0.5 and up[1, 0, 0] == 2.0 and up[0, 7, 0] == 3.0 and up[5, 0, 0] == 8.0  # the last tap is clamped


def test_upsample_params_layout_and_defaults():
    from rsoderh_raytracing_amd import state
    assert C.sizeof(state.UpsampleParams) == 12
    assert [f[0] for f in state.UpsampleParams._fields_] == ["flags", "sigma_normal", "sigma_depth"]
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "flags RSRT_UPSAMPLE_DEMODULATE, sigma_normal 0.5, sigma_depth 0.3" in hdr
    assert "RSRT_UPSAMPLE_DEMODULATE = 1u, RSRT_UPSAMPLE_DENOISED = 2u, RSRT_UPSAMPLE_TEMPORAL = 4u" in hdr
    assert state.UPSAMPLE_DEFAULTS == {"sigma_normal": 0.5, "sigma_depth": 0.3, "demodulate": True}
    assert (state.UPSAMPLE_DEMODULATE, state.UPSAMPLE_DENOISED, state.UPSAMPLE_TEMPORAL) == (1, 2, 4)
    up = open(os.path.join(util.ROOT, "include", "rsrt_upsample.h")).read()
    assert "#define RSRT_UP_SIGMA_NORMAL 0.5f" in up and "#define RSRT_UP_SIGMA_DEPTH 0.3f" in up
    assert (upsample_ref.SIGMA_NORMAL, upsample_ref.SIGMA_DEPTH) == (0.5, 0.3)


def test_library_exports_the_upsampler():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_guide_render", "rsrt_guide_bind", "rsrt_guide_clear", "rsrt_guide_download", "rsrt_upsample", "rsrt_upsampled_download",
              "rsrt_upsampled_display_srgb8"):
        assert hasattr(lib, n), n
    for m in ("render_guide", "bind_guide", "clear_guide", "download_guide", "upsample", "upsampled_display_srgb8", "render_upsampled"):
        assert hasattr(R.State, m), m


def test_up_kernel_uses_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = [n for n in md if "rt_up_kernel" in n]
    assert len(names) == 1, names
    k = md[names[0]]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "upsample_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "upsample_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_upsampler_compiles(tmp_path):
    build_cpp_demo(tmp_path)
