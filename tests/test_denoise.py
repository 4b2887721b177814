"""The denoiser without a GPU: its published per-pixel arithmetic (include/rsrt_denoise.h), compiled for the CPU, against the numpy
restatement the GPU tests hold the kernels to (tests/denoise_ref.py), bit for bit; the ABI and the parameter defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build


@pytest.fixture(scope="module")
def host_filter(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dn") / "libdn.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "denoise_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.dn_filter.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_float] * 3 + [C.c_int, C.c_void_p]

    def run(sums, aov, S, T, L_, sc, sn, sz, demod):
        h, w = sums.shape[:2]
        sums, aov = np.ascontiguousarray(sums, np.float32), np.ascontiguousarray(aov, np.float32)
        out = np.zeros((h, w, 3), np.float32)
        L.dn_filter(sums.ctypes.data, aov.ctypes.data, w, h, S, T, L_, sc, sn, sz, int(demod), out.ctypes.data)
        return out
    return run


def synthetic(h, w, spp, aov_spp, seed, miss_frac=0.2):
    """Noisy sums and AOV records with two materials, a normal step, a depth ramp and pixels without hits."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = np.where((xs < w // 2)[..., None], np.float32([0.8, 0.3, 0.2]), np.float32([0.2, 0.5, 0.9]))
    sums = np.zeros((h, w, 4), np.float32)
    sums[..., :3] = (base * spp + rng.normal(0, 0.6, (h, w, 3)) * np.sqrt(spp)).astype(np.float32)
    sums[..., 3] = 1.0
    hits = rng.integers(0, aov_spp + 1, (h, w)).astype(np.float32)
    hits[rng.random((h, w)) < miss_frac] = 0.0
    aov = np.zeros((h, w, 8), np.float32)
    aov[..., :3] = (base * 0.9 * hits[..., None]).astype(np.float32)
    aov[..., 3] = hits
    nrm = np.where((ys < h // 2)[..., None], np.float32([0, 1, 0]), np.float32([0, 0.6, 0.8]))
    aov[..., 4:7] = (nrm * hits[..., None] + rng.normal(0, 0.01, (h, w, 3)) * hits[..., None]).astype(np.float32)
    aov[..., 7] = ((3.0 + 0.01 * xs) * hits).astype(np.float32)
    return sums, aov


@pytest.mark.parametrize("h,w", [(91, 173), (1, 1), (300, 7)])
@pytest.mark.parametrize("iters", [0, 1, 3, 6])
@pytest.mark.parametrize("demod", [True, False])
def test_header_arithmetic_matches_numpy_bit_for_bit(host_filter, h, w, iters, demod):
    sums, aov = synthetic(h, w, 4, 3, seed=h * 1000 + w + iters)
    args = (4, 3, iters, 2.0, 0.3, 0.2, demod)
    got = host_filter(sums, aov, *args)
    want = denoise_ref.denoise(sums, aov, 4, 3, iters, 2.0, 0.3, 0.2, demod)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if iters == 0:
        assert np.array_equal(got, sums[..., :3] / np.float32(4))


def test_fma32_is_the_correctly_rounded_fma():
    """The restated camera ray uses f32 fma (the kernels' dot / mat3_mul); fma32 against exact rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a, b, c = (rng.standard_normal(3000).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, 3000).astype(np.float32) for _ in range(3))
    got = denoise_ref.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = Fraction(float(got[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(g - exact) <= abs(Fraction(float(lo)) - exact) and abs(g - exact) <= abs(Fraction(float(hi)) - exact), i


def test_denoise_params_layout_and_defaults():
    from rsoderh_raytracing_amd import state
    assert C.sizeof(state.DenoiseParams) == 20
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "iterations 5 (0..8" in hdr and "sigma_color 2.0, sigma_normal 0.5, sigma_depth 0.3" in hdr
    assert state.DENOISE_DEFAULTS == {"iterations": 5, "sigma_color": 2.0, "sigma_normal": 0.5, "sigma_depth": 0.3, "demodulate": True}


def test_library_exports_the_denoiser():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_aov_render", "rsrt_aov_bind", "rsrt_aov_clear", "rsrt_aov_download", "rsrt_denoise", "rsrt_denoised_download",
              "rsrt_denoised_display_srgb8"):
        assert hasattr(lib, n), n
    assert hasattr(R.State, "denoise") and hasattr(R.State, "render_aov")


def test_new_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = [n for n in md if any(k in n for k in ("rt_aov_kernel", "rt_dn_prepare_kernel", "rt_dn_level_kernel"))]
    assert len(names) == 5, names
    for n in names:
        assert md[n]["private_segment_fixed_size"] == 0 and md[n]["vgpr_spill_count"] == 0, (n, md[n])


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "denoise_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "denoise_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_denoiser_compiles(tmp_path):
    build_cpp_demo(tmp_path)
