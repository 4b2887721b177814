"""The noise estimate without a GPU: its published arithmetic (include/rsrt_noise.h), compiled for the CPU, against the numpy
restatement the GPU tests hold the kernel to (tests/noise_ref.py), bit for bit, special pixels and partial tiles included; the ABI,
the parameter defaults and the kernel's code object; and on checker-rendered frames that the estimate falls as the samples grow and
sits where the true error sits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import noise_ref
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build

FRAMES = [(37, 70), (1, 1), (4, 64), (7, 300)]  # (h, w)
TILES = [(16, 16), (8, 8), (64, 1), (1, 64), (128, 32)]  # (tile_w, tile_h); the last is larger than most of the frames
COUNTS = [(4, 8), (3, 8)]


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


@pytest.fixture(scope="module")
def host_noise(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("noise") / "libnoise.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "noise_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.noise_tiles.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
    L.noise_tiles.restype = C.c_uint32

    def run(s1, n1, s2, n2, tile, threshold=0.0):
        s1, s2 = (np.ascontiguousarray(a, np.float32) for a in (s1, s2))
        h, w = s1.shape[:2]
        tiles = np.zeros((-(-h // tile[1]), -(-w // tile[0])), np.float32)
        summ = np.zeros(2, np.float32)
        above = L.noise_tiles(s1.ctypes.data, s2.ctypes.data, w, h, n1, n2, tile[0], tile[1], threshold, tiles.ctypes.data, summ.ctypes.data)
        return tiles, {"max_error": float(summ[0]), "mean_error": float(summ[1]), "tiles_x": tiles.shape[1], "tiles_y": tiles.shape[0],
                       "tiles_above": above}
    return run


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n1,n2", COUNTS)
def test_header_arithmetic_matches_numpy_bit_for_bit(host_noise, h, w, tile, n1, n2):
    s1, s2, special = noise_ref.synthetic(h, w, n1, n2, seed=1000 * h + w)
    threshold = 0.25
    got, gs = host_noise(s1, n1, s2, n2, tile, threshold)
    want, ws = noise_ref.estimate(s1, n1, s2, n2, tile, threshold)
    assert got.shape == want.shape == (-(-h // tile[1]), -(-w // tile[0]))
    assert not np.isnan(got).any() and (got >= 0).all()
    assert same(got, want)
    assert gs["tiles_above"] == ws["tiles_above"] and same(gs["max_error"], ws["max_error"]) and same(gs["mean_error"], ws["mean_error"])
    e = noise_ref.pixel_error(s1, n1, s2, n2).ravel()
    if special:
        assert e[special["zero"]] == 0.0 and np.isfinite(e[special["negative"]]) and e[special["negative"]] > 0
        bad = set()
        for k in ("inf", "nan", "nan_snapshot"):  # a non-finite pixel makes its tile +inf, and that tile counts as above any threshold
            assert e[special[k]] == np.inf
            y, x = divmod(special[k], w)
            assert got[y // tile[1], x // tile[0]] == np.inf
            bad.add((y // tile[1], x // tile[0]))
        assert int(np.isinf(got).sum()) == len(bad) and gs["max_error"] == np.inf and gs["mean_error"] == np.inf
        _, inf_thr = host_noise(s1, n1, s2, n2, tile, float("inf"))
        assert inf_thr["tiles_above"] == len(bad) == noise_ref.summary(want, np.inf)["tiles_above"]
    else:
        assert np.isfinite(got).all()


@pytest.mark.parametrize("tile", TILES)
def test_equal_means_give_zeros(host_noise, tile):
    s1, _, _ = noise_ref.synthetic(37, 70, 4, 8, seed=9)
    s1 = np.abs(np.nan_to_num(s1, nan=1.0, posinf=1.0))
    s2 = s1 * np.float32(2)  # exact: S2 / 8 == S1 / 4
    got, gs = host_noise(s1, 4, s2, 8, tile)
    assert not got.any() and gs["max_error"] == 0.0 and gs["mean_error"] == 0.0 and gs["tiles_above"] == 0
    want, ws = noise_ref.estimate(s1, 4, s2, 8, tile)
    assert same(got, want) and ws["tiles_above"] == 0


def test_bad_tiles_are_refused(host_noise):
    s = np.ones((4, 4, 4), np.float32)
    for tile in ((8, 6), (128, 64), (65536, 65536)):  # 48 pixels, 8192 pixels, a product that wraps to 0 in 32 bits
        assert not noise_ref.tile_ok(*tile)
        assert host_noise(s, 1, s, 2, tile)[1]["tiles_above"] == 0xffffffff
    for tile in TILES + [(64, 64), (4096, 1)]:
        assert noise_ref.tile_ok(*tile)
        assert host_noise(s, 1, s + s, 2, tile)[1]["tiles_above"] == 0


def test_noise_struct_layouts_and_defaults():
    from rsoderh_raytracing_amd import state
    assert C.sizeof(state.NoiseParams) == 16 and C.sizeof(state.NoiseSummary) == 24
    assert [f[0] for f in state.NoiseParams._fields_] == ["tile_w", "tile_h", "threshold", "flags"]
    assert [f[0] for f in state.NoiseSummary._fields_] == ["max_error", "mean_error", "tiles_x", "tiles_y", "tiles_above", "_pad"]
    assert state.NoiseSummary.tiles_x.offset == 8 and state.NoiseSummary.tiles_above.offset == 16
    assert state.NOISE_DEFAULTS == {"tile": (16, 16), "threshold": 0.0}
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "rsrt_noise_params defaults: tile_w 16, tile_h 16, threshold 0, flags 0" in hdr
    ns = open(os.path.join(util.ROOT, "include", "rsrt_noise.h")).read()
    assert "#define RSRT_NOISE_EPS 1.0e-3f" in ns and "#define RSRT_NOISE_TILE_W 16u" in ns and "#define RSRT_NOISE_TILE_H 16u" in ns
    assert noise_ref.EPS == np.float32(1e-3) and noise_ref.TILE == (16, 16)
    import inspect
    sig = inspect.signature(R.State.render_to_noise).parameters
    assert (sig["min_samples"].default, sig["max_samples"].default, sig["tile"].default) == (8, 1024, (16, 16))
    sig = inspect.signature(R.State.noise_estimate).parameters
    assert (sig["tile"].default, sig["threshold"].default) == ((16, 16), 0.0)


def test_library_exports_the_noise_estimate():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_noise_snapshot", "rsrt_noise_estimate", "rsrt_noise_download", "rsrt_noise_reset"):
        assert hasattr(lib, n), n
    for m in ("noise_snapshot", "noise_estimate", "noise_download", "noise_reset", "render_to_noise"):
        assert hasattr(R.State, m), m


def test_noise_kernel_uses_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = [n for n in md if "rt_noise_tile_kernel" in n]
    assert len(names) == 1, names
    k = md[names[0]]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "noise_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "noise_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_noise_estimate_compiles(tmp_path):
    build_cpp_demo(tmp_path)


# -- on rendered frames ------------------------------------------------------------------------------------------------------------
_frames = {}


def checker_frames(name, w, h):
    """The checker's sums of samples [0, n) for n = 4, 8, 32, 64 and of the disjoint samples [1000, 1512): rendered once a scene."""
    if name not in _frames:
        sc = R.Scene.load_toml(util.scene_path(name))
        args = (util.oracle_scene(sc), util.oracle_env(util.small_env()), sc.camera_uniform().view(oracle.CAMERA), w, h)
        acc = np.zeros((h, w, 4), np.float32)
        sums, at = {}, 0
        for n in (4, 8, 32, 64):
            oracle.render(*args, at, n - at, 8, sum_rgba=acc, fast=True)
            sums[n], at = acc.copy(), n
        ref, _ = oracle.render(*args, 1000, 512, 8, fast=True)
        for a in list(sums.values()) + [ref]:
            a.setflags(write=False)
        _frames[name] = (sums, ref)
    return _frames[name]


SCENES = [("house", 96, 54), ("suzanne", 80, 48)]


@pytest.mark.parametrize("name,w,h", SCENES)
def test_estimate_falls_as_the_samples_grow(name, w, h):
    """16 x 16 tiles; the issue's own run of this restatement: mean tile error house 9.82 -> 5.44, suzanne 7.77 -> 3.08; max tile error
    house 19.7 -> 9.95, suzanne 19.1 -> 7.51 (the contract's f32 sums print the same digits)."""
    sums, _ = checker_frames(name, w, h)
    _, lo = noise_ref.estimate(sums[4], 4, sums[8], 8)
    _, hi = noise_ref.estimate(sums[32], 32, sums[64], 64)
    print("%s %dx%d: mean tile error (4, 8) %.6f -> (32, 64) %.6f; max %.6f -> %.6f" % (name, w, h, lo["mean_error"], hi["mean_error"],
                                                                                      lo["max_error"], hi["max_error"]))
    assert np.isfinite([lo["max_error"], hi["max_error"]]).all()
    assert hi["mean_error"] < lo["mean_error"]
    assert hi["max_error"] < lo["max_error"]


@pytest.mark.parametrize("name,w,h", SCENES)
def test_estimate_sits_where_the_true_error_sits(name, w, h):
    """The frame mean of the estimate at (32, 64) over the frame mean of the true error of the 64-sample mean, sum |m - ref| /
    sqrt(max(sum ref, 0) + 1e-3) against 512 spp of the disjoint samples 1000-1511, both through the contract's f32 tile sums: within
    [0.7, 1.1].  The issue's throwaway run (f64 tile sums) gave 0.893 on house and 0.877 on suzanne; below 1 because the reference
    carries noise of its own."""
    sums, ref = checker_frames(name, w, h)
    tiles, s = noise_ref.estimate(sums[32], 32, sums[64], 64)
    F = np.float32
    m, r = sums[64][..., :3] / F(64), ref[..., :3] / F(512)
    d = np.abs(m - r)
    true = ((d[..., 0] + d[..., 1]) + d[..., 2]) / np.sqrt(np.maximum((r[..., 0] + r[..., 1]) + r[..., 2], F(0)) + noise_ref.EPS)
    true_mean = noise_ref.summary(noise_ref.tile_errors(true.astype(F)))["mean_error"]
    ratio = s["mean_error"] / true_mean
    print("%s %dx%d: estimate %.6f, true error %.6f, ratio %.4f" % (name, w, h, s["mean_error"], true_mean, ratio))
    assert 0.7 <= ratio <= 1.1
