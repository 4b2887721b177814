"""Local exposure without a GPU: its published arithmetic (include/rsrt_local.h), compiled for the CPU, against the numpy restatement
the GPU tests hold the kernels to (tests/local_ref.py), bit for bit, special pixels included: the q map, the raw and the blurred grid,
the gains and the display bytes; q against the meter's word; den > 0; rsrt_local_exp2's bounds; the strength-0 identities; the no-halo
step; the constant image; monotonicity in the strengths; the max_stops clamp; the parameter check; the ABI and the kernels' code
objects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_ref
import exposure_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

# (h, w, cell)
CASES = [(1, 1, 8), (1, 7, 8), (2, 2, 8), (3, 5, 8), (7, 9, 8), (8, 8, 8), (9, 17, 8), (17, 65, 8), (33, 65, 32), (33, 65, 64), (70, 130, 32), (70, 130, 64)]
F = np.float32


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def seed_of(h, w):
    return 1000 * h + w


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("local") / "liblocal.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "local_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.local_q_map.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.local_q.argtypes = [C.c_float]
    L.local_q.restype = C.c_uint32
    L.local_meter_word.argtypes = [C.c_float]
    L.local_meter_word.restype = C.c_uint32
    L.local_raw_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_void_p]
    L.local_blur.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.local_gains.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.local_display.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.local_exp2.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.local_params_ok.argtypes = [C.c_void_p]
    L.local_cell_ok.argtypes = [C.c_uint32]
    L.local_defaults.argtypes = [C.c_void_p, C.c_void_p]
    L.local_layout.argtypes = [C.c_void_p]

    def params(**kw):
        q = dict(local_ref.DEFAULTS, **kw)
        return state.LocalParams(q["shadows"], q["highlights"], q["key"], q["max_stops"], q.get("flags", 0), 0)

    class Host:
        @staticmethod
        def q_map(sums, total):
            sums = np.ascontiguousarray(sums, F)
            out = np.full(sums.shape[:2], 7, np.uint32)
            L.local_q_map(sums.ctypes.data, out.size, total, out.ctypes.data)
            return out

        @staticmethod
        def raw_grid(sums, total, cell):
            sums = np.ascontiguousarray(sums, F)
            h, w = sums.shape[:2]
            out = np.full((local_ref.GZ, local_ref.cells(h, cell), local_ref.cells(w, cell), 2), 7, np.uint32)
            L.local_raw_grid(sums.ctypes.data, h, w, total, cell, out.ctypes.data)
            return out

        @staticmethod
        def blur(grid):
            out = np.ascontiguousarray(grid, np.uint32).copy()
            L.local_blur(out.ctypes.data, out.shape[2], out.shape[1])
            return out

        @staticmethod
        def gains(sums, total, exposure, grid, cell, **kw):
            """(base, den > 0, gain), each [h, w]."""
            sums, grid = np.ascontiguousarray(sums, F), np.ascontiguousarray(grid, np.uint32)
            h, w = sums.shape[:2]
            base, den, gain = np.full((h, w), 7, F), np.full((h, w), 7, np.uint8), np.full((h, w), 7, F)
            p = params(**kw)
            L.local_gains(sums.ctypes.data, h, w, total, exposure, C.byref(p), grid.ctypes.data, cell, base.ctypes.data, den.ctypes.data, gain.ctypes.data)
            return base, den.astype(bool), gain

        @staticmethod
        def display(sums, total, exposure, gain, intensity=0.0, b=None):
            sums, gain = np.ascontiguousarray(sums, F), np.ascontiguousarray(gain, F)
            h, w = sums.shape[:2]
            out = np.zeros((h, w, 4), np.uint8)
            b = None if b is None else np.ascontiguousarray(b, F)
            L.local_display(sums.ctypes.data, h, w, total, exposure, gain.ctypes.data, intensity, None if b is None else b.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def exp2(e):
            e = np.ascontiguousarray(e, F)
            out = np.empty_like(e)
            L.local_exp2(e.ctypes.data, e.size, out.ctypes.data)
            return out

        @staticmethod
        def ok(**kw):
            p = params(**kw)
            return bool(L.local_params_ok(C.byref(p)))
    Host.L = L
    return Host


@pytest.mark.parametrize("h,w,cell", CASES)
def test_header_arithmetic_matches_numpy_bit_for_bit(host, h, w, cell):
    sums, special = local_ref.synthetic(h, w, seed=seed_of(h, w))
    assert bool(special) == (h * w >= 16)
    flat = lambda a: a.reshape(-1)  # noqa: E731
    for total in (1, 3):
        q = host.q_map(sums, total)
        assert np.array_equal(q, local_ref.q_map(sums, total))
        if special:  # skipped or clamped as documented
            for name in ("nan", "neg_inf", "negative", "neg_zero"):
                assert flat(q)[special[name]] == local_ref.SKIPPED, name
            assert flat(q)[special["denormal"]] == 0 and flat(q)[special["inf"]] == 8191 and flat(q)[special["huge"]] == 8191
        raw = host.raw_grid(sums, total, cell)
        assert np.array_equal(raw, local_ref.raw_grid(q, cell))
        counted = q != local_ref.SKIPPED
        assert raw[..., 0].sum() == counted.sum() and raw[..., 1].sum() == q[counted].astype(np.int64).sum()
        grid = host.blur(raw)
        assert np.array_equal(grid, local_ref.blur(raw)) and np.array_equal(grid, local_ref.grid_of(sums, total, cell))
        b = bloom_ref.bloom(sums, total, 0.37, 3)
        for exposure in (1.0, 0.37, 40.0):
            for kw in ({}, {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}, {"shadows": 0.0, "highlights": 1.0, "max_stops": 16.0}):
                case = (total, exposure, kw)
                base, den, gain = host.gains(sums, total, exposure, grid, cell, **kw)
                assert den[counted].all() and not den[~counted].any(), case  # every counted pixel finds den > 0
                assert same(base[counted], local_ref.base_of(grid, q, cell)[counted]), case
                want = local_ref.gains(sums, total, exposure, grid, cell, **kw)
                assert same(gain, want), case
                assert np.isfinite(gain).all() and (gain > 0).all() and (gain[~counted] == 1).all(), case
                assert np.array_equal(host.display(sums, total, exposure, gain), local_ref.display(sums, total, exposure, want)), case
            if exposure == 0.37:
                assert np.array_equal(host.display(sums, total, exposure, gain, 0.5, b), local_ref.display(sums, total, exposure, want, 0.5, b)), case


def test_q_is_the_meters_word_in_finer_steps(host):
    rng = np.random.default_rng(1)
    lum = np.concatenate([np.exp(rng.uniform(-60, 60, 4000)), [2.0 ** -16, 2.0 ** 16, 1e-45, 1e-41, 3e38, np.inf, 1.0, 0.18],
                          np.nextafter(F(2.0) ** np.arange(-18, 19, dtype=F), F(0)), F(2.0) ** np.arange(-18, 19, dtype=F)]).astype(F)
    q = local_ref.q_of_luminance(lum)
    assert np.array_equal(q >> 5, exposure_ref.words(lum)) and q.max() == 8191 and q.min() == 0
    for v in lum[::7]:
        assert host.L.local_q(v) == local_ref.q_of_luminance(v) and host.L.local_q(v) >> 5 == host.L.local_meter_word(v), v
    # exact at powers of two: 256 steps an octave from 2^-16
    assert [int(local_ref.q_of_luminance(F(2.0) ** k)) for k in (-16, -4, 0, 4, 15)] == [0, 3072, 4096, 5120, 7936]


def test_exp2_is_exact_at_integers_monotone_and_within_2_to_the_minus_12(host):
    ints = np.arange(-16, 17, dtype=F)
    e = np.unique(np.concatenate([np.arange(-16 * 4096, 16 * 4096 + 1, dtype=np.float64) / 4096, ints, np.nextafter(ints, F(-np.inf))[1:],
                                  np.nextafter(ints, F(np.inf))[:-1]]).astype(F))
    assert e[0] == -16 and e[-1] == 16 and (np.diff(e) > 0).all()
    got = host.exp2(e)
    assert same(got, local_ref.exp2(e))
    at = np.isin(e, ints)
    assert at.sum() == 33 and same(got[at], F(2.0) ** e[at])  # exact at integers
    assert (np.diff(got) >= 0).all()  # monotone non-decreasing, the float neighbours of the integers included
    rel = np.abs(got.astype(np.float64) / 2.0 ** e.astype(np.float64) - 1)
    print("rsrt_local_exp2: largest relative error %.3g (2^%.2f)" % (rel.max(), np.log2(rel.max())))
    assert rel.max() <= 2.0 ** -12
    assert same(host.exp2(F([0.0, -0.0])), F([1, 1]))


@pytest.mark.parametrize("h,w,cell", CASES)
def test_strength_zero_is_the_exposed_and_the_bloomed_display(host, h, w, cell):
    sums, _ = local_ref.synthetic(h, w, seed=seed_of(h, w))
    for total in (1, 3):
        grid = host.blur(host.raw_grid(sums, total, cell))
        for exposure in (1.0, 0.37):
            _, _, gain = host.gains(sums, total, exposure, grid, cell, shadows=0.0, highlights=0.0)
            assert same(gain, np.ones((h, w), F))  # exactly 1: e is +-0
            assert same(local_ref.gains(sums, total, exposure, grid, cell, shadows=0.0, highlights=0.0), gain)
            plain = exposure_ref.display(sums, total, exposure)
            assert np.array_equal(host.display(sums, total, exposure, gain), plain)
            assert np.array_equal(local_ref.display(sums, total, exposure, gain), plain)
            b = bloom_ref.bloom(sums, total, exposure, 2)
            bloomed = bloom_ref.display(sums, total, exposure, 0.5, b)
            assert np.array_equal(host.display(sums, total, exposure, gain, 0.5, b), bloomed)
            assert np.array_equal(local_ref.display(sums, total, exposure, gain, 0.5, b), bloomed)
    if h * w >= 16:  # ... and the default strengths do change the picture
        _, _, gain = host.gains(sums, 1, 1.0, grid, cell)
        assert not np.array_equal(host.display(sums, 1, 1.0, gain), exposure_ref.display(sums, 1, 1.0))


@pytest.mark.parametrize("edge", [64, 48])
def test_a_step_of_eight_octaves_has_no_halo(host, edge):
    """Two flat regions three or more octave planes apart share no cell of the blurred grid, so each side's base is its own q:
    nothing of the other side leaks across the edge, at any distance from it."""
    h, w, cell = 96, 128, 32
    sums = np.ones((h, w, 4), F)
    sums[:, :edge, :3] = 2.0 ** -4
    sums[:, edge:, :3] = 2.0 ** 4
    q = host.q_map(sums, 1)
    assert sorted(set(q.ravel() >> 8)) == [12, 20]
    grid = host.blur(host.raw_grid(sums, 1, cell))
    base, den, _ = host.gains(sums, 1, 1.0, grid, cell)
    assert den.all() and same(base, local_ref.base_of(grid, q, cell))
    print("largest |base - q| across the step: %g" % np.abs(base - q.astype(F)).max())
    assert np.array_equal(base, q.astype(F))  # the difference is 0
    # so a pixel at the edge has the gain of one far from it
    _, _, gain = host.gains(sums, 1, 1.0, grid, cell, shadows=1.0, highlights=1.0, max_stops=16.0)
    assert len(np.unique(gain[:, :edge])) == 1 and len(np.unique(gain[:, edge:])) == 1 and gain[0, 0] > 1 > gain[0, -1]


@pytest.mark.parametrize("h,w,cell", [(1, 1, 8), (9, 17, 8), (33, 65, 32), (70, 130, 64), (70, 130, 16)])
def test_a_constant_image_at_the_key_keeps_its_exposure(host, h, w, cell):
    for exposure in (1.0, 0.37, 8.0):
        c = F(F(local_ref.DEFAULTS["key"]) / F(exposure))
        sums = np.ones((h, w, 4), F)
        sums[..., :3] = c
        q = host.q_map(sums, 1)
        assert q.min() == q.max() == local_ref.mid_of(local_ref.DEFAULTS["key"], exposure)  # (the luminance of a grey is the grey, to an ulp)
        grid = host.blur(host.raw_grid(sums, 1, cell))
        base, den, gain = host.gains(sums, 1, exposure, grid, cell, shadows=1.0, highlights=1.0)
        err = np.abs(base.astype(np.float64) - q)
        print("constant image %dx%d cell %d exposure %g: largest |base - q| %.3g Q8 units, largest |gain - 1| %.3g" %
              (h, w, cell, exposure, err.max(), np.abs(gain.astype(np.float64) - 1).max()))
        assert den.all() and err.max() <= 2.0 ** -7  # sixteen f32 roundings on values up to 2^13
        assert np.abs(gain.astype(np.float64) - 1).max() <= 2.0 ** -12
        shown, plain = host.display(sums, 1, exposure, gain), exposure_ref.display(sums, 1, exposure)
        assert np.abs(shown.astype(int) - plain.astype(int)).max() <= 1


def test_gain_is_monotone_in_the_strengths_and_clamped_by_max_stops(host):
    h, w, cell = 70, 130, 32
    sums, _ = local_ref.synthetic(h, w, seed=11)
    total, exposure = 1, 0.8
    q = host.q_map(sums, total)
    counted = q != local_ref.SKIPPED
    grid = host.blur(host.raw_grid(sums, total, cell))
    base, _, _ = host.gains(sums, total, exposure, grid, cell)
    mid = local_ref.mid_of(local_ref.DEFAULTS["key"], exposure)
    above, below = counted & (base > mid), counted & (base < mid)
    assert above.sum() > 100 and below.sum() > 100
    steps = (0.0, 0.25, 0.5, 0.75, 1.0)
    by_h = [host.gains(sums, total, exposure, grid, cell, highlights=s, max_stops=16.0)[2] for s in steps]
    by_s = [host.gains(sums, total, exposure, grid, cell, shadows=s, max_stops=16.0)[2] for s in steps]
    for a, b in zip(by_h, by_h[1:]):
        assert (b[above] <= a[above]).all() and same(b[below], a[below])  # highlights: non-increasing above the key, nothing below it
    for a, b in zip(by_s, by_s[1:]):
        assert (b[below] >= a[below]).all() and same(b[above], a[above])
    assert (by_h[-1][above] <= 1).all() and (by_h[-1][above] < 1).any() and (by_s[-1][below] >= 1).all() and (by_s[-1][below] > 1).any()
    # the clamp: no gain moves a pixel by more than max_stops, and with strengths 1 some reach it
    for stops in (0.0, 0.5, 2.0):
        g = host.gains(sums, total, exposure, grid, cell, shadows=1.0, highlights=1.0, max_stops=stops)[2]
        lo, hi = host.exp2(F([-stops, stops]))
        assert (g >= lo).all() and (g <= hi).all() and (g == lo).any() and (g == hi).any(), stops
        assert same(g, local_ref.gains(sums, total, exposure, grid, cell, shadows=1.0, highlights=1.0, max_stops=stops))
    assert same(host.gains(sums, total, exposure, grid, cell, shadows=1.0, highlights=1.0, max_stops=0.0)[2], np.ones((h, w), F))


def test_params_ok_accepts_and_rejects(host):
    good = [{}, {"shadows": 0.0}, {"shadows": 1.0}, {"highlights": 0.0}, {"highlights": 1.0}, {"key": 1e-30}, {"key": 3e38}, {"max_stops": 0.0},
            {"max_stops": 16.0}, {"shadows": -0.0}]
    bad = [{k: v} for k in ("shadows", "highlights") for v in (-0.001, 1.001, float("nan"), float("inf"), float("-inf"))]
    bad += [{"key": v} for v in (0.0, -0.18, float("nan"), float("inf"))]
    bad += [{"max_stops": v} for v in (-0.5, 16.5, float("nan"), float("inf"))]
    bad += [{"flags": v} for v in (1, 2, 0x80000000)]
    d = {k: v for k, v in local_ref.DEFAULTS.items() if k != "cell"}
    for kw in good:
        assert host.ok(**kw) and local_ref.params_ok(**dict(d, **kw)), kw
    for kw in bad:
        assert not host.ok(**kw) and not local_ref.params_ok(**dict(d, **kw)), kw
    for cell in range(0, 130):
        assert bool(host.L.local_cell_ok(cell)) == (cell in local_ref.CELLS) == (cell in state.LOCAL_CELLS), cell


def test_struct_layout_and_defaults(host):
    lay = np.zeros(7, np.uint32)
    host.L.local_layout(lay.ctypes.data)
    P = state.LocalParams
    assert list(lay) == [C.sizeof(P), P.highlights.offset, P.key.offset, P.max_stops.offset, P.flags.offset, P._pad.offset, state.LOCAL_GZ]
    assert C.sizeof(P) == 24 and [f[0] for f in P._fields_] == ["shadows", "highlights", "key", "max_stops", "flags", "_pad"]
    d, cell = P(), C.c_uint32()
    host.L.local_defaults(C.byref(d), C.byref(cell))
    got = {"cell": cell.value, "shadows": d.shadows, "highlights": d.highlights, "key": d.key, "max_stops": d.max_stops}
    want = {k: (v if isinstance(v, int) else float(F(v))) for k, v in local_ref.DEFAULTS.items()}
    assert got == want == {"cell": 32, "shadows": 0.5, "highlights": 0.5, "key": float(F(0.18)), "max_stops": 4.0} and (d.flags, d._pad) == (0, 0)
    assert {k: (v if isinstance(v, int) else float(F(v))) for k, v in state.LOCAL_DEFAULTS.items()} == want
    assert local_ref.GZ == state.LOCAL_GZ == 32
    import inspect
    sig = inspect.signature(R.State.local_exposure).parameters
    assert [sig[k].default for k in ("source", "cell", "sample_total", "stream")] == ["mean", None, None, None]
    sig = inspect.signature(R.State.display_local_srgb8).parameters
    assert [sig[k].default for k in ("source", "exposure", "shadows", "highlights", "bloom_intensity", "sample_total")] == ["mean", None, None, None, 0.0, None]
    assert inspect.signature(R.State.local_gain).parameters["exposure"].default is None


SYMBOLS = ("rsrt_local_exposure", "rsrt_local_exposure_download", "rsrt_local_exposure_reset", "rsrt_local_gain_download", "rsrt_display_local_srgb8")


def test_library_exports_local_exposure():
    lib = C.CDLL(_build.build_hip())
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    for m in ("local_exposure", "local_exposure_download", "local_exposure_reset", "local_gain", "display_local_srgb8"):
        assert hasattr(R.State, m), m
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    for n in SYMBOLS:
        assert "Rust: pub fn %s(" % n in hdr, n  # every entry point carries its Rust signature


KERNELS = ("rt_local_splat_kernel", "rt_local_blur_kernel", "rt_display_local_kernel", "rt_local_gain_kernel")


def test_local_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def tile_constants():
    """RT_LC_PW, RT_LC_PH — the splat workgroup's pixel block — and RT_LC_TW, RT_LC_TH — the display tile — from the source's #defines."""
    import re
    src = open(os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip", "rt_local.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)\b" % n, src).group(1)) for n in ("RT_LC_PW", "RT_LC_PH", "RT_LC_TW", "RT_LC_TH"))


def test_tile_constants_are_readable():
    pw, ph, tw, th = tile_constants()
    assert pw % 64 == 0 and ph % 64 == 0 and tw >= 1 and th >= 1 and tw * th <= 1024


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "local_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "local_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_local_exposure_compiles(tmp_path):
    build_cpp_demo(tmp_path)
