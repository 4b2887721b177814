"""Auto-exposure without a GPU: its published arithmetic (include/rsrt_exposure.h), compiled for the CPU, against the numpy
restatement the GPU tests hold the kernels to (tests/exposure_ref.py), bit for bit, special pixels included; power-of-two invariance;
the exposed display at exposure 1 against the plain one; degenerate histograms; the parameter check; the ABI and the kernels' code
objects; and on checker-rendered frames that the meter reads the true log-average."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exposure_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(37, 70), (1, 1), (4, 64), (7, 300)]  # (h, w)
TOTALS = [1, 3]
F = np.float32
# the defaults; everything; a sliver in the middle; a clamp that bites from either side; adaptation from a previous exposure
PARAM_SETS = [{}, {"low_permille": 0, "high_permille": 1000}, {"low_permille": 499, "high_permille": 500},
              {"min_exposure": 4.0, "max_exposure": 8.0}, {"min_exposure": 2.0 ** -10, "max_exposure": 2.0 ** -9},
              {"blend": 0.0, "previous_exposure": 0.7}, {"blend": 0.25, "previous_exposure": 0.7}, {"blend": 1.0, "previous_exposure": 0.7}]


def bits(x):
    return np.asarray(x, F).view(np.uint32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("exposure") / "libexposure.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "exposure_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.exposure_histogram.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    L.exposure_params_ok.argtypes = [C.c_void_p]
    L.exposure_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.exposure_defaults.argtypes = [C.c_void_p]
    L.exposure_display.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_void_p]
    L.exposure_layout.argtypes = [C.c_void_p]

    class Host:
        @staticmethod
        def params(**kw):
            q = dict(exposure_ref.DEFAULTS, **kw)
            return state.ExposureParams(q["low_permille"], q["high_permille"], q["key"], q["min_exposure"], q["max_exposure"], q["blend"],
                                        q["previous_exposure"], 0)

        @staticmethod
        def histogram(sums, total):
            sums = np.ascontiguousarray(sums, F)
            hist = np.full(exposure_ref.WORDS, 7, np.uint32)
            L.exposure_histogram(sums.ctypes.data, sums.size // 4, total, hist.ctypes.data)
            return hist

        @staticmethod
        def result(hist, **kw):
            p, r = Host.params(**kw), state.ExposureResult()
            hist = np.ascontiguousarray(hist, np.uint32)
            L.exposure_result(hist.ctypes.data, C.byref(p), C.byref(r))
            return {"exposure": F(r.exposure), "target": F(r.target), "average_luminance": F(r.average_luminance), "metered": r.metered,
                    "skipped": r.skipped}

        @staticmethod
        def ok(**kw):
            p = Host.params(**kw)
            return bool(L.exposure_params_ok(C.byref(p)))

        @staticmethod
        def display(sums, total, exposure=None):
            sums = np.ascontiguousarray(sums, F)
            out = np.zeros(sums.shape[:-1] + (4,), np.uint8)
            L.exposure_display(sums.ctypes.data, sums.size // 4, total, 1.0 if exposure is None else exposure, exposure is not None, out.ctypes.data)
            return out
    Host.L = L
    return Host


def same_result(got, want):
    return got["metered"] == want["metered"] and got["skipped"] == want["skipped"] and \
        all(bits(got[k]) == bits(want[k]) for k in ("exposure", "target", "average_luminance"))


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("total", TOTALS)
def test_header_arithmetic_matches_numpy_bit_for_bit(host, h, w, total):
    sums, special = exposure_ref.synthetic(h, w, seed=1000 * h + w)
    got, want = host.histogram(sums, total), exposure_ref.histogram(sums, total)
    assert np.array_equal(got, want) and int(got.astype(np.int64).sum()) == h * w
    for kw in PARAM_SETS:
        g, r = host.result(got, **kw), exposure_ref.from_histogram(want, **kw)
        assert same_result(g, r), (kw, g, r)
        assert g["metered"] + g["skipped"] == h * w
        if g["metered"]:
            q = dict(exposure_ref.DEFAULTS, **kw)
            assert F(q["min_exposure"]) <= g["target"] <= F(q["max_exposure"]) and g["exposure"] > 0
    word = exposure_ref.words(exposure_ref.luminance(sums, total)).ravel()
    if special:
        for k in ("zero", "negative", "nan"):
            assert word[special[k]] == 256, k
        assert word[special["negative_channel"]] < 256  # (-0.5, 2, 0.25): a positive luminance counts
        assert word[special["tiny"]] == 0 and word[special["inf"]] == 255 and word[special["huge"]] == 255
        assert got[256] == 3 and got[0] >= 1 and got[255] == 2
        # a clamp that bites: the target is the bound itself
        assert host.result(got, min_exposure=4.0, max_exposure=8.0)["target"] == 4.0
        assert host.result(got, min_exposure=2.0 ** -10, max_exposure=2.0 ** -9)["target"] == F(2.0 ** -9)
    # the blends, said in words: 0 keeps the previous exposure, 1 lands within an ulp of the target
    t = host.result(got)["target"]
    assert host.result(got, blend=0.0, previous_exposure=0.7)["exposure"] == F(0.7)
    assert abs(float(host.result(got, blend=1.0, previous_exposure=0.7)["exposure"]) - float(t)) <= 2 * float(np.spacing(max(t, F(0.7))))


def in_f16_range(h, w, seed):
    """Sums whose means, times 4 and times 1 / 8 too, stay inside binary16's normal range for totals 1 and 3."""
    rng = np.random.default_rng(seed)
    s = np.ones((h, w, 4), F)
    s[..., :3] = np.exp2(rng.uniform(-8, 10, (h, w, 3))).astype(F)
    return s


@pytest.mark.parametrize("total", TOTALS)
def test_power_of_two_invariance(host, total):
    base = in_f16_range(37, 70, 5)
    h0 = host.histogram(base, total)
    r0 = host.result(h0)
    d0 = host.display(base, total, float(r0["exposure"]))
    assert h0[256] == 0 and np.array_equal(h0, exposure_ref.histogram(base, total))
    for scale, shift in ((4.0, 16), (0.125, -24)):
        hs = host.histogram(base * F(scale), total)
        assert np.array_equal(hs[:256], np.roll(h0[:256], shift)) and hs[256] == 0  # (nothing near the ends: the roll moves zeros around)
        assert not h0[:24].any() and not h0[-16:].any()
        rs = host.result(hs)
        assert bits(rs["average_luminance"]) == bits(r0["average_luminance"] * F(scale))
        assert bits(rs["exposure"]) == bits(r0["exposure"] / F(scale)) and bits(rs["target"]) == bits(rs["exposure"])
        assert np.array_equal(host.display(base * F(scale), total, float(rs["exposure"])), d0)
    assert len(np.unique(d0[..., :3])) > 50  # (a picture, not a clipped or black frame)


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("total", TOTALS)
def test_exposure_one_is_the_plain_display(host, h, w, total):
    sums, _ = exposure_ref.synthetic(h, w, seed=1000 * h + w)
    plain = host.display(sums, total)
    assert np.array_equal(host.display(sums, total, 1.0), plain)
    assert np.array_equal(exposure_ref.display(sums, total, 1.0), plain)
    import test_display
    assert np.array_equal(test_display.display_numpy(sums, total), plain)
    for e in (0.37, 4.0):
        assert np.array_equal(host.display(sums, total, e), exposure_ref.display(sums, total, e)), e


def test_degenerate_histograms(host):
    # every pixel skipped: the N == 0 rule
    none = np.zeros((3, 5, 4), F)
    none[0, 0, :3] = np.nan
    none[0, 1, :3] = -1
    h = host.histogram(none, 1)
    assert h[256] == 15 and not h[:256].any()
    for prev, want in ((0.0, 1.0), (0.37, 0.37)):
        for blend in (0.0, 0.5, 1.0):
            r = host.result(h, previous_exposure=prev, blend=blend)
            assert same_result(r, exposure_ref.from_histogram(h, previous_exposure=prev, blend=blend))
            assert r["metered"] == 0 and r["skipped"] == 15 and r["average_luminance"] == 0 and r["exposure"] == r["target"] == F(want)
    # one pixel, at every trim: that pixel's bin centre
    one = np.ones((1, 1, 4), F)
    one[0, 0, :3] = 0.5  # L = 0.5 up to rounding: bin of 2^-1 (or the last of the octave below)
    h = host.histogram(one, 1)
    b = int(np.flatnonzero(h)[0])
    assert h.sum() == 1 and b in ((126 << 3) - exposure_ref.LO, (126 << 3) - exposure_ref.LO - 1)
    for kw in PARAM_SETS[:3]:
        r = host.result(h, **kw)
        assert same_result(r, exposure_ref.from_histogram(h, **kw))
        assert bits(r["average_luminance"]) == ((exposure_ref.LO + b) << 20) + (1 << 19)
    # all pixels in one bin: average_luminance is that bin's centre, whatever the trim
    for b in (0, 100, 255):
        h = np.zeros(257, np.uint32)
        h[b], h[256] = 12345, 17
        for kw in PARAM_SETS[:3]:
            r = host.result(h, **kw)
            assert same_result(r, exposure_ref.from_histogram(h, **kw))
            assert bits(r["average_luminance"]) == ((exposure_ref.LO + b) << 20) + (1 << 19) and r["metered"] == 12345 and r["skipped"] == 17
    # two bins, the trim cutting between them: ranks [a, b) weigh the bins
    h = np.zeros(257, np.uint32)
    h[10], h[20] = 100, 100
    r = host.result(h, low_permille=250, high_permille=750)  # ranks [50, 150): half and half -> bin 15.0
    assert bits(r["average_luminance"]) == ((exposure_ref.LO + 15) << 20) + (1 << 19)
    r = host.result(h, low_permille=0, high_permille=500)  # ranks [0, 100): bin 10 alone
    assert bits(r["average_luminance"]) == ((exposure_ref.LO + 10) << 20) + (1 << 19)
    # the largest frame the contract names: 16384 x 16384 pixels in the top bin does not overflow
    h = np.zeros(257, np.uint32)
    h[255] = 16384 * 16384
    assert same_result(host.result(h, low_permille=0, high_permille=1000), exposure_ref.from_histogram(h, low_permille=0, high_permille=1000))


def test_params_ok_refuses_each_bad_field(host):
    assert host.ok() and exposure_ref.params_ok(**exposure_ref.DEFAULTS)
    good = [{"low_permille": 0, "high_permille": 1}, {"high_permille": 1000}, {"blend": 0.0}, {"previous_exposure": 3.0},
            {"min_exposure": 2.0, "max_exposure": 2.0}]
    bad = [{"low_permille": 950}, {"low_permille": 951}, {"high_permille": 1001}, {"low_permille": 0, "high_permille": 0}]
    for name in ("key", "min_exposure", "max_exposure"):
        bad += [{name: v} for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad += [{"min_exposure": 2.0, "max_exposure": 1.0}]
    bad += [{"blend": v} for v in (-0.01, 1.01, float("nan"), float("inf"))]
    bad += [{"previous_exposure": v} for v in (-1.0, float("nan"), float("inf"))]
    for kw in good:
        assert host.ok(**kw) and exposure_ref.params_ok(**dict(exposure_ref.DEFAULTS, **kw)), kw
    for kw in bad:
        assert not host.ok(**kw) and not exposure_ref.params_ok(**dict(exposure_ref.DEFAULTS, **kw)), kw


def test_struct_layouts_and_defaults(host):
    lay = np.zeros(11, np.uint32)
    host.L.exposure_layout(lay.ctypes.data)
    P, Rs = state.ExposureParams, state.ExposureResult
    assert list(lay) == [C.sizeof(P), P.high_permille.offset, P.key.offset, P.blend.offset, P.previous_exposure.offset, P.flags.offset,
                         C.sizeof(Rs), Rs.target.offset, Rs.average_luminance.offset, Rs.metered.offset, Rs.skipped.offset]
    assert C.sizeof(P) == 32 and C.sizeof(Rs) == 24
    assert [f[0] for f in P._fields_] == ["low_permille", "high_permille", "key", "min_exposure", "max_exposure", "blend", "previous_exposure", "flags"]
    assert [f[0] for f in Rs._fields_] == ["exposure", "target", "average_luminance", "metered", "skipped", "_pad"]
    d = state.ExposureParams()
    host.L.exposure_defaults(C.byref(d))
    got = {k: getattr(d, k) for k in exposure_ref.DEFAULTS}
    assert d.flags == 0 and got == {k: (v if isinstance(v, int) else float(F(v))) for k, v in exposure_ref.DEFAULTS.items()}
    assert state.EXPOSURE_DEFAULTS == exposure_ref.DEFAULTS and state.EXPOSURE_WORDS == exposure_ref.WORDS == 257
    assert state.EXPOSURE_SOURCES == {"mean": 0, "denoised": 1, "temporal": 2, "upsampled": 3}
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_EXPOSURE_MEAN = 0" in hdr and "RSRT_EXPOSURE_DENOISED = 1" in hdr and "RSRT_EXPOSURE_TEMPORAL = 2" in hdr and "RSRT_EXPOSURE_UPSAMPLED = 3" in hdr
    ex = open(os.path.join(util.ROOT, "include", "rsrt_exposure.h")).read()
    assert "#define RSRT_EXPOSURE_LO 888u" in ex and exposure_ref.LO == 888 and bits(F(2.0 ** -16)) >> 20 == 888
    import inspect
    sig = inspect.signature(R.State.render_to_noise).parameters
    assert sig["exposure"].default is None
    sig = inspect.signature(R.State.auto_exposure).parameters
    assert (sig["source"].default, sig["blend"].default) == ("mean", 1.0)


def test_library_exports_auto_exposure():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_exposure_meter", "rsrt_exposure_download", "rsrt_exposure_reset", "rsrt_display_exposed_srgb8"):
        assert hasattr(lib, n), n
    for m in ("exposure_meter", "exposure_download", "auto_exposure", "exposure_reset", "display_exposed_srgb8"):
        assert hasattr(R.State, m), m


def test_exposure_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in ("rt_exposure_hist_kernel", "rt_display_exposed_kernel"):
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "exposure_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "exposure_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_auto_exposure_compiles(tmp_path):
    build_cpp_demo(tmp_path)


@pytest.mark.parametrize("name,w,h", [("house", 96, 54), ("suzanne", 80, 48)])
def test_meter_reads_the_true_log_average_of_rendered_frames(host, name, w, h):
    """The metered average_luminance against the geometric mean, in float64, of the luminances the trim keeps (ranks [a, b) of the
    metered pixels sorted by luminance): within a quarter octave.  The bound is derived, not fitted: the piecewise-linear logarithm
    reads at most 0.086 octave low, the bin centres are at most 1 / 16 octave from a pixel, and the rest (0.1 octave) is for rank ties
    at the trim's edges, where the histogram cuts a bin in proportion and the sort cuts it by value.  Measured (average / true):
    house 96x54 49.6596 / 48.5785 = 1.0223 (+0.0318 octave), suzanne 80x48 56.3934 / 56.5132 = 0.9979 (-0.0031 octave)."""
    import test_noise
    sums, _ = test_noise.checker_frames(name, w, h)
    acc = sums[64]
    hist = host.histogram(acc, 64)
    assert np.array_equal(hist, exposure_ref.histogram(acc, 64)) and int(hist.sum()) == w * h
    r = host.result(hist)
    assert same_result(r, exposure_ref.from_histogram(hist))
    c = acc[..., :3].astype(np.float64) / 64.0
    lum = (0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]).ravel()
    lum = np.sort(lum[lum > 0])
    n = lum.size
    assert n == r["metered"] and n > 0.9 * w * h
    a, b = n * 100 // 1000, (n * 950 + 999) // 1000
    true = 2.0 ** np.mean(np.log2(lum[a:b]))
    octaves = float(np.log2(float(r["average_luminance"]) / true))
    print("%s %dx%d: average_luminance %.6f, true log-average %.6f, ratio %.4f (%+.4f octave), exposure %.4f"
          % (name, w, h, r["average_luminance"], true, float(r["average_luminance"]) / true, octaves, r["exposure"]))
    assert abs(octaves) <= 0.25
