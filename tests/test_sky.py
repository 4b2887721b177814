"""The procedural daylight sky without a GPU: its published arithmetic (include/rsrt_sky.h), as librsrt_host.so's rsrt_sky_fill runs it
(shares once a row and a column) and as tests/cpp/sky_host.cpp does (everything per texel), against the numpy restatement the GPU
tests hold the kernel to (tests/sky_ref.py), bit for bit; the constants of a parameter set; rsrt_sky_exp2 against float64; that
every output is finite and >= 0, the zenith blue, the sun where it was put and its disc worth the illuminance asked for; the
parameter check; the layout and the defaults; Environment.sky; the ABI and the kernels' code objects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sky_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, host as H, state

F = np.float32
SIZES = sky_ref.SIZES + [(1, 1)]


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def c_params(**kw):
    """SkyParams of the defaults with kw over them, without SkyParams.of's checks (refused values included)."""
    return state.SkyParams.of(**dict(sky_ref.DEFAULTS, **kw))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sky") / "libsky.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "sky_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.sky_fill.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sky_prepare.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.sky_exp2.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.sky_params_ok.argtypes = [C.c_void_p]
    L.sky_defaults.argtypes = [C.c_void_p]
    L.sky_layout.argtypes = [C.c_void_p]
    L.sky_limits.argtypes = [C.c_void_p]

    class Host:
        @staticmethod
        def fill(w, h, **kw):
            p, out = c_params(**kw), np.full((h, w, 4), 7, F)
            assert L.sky_fill(h, w, C.byref(p), out.ctypes.data) == 0
            return out

        @staticmethod
        def prepare(h, **kw):
            p, out = c_params(**kw), np.full(33, 7, F)
            L.sky_prepare(C.byref(p), h, out.ctypes.data)
            return out

        @staticmethod
        def exp2(t):
            t = np.ascontiguousarray(t, F)
            out = np.full(t.shape, 7, F)
            L.sky_exp2(t.ctypes.data, t.size, out.ctypes.data)
            return out

        @staticmethod
        def ok(**kw):
            p = c_params(**kw)
            return bool(L.sky_params_ok(C.byref(p)))
    Host.L = L
    return Host


# ---------------------------------------------------------------------------------------------------- a: bit parity
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("case", sorted(sky_ref.CASES))
def test_fill_matches_numpy_bit_for_bit(host, case, w, h):
    kw = sky_ref.CASES[case]
    want = sky_ref.reference(case, w, h)
    assert np.isfinite(want).all() and (want >= 0).all() and not want[..., 3].any()
    assert same(H.sky_fill(w, h, **kw), want), "librsrt_host.so: shares once a row and a column"
    assert same(host.fill(w, h, **kw), want), "the header, everything per texel"
    if case == "sun_at_zenith":  # g = 0 exactly where the map has a texel on the sun; F(0, 0) in the constants
        assert sky_ref.prepare(sky_ref.params(**kw), h)["sun_dir"][1] == 1
    if (w, h) == (37, 19):  # the middle row is the shader's almost-horizon: cos theta tiny and positive, clamped up to 2^-10
        ct = sky_ref.rows(sky_ref.prepare(sky_ref.params(**kw), h), h)[1][9]
        assert 0 < ct < sky_ref.MIN_COS


@pytest.mark.parametrize("case", sorted(sky_ref.CASES))
def test_prepared_constants_match_numpy_field_by_field(host, case):
    for _, h in SIZES + [(2048, 1024)]:
        got = host.prepare(h, **sky_ref.CASES[case])
        k = sky_ref.prepare(sky_ref.params(**sky_ref.CASES[case]), h)
        at = 0
        for name, n in sky_ref.CONSTANTS:
            assert same(got[at:at + n], np.atleast_1d(np.asarray(k[name], F))), (name, h)
            at += n
        assert at == 33
    # the widened radius: 1.5 texels on a coarse map, the given one on a fine one
    assert sky_ref.prepare(sky_ref.params(), 32)["r_eff"] == F(F(F(1.5) * sky_ref.PIF) / F(32))
    assert sky_ref.prepare(sky_ref.params(), 1024)["r_eff"] == F(0.00465)


def test_exp2_against_float64(host):
    """Within 2^-17 of 2^t relatively over the range the sky uses (t <= 0) and a little beyond — the bound include/rsrt_sky.h states and
    derives: the polynomial's own published 2^-18.2 plus its five roundings.  Measured: 3.4e-6 (2^-18.2)."""
    k = np.arange(-126 * 1024, 2 * 1024 + 1)
    ints = np.arange(-126, 3).astype(F)
    t = np.concatenate([(k / 1024.0).astype(F), np.nextafter(ints, F(-200)), np.nextafter(ints, F(200))])
    t = t[t >= -126]
    got = host.exp2(t)
    assert same(got, sky_ref.exp2(t))
    err = np.abs(got.astype(np.float64) / np.exp2(t.astype(np.float64)) - 1.0).max()
    print("rsrt_sky_exp2: largest relative error %.3g (2^%.2f)" % (err, np.log2(err)))
    assert err <= 2.0 ** -17
    # exact at the integers, 1 at 0
    assert same(host.exp2(ints), np.exp2(ints.astype(np.float64)).astype(F)) and host.exp2(F(0))[()] == 1
    # the clamps: exactly 0 below -126 (and for NaN), the smallest normal at -126, 2^126 from 126 up; never subnormal, never inf
    edge = np.array([-126, np.nextafter(F(-126), F(-200)), -127, -1000, -3.0e38, -np.inf, np.nan, 126, 126.5, 1000, 3.0e38, np.inf], F)
    with np.errstate(invalid="ignore"):
        got = host.exp2(edge)
    assert same(got, np.array([2.0 ** -126] + [0] * 6 + [2.0 ** 126] * 5, F))
    # monotone non-decreasing, over a fine sweep through the clamps and across every octave's join
    s = np.sort(np.concatenate([np.linspace(-130, 130, 200001).astype(F), t]))
    v = host.exp2(s)
    assert (np.diff(v) >= 0).all() and (v[s >= -126] >= F(2.0 ** -126)).all()


# ---------------------------------------------------------------------------------------------------- b: properties at 256 x 128
W, HH = 256, 128


def test_every_value_is_finite_and_not_negative():
    el = [float(sky_ref.MIN_ELEVATION), 0.3, 0.9, float(sky_ref.MAX_ELEVATION)]
    for e in el:
        for T in (2.0, 3.5, 6.0, 10.0):
            for az in (0.0, -2.5):
                a = H.sky_fill(W, HH, sun_elevation=e, turbidity=T, sun_azimuth=az, sun_radius=0.1 if T == 6.0 else 0.00465)
                assert np.isfinite(a).all() and (a >= 0).all() and not a[..., 3].any(), (e, T, az)
                assert a[..., :3].max() > 0
    # amounts near the largest float saturate instead of reaching inf or inf * 0
    big = 3.0e38
    for kw in ({"ground_albedo": (big, 1.0, 0.0), "scale": 0.0, "sun_illuminance": big}, {"scale": big, "sun_illuminance": big, "ground_albedo": (big,) * 3},
               {"sun_azimuth": big}):  # (an azimuth beyond rsrt_sinf's range: see include/rsrt_sky.h)
        a = H.sky_fill(64, 32, **kw)
        assert np.isfinite(a).all() and (a >= 0).all(), kw


def test_a_clear_zenith_is_blue():
    a = H.sky_fill(W, HH, turbidity=2.0, sun_elevation=float(np.deg2rad(60.0)))
    top = a[0].mean(axis=0)
    assert top[2] > top[0] and top[2] > top[1], top
    assert (a[0, :, 2] > a[0, :, 0]).all()


@pytest.mark.parametrize("case", ["defaults", "turned", "sun_at_1_degree", "sun_at_zenith"])
def test_the_brightest_texel_is_at_the_sun(case):
    p = sky_ref.params(**sky_ref.CASES[case])
    a = sky_ref.reference(case, W, HH)
    lum = a[..., :3].astype(np.float64) @ [0.2126, 0.7152, 0.0722]
    y, x = np.unravel_index(np.argmax(lum), lum.shape)
    d = sky_ref.directions(W, HH)[y, x].astype(np.float64)
    el, az = p["sun_elevation"], p["sun_azimuth"]
    s = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    angle = np.arctan2(np.linalg.norm(np.cross(d, s)), d @ s)
    assert angle <= np.pi / HH * np.sqrt(2.0), (case, x, y, angle)  # within one texel (its diagonal) of the sun's direction


@pytest.mark.parametrize("w,h", [(64, 32), (256, 128)])
def test_the_disc_carries_the_attenuated_illuminance(w, h):
    """The sum over texels of the sun term x the texel's solid angle / scale against E e^(-tau m), per channel.  The margin is what
    the same sum gives in float64 (sky_ref.disc_illuminance_f64): what the one-texel ramp and the grid make of a disc widened to 1.5
    texels.  Measured in float64: 1.0418 at 64 x 32, 1.0450 at 256 x 128 — the ramp does not lose, it adds: a linear ramp one texel
    wide around a radius of R texels integrates to the area of a disc of radius sqrt(R^2 + 1/12), 1 + 1/27 = 1.037 at R = 1.5; the rest
    is the grid.  The f32 evaluation must then agree with the float64 one to 1e-4: exp2's 3.4e-6, atan2's 3 ulp of an angle of a few
    hundredths times H / pi texels a radian, and the rounding of a sum of some twenty texels, each far below it."""
    p = sky_ref.params()
    with_disc = H.sky_fill(w, h, **sky_ref.CASES["defaults"]).astype(np.float64)
    without = H.sky_fill(w, h, sun_illuminance=0.0).astype(np.float64)
    sun = (with_disc - without)[..., :3]
    assert (sun >= 0).all() and 4 <= (sun[..., 0] > 0).sum() <= 40
    got = (sun * sky_ref.solid_angles(w, h)[:, None, None]).sum(axis=(0, 1)) / p["scale"]
    T, cs = p["turbidity"], np.sin(p["sun_elevation"])
    m = 1.0 / (cs + 0.025 * np.exp(-11.0 * cs))
    tau = sky_ref.TAU_R.astype(np.float64) + (0.04608 * T - 0.04586) * sky_ref.LAMBDA.astype(np.float64)
    want = p["sun_illuminance"] * np.exp(-tau * m)
    ratio = got / want
    exact = sky_ref.disc_illuminance_f64(w, h, p)
    print("disc illuminance / attenuated illuminance at %dx%d: f32 %s, float64 %.6f" % (w, h, ratio, exact))
    margin = abs(exact - 1.0)
    assert margin <= 0.05  # measured 0.0418 (64 x 32), 0.0450 (256 x 128)
    assert (np.abs(ratio - 1.0) <= margin + 1e-4).all() and (np.abs(ratio - exact) <= 1e-4).all(), (ratio, exact)
    assert want[0] > want[1] > want[2]  # the low sun is red: blue is attenuated most


# ---------------------------------------------------------------------------------------------------- c: the parameter check
@pytest.mark.parametrize("name", sorted(sky_ref.REFUSED))
def test_every_refusal(host, name):
    kw = sky_ref.REFUSED[name]
    assert not host.ok(**kw) and not sky_ref.params_ok(dict(sky_ref.DEFAULTS, **kw))
    with pytest.raises(ValueError, match="rsrt_sky_fill refused"):
        H.sky_fill(8, 4, **kw)
    with pytest.raises(ValueError, match="rsrt_sky_fill refused"):
        R.Environment.sky(8, 4, **kw)


def test_boundary_values_are_accepted_and_a_refused_fill_writes_nothing(host):
    assert host.ok() and all(host.ok(**kw) for kw in sky_ref.CASES.values())
    one_degree, ninety = float(F(np.deg2rad(1.0))), float(F(np.pi / 2))
    assert F(one_degree) == sky_ref.MIN_ELEVATION and F(ninety) == sky_ref.MAX_ELEVATION
    for kw in ({"sun_elevation": one_degree}, {"sun_elevation": ninety}, {"turbidity": 2.0}, {"turbidity": 10.0}, {"sun_radius": 0.0}, {"sun_radius": float(F(0.1))},
               {"scale": 0.0}, {"sun_illuminance": 0.0}, {"sun_azimuth": -7.0}):
        assert host.ok(**kw) and sky_ref.params_ok(sky_ref.params(**kw)), kw
        a = H.sky_fill(8, 4, **kw)
        assert np.isfinite(a).all() and (a >= 0).all(), kw
    L = H.lib()
    out = np.full((4, 8, 4), 7, F)
    p = c_params(turbidity=11.0)
    assert L.rsrt_sky_fill(8, 4, C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0 and (out == 7).all()
    p = c_params()
    assert L.rsrt_sky_fill(0, 4, C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0 and L.rsrt_sky_fill(8, 0, C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0
    assert L.rsrt_sky_fill(8, 4, None, out.ctypes.data_as(C.c_void_p)) != 0 and L.rsrt_sky_fill(8, 4, C.byref(p), None) != 0 and (out == 7).all()
    with pytest.raises(TypeError, match="unknown sky parameter"):
        H.sky_fill(8, 4, sun_height=1.0)


# ---------------------------------------------------------------------------------------------------- d: layout, defaults, the interface
def test_layout_and_defaults_agree_with_the_header(host):
    lay = np.zeros(9, np.uint32)
    host.L.sky_layout(lay.ctypes.data)
    P = state.SkyParams
    assert list(lay[:8]) == [C.sizeof(P)] + [getattr(P, n).offset for n in ("sun_elevation", "turbidity", "ground_albedo", "scale", "sun_illuminance",
                                                                              "sun_radius", "flags")]
    assert C.sizeof(P) == 40 and P.sun_azimuth.offset == 0 and lay[8] == 33 * 4
    assert [n for n, _ in P._fields_] == list(sky_ref.FIELDS)
    d = P()
    host.L.sky_defaults(C.byref(d))
    want = P.of()
    assert bytes(d) == bytes(want)
    assert set(state.SKY_DEFAULTS) == set(sky_ref.FIELDS)
    for n in sky_ref.FIELDS:
        a, b = state.SKY_DEFAULTS[n], sky_ref.DEFAULTS[n]
        assert same(np.asarray(a, F), np.asarray(b, F)), n
    assert d.sun_illuminance == 128 and d.scale == 1 / 64 and d.sun_radius == F(0.00465) and d.flags == 0
    lim = np.zeros(5, F)
    host.L.sky_limits(lim.ctypes.data)
    assert same(lim, np.array([np.deg2rad(1.0), np.pi / 2, 2, 10, 0.1], F))


def test_environment_sky_builds_the_host_alias_table():
    env = R.Environment.sky(64, 32, sun_azimuth=2.1, sun_elevation=0.6)
    assert (env.width, env.height) == (64, 32) and same(env.rgba, H.sky_fill(64, 32, sun_azimuth=2.1, sun_elevation=0.6))
    want, left = R.AliasTable.build_by_luminance(env.rgba[:, :, :3])
    assert util.fields_equal(env.alias, want) and env.leftover == left
    assert abs(float(env.alias["pmf"].astype(np.float64).sum()) - 1.0) < 1e-3
    big = R.Environment.sky()  # the default size
    assert (big.width, big.height) == (2048, 1024) and np.isfinite(big.rgba).all() and big.rgba.max() < 65504  # under the binary16 range
    assert big.rgba.max() > 2.0e4  # the disc: about 1.9e6 kcd/m^2 attenuated over an air mass of 1.4, / 64


def test_abi_and_the_kernels_code_objects():
    assert "rsrt_environment_sky" in state._SYMBOLS and "rsrt_environment_download" in state._SYMBOLS
    lib = C.CDLL(_build.build_hip())
    assert hasattr(lib, "rsrt_environment_sky") and hasattr(lib, "rsrt_environment_download")
    assert hasattr(C.CDLL(_build.build_host()), "rsrt_sky_fill")
    import test_code_object
    if not os.path.exists(os.path.join(test_code_object.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    md = {n: m for n, m in test_code_object.kernel_metadata().items() if "rt_sky_" in n}
    assert sorted(n.split("kernel")[0] for n in md) == ["_Z18rt_sky_fill_", "_Z20rt_sky_shares_"]
    for n, m in md.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["vgpr_count"] <= 64, (n, m)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "sky_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "sky_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_sky_compiles(tmp_path):
    build_cpp_demo(tmp_path)
