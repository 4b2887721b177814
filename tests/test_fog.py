"""Volumetric fog without a GPU: its published arithmetic (include/rsrt_fog.h), compiled for the CPU, against the numpy restatement the
GPU tests hold the kernels to (tests/fog_ref.py), bit for bit, edge inputs included; the parameter check; the ABI; the restatement end
to end against a float64 closed form; the sun of a sky as the light; the kernels' code objects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fog_ref
import sky_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

F = np.float32
same = util.same_bits_or_nan
LIGHT = fog_ref.unit((0.4, 0.6, -0.7))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def c_params(p):
    return state.FogParams.of(**p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fog") / "libfog.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "fog_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    V, Z, U = C.c_void_p, C.c_size_t, C.c_uint32
    L.fog_prepare.argtypes = [V, V, V]
    L.fog_light_term.argtypes = [V, V, Z, V, V, V]
    L.fog_phase.argtypes = [V, V, Z, V]
    L.fog_march_point.argtypes = [V, V, V, V, V, V, U, Z, V, V, V, V, V, V]
    L.fog_sample.argtypes = [V, V, V, V, V, V, Z, V]
    L.fog_compose.argtypes = [V, V, C.c_float, Z, V]
    L.fog_light_from_sky.argtypes = [V, U, V, V]
    L.fog_params_ok.argtypes = [V]
    L.fog_defaults.argtypes = [V]
    L.fog_layout.argtypes = [V]
    return L


def random_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.sqrt((v * v).sum(axis=1, keepdims=True))).astype(F)


PARAM_SETS = [
    {},
    {"anisotropy": 0.0, "ambient": (0.1, 0.2, 0.3)},
    {"anisotropy": 0.95, "density": 0.3, "albedo": (0.9, 0.5, 0.0), "light_irradiance": (3.0, 2.5, 2.0), "steps": 1},
    {"anisotropy": -0.95, "density": 2.5, "max_distance": 7.0, "steps": 64, "ambient": 0.05},
    {"density": 0.0, "ambient": 1.0, "steps": 5},
    {"density": 1.0e6, "max_distance": 1.0e30, "steps": 3},
    {"density": 1.0e-30, "light_irradiance": 1.0e30, "steps": 9, "flags": 0},
]


def param_set(kw):
    return fog_ref.params(**dict({"light_dir": LIGHT}, **kw))


@pytest.mark.parametrize("kw", PARAM_SETS)
def test_header_arithmetic_matches_numpy_bit_for_bit(host, kw):
    p = param_set(kw)
    assert fog_ref.params_ok(p)
    cp, k = c_params(p), fog_ref.prepare(p)
    got, words = np.full(17, 7, F), np.zeros(2, np.uint32)
    host.fog_prepare(C.byref(cp), ptr(got), ptr(words))
    assert same(got, fog_ref.constants_vector(k)) and words.tolist() == [p["steps"], p["flags"]]

    rng = np.random.default_rng(len(str(kw)))
    n = 3000
    light = np.asarray(LIGHT, F)
    d = random_dirs(rng, n)
    d[0], d[1] = light, -light  # cos theta = +-1 (to rounding)
    d[2] = (1, 0, 0)
    cos, ph, s_sun = np.full(n, 7, F), np.full(n, 7, F), np.full((n, 3), 7, F)
    host.fog_light_term(C.byref(cp), ptr(d), n, ptr(cos), ptr(ph), ptr(s_sun))
    want_cos = fog_ref.cos_theta(k, d)
    assert same(cos, want_cos) and same(ph, fog_ref.phase(k, want_cos)) and same(s_sun, fog_ref.sun(k, ph))
    assert np.isfinite(ph).all() and (ph > 0).all() and np.isfinite(s_sun).all()
    exact = np.array([1.0, -1.0, 0.0, 0.5, -0.25], F)  # the phase function at exact cosines
    ph_exact = np.full(exact.size, 7, F)
    host.fog_phase(C.byref(cp), ptr(exact), exact.size, ptr(ph_exact))
    assert same(ph_exact, fog_ref.phase(k, exact))
    g = float(F(p["anisotropy"]))
    want64 = (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * exact.astype(np.float64)) ** 1.5)
    assert np.allclose(ph_exact, want64, rtol=3e-4 if abs(g) > 0.9 else 2e-6)  # (q = 1 + g^2 - 2 g cancels to 0.0025 at |g| = 0.95)

    # the march: hits before, at and beyond max_distance, misses, xi at both ends, every step
    o = rng.normal(size=(n, 3)).astype(F)
    hit = (rng.random(n) < 0.7).astype(np.int32)
    dist = F(p["max_distance"])
    t_hit = (rng.random(n) * 1.5 * float(dist)).astype(F)
    t_hit[:4] = (0.0, dist, np.nextafter(dist, F(0)), np.nextafter(dist, F(np.inf)))
    hit[:4] = 1
    xi = rng.random(n).astype(F)
    xi[:6] = (0, 1, 0, 1, 0.5, 0.5)
    L = fog_ref.segment(k, hit != 0, t_hit)
    assert L[1] == dist and L[3] == dist and L[2] < dist and (L[hit == 0] == dist).all() and (L <= dist).all()
    dl = fog_ref.delta(k, L)
    for step in sorted({0, p["steps"] // 2, p["steps"] - 1}):
        outs = [np.full(n, 7, F) for _ in range(3)] + [np.full((n, 3), 7, F)] + [np.full(n, 7, F) for _ in range(2)]
        host.fog_march_point(C.byref(cp), ptr(o), ptr(d), ptr(hit), ptr(t_hit), ptr(xi), step, n, *[ptr(a) for a in outs])
        t = fog_ref.t_of(step, xi, dl)
        want = [L, dl, t, fog_ref.point(o, d, t), fog_ref.transmittance(k, t), fog_ref.transmittance(k, L)]
        assert all(same(a, b) for a, b in zip(outs, want)), step
        assert ((outs[4] >= 0) & (outs[4] <= 1)).all()
    if p["density"] == 0:
        assert (outs[4] == 1).all() and (outs[5] == 1).all()

    # the per-sample sum over two samples, and compose
    rec = np.zeros((n, 4), F)
    want_rec = rec.copy()
    for s in range(2):
        lit = rng.random((n, p["steps"])) < 0.6
        lit[:8], lit[8:16] = True, False
        lit8 = np.ascontiguousarray(lit, np.uint8)
        host.fog_sample(C.byref(cp), ptr(d), ptr(hit), ptr(t_hit), ptr(xi), ptr(lit8), n, ptr(rec))
        want_rec = fog_ref.sample(k, d, hit != 0, t_hit, xi, lit, want_rec)
        assert same(rec, want_rec), s
    colour = (rng.random((n, 3)) * 4).astype(F)
    colour[0] = (-0.0, 0.0, 1.0)
    out = np.full((n, 4), 7, F)
    host.fog_compose(ptr(colour), ptr(rec), 2.0, n, ptr(out))
    assert same(out, fog_ref.compose(colour, rec, 2)) and (out[:, 3] == 1).all()
    if p["density"] == 0:  # a clear medium: the source itself, a negative zero included
        assert (rec[:, :3] == 0).all() and (rec[:, 3] == 2).all() and np.array_equal(util.bits(out[:, :3]), util.bits(colour))


def test_params_ok_accepts_and_rejects(host):
    nan, inf = float("nan"), float("inf")
    good = [{}, {"density": 0.0}, {"density": 1.0e6}, {"albedo": 0.0}, {"albedo": (0.0, 0.5, 1.0)}, {"anisotropy": 0.95}, {"anisotropy": -0.95}, {"anisotropy": 0.0},
            {"light_dir": (1.0, 0.0, 0.0)}, {"light_dir": (1.0004, 0.0, 0.0)}, {"light_dir": (0.0, -0.9996, 0.0)}, {"light_irradiance": 0.0},
            {"light_irradiance": 3.0e38}, {"ambient": 3.0e38}, {"max_distance": 1.0e-30}, {"max_distance": 3.0e38}, {"steps": 1}, {"steps": 64}, {"flags": 0},
            {"flags": 1}, {"density": 1.0e6, "max_distance": 1.0e30}]
    largest = float(fog_ref.LARGEST)
    # one sample's sum and inscatter must stay finite (rsrt_fog.h "Finiteness"): the nearest accepted neighbours of the sets refused below
    good += [{"density": 1.0e6, "light_irradiance": 2.6e31}, {"density": 1.0e6, "ambient": 2.1e31}, {"density": 1.0, "anisotropy": 0.95, "light_irradiance": 3.9e34},
             {"density": 0.0768, "light_irradiance": largest}, {"density": 0.0197, "ambient": largest}, {"density": 0.0, "light_irradiance": largest, "ambient": largest},
             {"albedo": 0.0, "density": 1.0e6, "light_irradiance": largest, "ambient": largest}, {"ambient": 3.0e38, "steps": 16}]
    bad = [{"density": v} for v in (-1e-30, -1.0, 1.0001e6, nan, inf, -inf)]
    bad += [{"albedo": v} for v in (-0.001, 1.001, nan, inf, (0.5, 0.5, 1.5), (nan, 0.5, 0.5), (0.5, -1.0, 0.5))]
    bad += [{"anisotropy": v} for v in (0.951, -0.951, 1.0, nan, inf)]
    bad += [{"light_dir": v} for v in ((0.0, 0.0, 0.0), (1.002, 0.0, 0.0), (0.0, 0.998, 0.0), (1.0, 1.0, 0.0), (nan, 0.0, 1.0), (inf, 0.0, 0.0))]
    bad += [{"light_irradiance": v} for v in (-1.0, nan, inf, (1.0, 1.0, -1e-30), (1.0, inf, 1.0))]
    bad += [{"ambient": v} for v in (-1.0, nan, inf, (-1e-30, 0.0, 0.0), (0.0, 0.0, nan))]
    bad += [{"max_distance": v} for v in (0.0, -0.0, -1.0, nan, inf)]
    bad += [{"steps": v} for v in (0, 65, 0xffffffff)]
    bad += [{"flags": v} for v in (2, 3, 0x80000000, 0x80000001)]
    bad += [{"density": 1.0e6, "max_distance": 3.0e38}, {"density": 2.0, "max_distance": 3.0e38}]  # density * max_distance must stay finite
    bad += [{"density": 1.0e6, "light_irradiance": largest}, {"density": 1.0e6, "ambient": largest}, {"density": 1.0, "anisotropy": 0.95, "light_irradiance": largest},
            {"density": 1.0e6, "light_irradiance": 2.7e31}, {"density": 1.0e6, "ambient": 2.2e31}, {"density": 1.0, "anisotropy": 0.95, "light_irradiance": 4.0e34},
            {"density": 0.077, "light_irradiance": largest}, {"density": 0.0199, "ambient": largest}, {"ambient": 3.0e38, "steps": 1}]
    for kw in good:
        p = fog_ref.params(**kw)
        assert host.fog_params_ok(C.byref(c_params(p))) and fog_ref.params_ok(p), kw
    for kw in bad:
        p = fog_ref.params(**kw)
        assert not host.fog_params_ok(C.byref(c_params(p))) and not fog_ref.params_ok(p), kw


def test_struct_layout_defaults_and_names(host):
    lay = np.zeros(13, np.uint32)
    host.fog_layout(ptr(lay))
    P = state.FogParams
    assert list(lay) == [C.sizeof(P), P.albedo.offset, P.anisotropy.offset, P.light_dir.offset, P.light_irradiance.offset, P.ambient.offset,
                         P.max_distance.offset, P.steps.offset, P.flags.offset, state.FOG_MAX_STEPS, state.FOG_JITTER, state.ALL_SOURCES["fog"], 76]
    assert C.sizeof(P) == 68 and [f[0] for f in P._fields_] == list(fog_ref.FIELDS)
    assert fog_ref.MAX_STEPS == state.FOG_MAX_STEPS == 64 and fog_ref.JITTER == state.FOG_JITTER == 1
    d = P()
    host.fog_defaults(C.byref(d))
    got = {"density": d.density, "albedo": tuple(d.albedo), "anisotropy": d.anisotropy, "light_dir": tuple(d.light_dir),
           "light_irradiance": tuple(d.light_irradiance), "ambient": tuple(d.ambient), "max_distance": d.max_distance, "steps": d.steps, "flags": d.flags}
    assert got == fog_ref.params() == fog_ref.params(**state.FOG_DEFAULTS)
    assert (got["density"], got["albedo"], got["anisotropy"], got["ambient"], got["max_distance"], got["steps"], got["flags"]) == \
        (float(F(0.05)), (1.0,) * 3, float(F(0.6)), (0.0,) * 3, 50.0, 16, 1)
    assert state.ALL_SOURCES == dict(state.DISPLAY_SOURCES, fog=6) and "fog" not in state.DISPLAY_SOURCES
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_EXPOSURE_FOG = 6" in hdr
    for n in FOG_SYMBOLS:
        assert n in state._SYMBOLS and ("rsrt_status %s(" % n) in hdr and ("pub fn %s(" % n) in hdr, n
    with pytest.raises(TypeError):
        state.FogParams.of(thickness=1.0)
    assert state.FogParams.of(jitter=False).flags == 0 and state.FogParams.of(jitter=True).flags == 1
    import inspect
    sig = inspect.signature(R.State.fog).parameters
    assert [k for k in sig if k != "self"][:3] == ["source", "out_ptr", "stream"] and sig["source"].default == "mean"
    sig = inspect.signature(R.State.render_fog).parameters
    assert [k for k in sig if k != "self"][:2] == ["n", "sample_begin"] and sig["n"].default is None and sig["sample_begin"].default is None


FOG_SYMBOLS = ("rsrt_fog_render", "rsrt_fog_bind", "rsrt_fog_clear", "rsrt_fog_download", "rsrt_fog_apply", "rsrt_fog_image_download", "rsrt_fog_reset")


def test_library_exports_the_fog_pass():
    lib = C.CDLL(_build.build_hip())
    for n in FOG_SYMBOLS:
        assert hasattr(lib, n), n
    for m in ("render_fog", "clear_fog", "download_fog", "fog_reset", "fog", "fog_download", "fog_light_from_sky", "bind_fog"):
        assert hasattr(R.State, m), m
    assert not hasattr(state.MultiState, "fog")  # (no image pass lives there)


KERNELS = ("rt_fog_kernel", "rt_fog_compose_kernel")


def test_fog_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel, count in zip(KERNELS, (2, 1)):  # (the march: one for the scene in LDS, one for global memory)
        names = [n for n in md if kernel in n]
        assert len(names) == count, (kernel, names)
        for n in names:
            k = md[n]
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)


def closed_form(p, d, L, lit):
    """(S_sun + S_amb) (1 - e^(-sigma L)) / sigma in float64, S_amb alone when occluded."""
    g, sigma = float(F(p["anisotropy"])), float(F(p["density"]))
    cos = float(np.dot(np.asarray(d, np.float64), np.asarray(p["light_dir"], np.float64)))
    phase = (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * cos) ** 1.5)
    sigma_s = sigma * np.asarray(p["albedo"], np.float64)
    s = sigma_s * np.asarray(p["ambient"], np.float64)
    if lit:
        s = s + sigma_s * phase * np.asarray(p["light_irradiance"], np.float64)
    return s * (1 - np.exp(-sigma * L)) / sigma, np.exp(-sigma * L)


def test_the_restatement_agrees_with_the_closed_form_of_a_lit_and_an_occluded_ray():
    """The whole march of one fully lit and one fully occluded pixel of `house` under a low sun (772 and 1110 such pixels of 3600),
    jitter off, sigma L = 1, 32 steps, against the float64 closed form.  The tolerance is the midpoint rule's relative error (sigma delta)^2 / 24 plus 2^-16 for rsrt_sky_exp2's published
    2^-17 and the f32 sum of at most 64 terms."""
    import denoise_ref
    sc = R.Scene.load_toml(util.scene_path("house"))
    osc = util.oracle_scene(sc)
    cam = np.array(sc.camera_uniform()).view(state.T.CAMERA).reshape(1)[0]
    w, h, steps, k = 80, 45, 32, 3
    base = dict(light_dir=fog_ref.unit((0.45, 0.2, 0.8)), albedo=(0.9, 0.8, 0.7), light_irradiance=(4.0, 3.0, 2.0), ambient=(0.2, 0.3, 0.4), max_distance=20.0, steps=steps, flags=0)
    _, lit = fog_ref.records(osc, cam, w, h, k, 1, fog_ref.params(density=0.1, **base))
    lit = lit[0]
    full, none = np.argwhere(lit.all(axis=-1)), np.argwhere(~lit.any(axis=-1))
    assert len(full) and len(none)
    for (y, x), is_lit in ((full[len(full) // 2], True), (none[len(none) // 2], False)):
        o, d = denoise_ref.camera_rays(cam, w, h, np.array([x]), np.array([y]), k)
        hit = __import__("oracle").cast_rays(osc, o, d, mode=0)
        L = min(float(hit["distance"][0]), 20.0) if hit["did_hit"][0] else 20.0
        p = fog_ref.params(density=1.0 / L, **base)
        rec, lit1 = fog_ref.records(osc, cam, w, h, k, 1, p, rows=[y])
        assert lit1[0, y, x].all() == is_lit and lit1[0, y, x].any() == is_lit  # (visibility does not depend on the density)
        sigma = float(F(p["density"]))
        want, want_t = closed_form(p, d[0], L, is_lit)
        tol = (sigma * L / steps) ** 2 / 24 + 2.0 ** -16
        got = rec[y, x].astype(np.float64)
        assert abs(sigma * L - 1) < 1e-6 and (want > 0).all()
        assert (np.abs(got[:3] - want) <= tol * want).all(), (is_lit, got, want, tol)
        assert abs(got[3] - want_t) <= 2.0 ** -16 * want_t, (got[3], want_t)


@pytest.mark.parametrize("kw,height", [({}, 1024), ({"sun_azimuth": 2.2, "sun_elevation": 0.3, "turbidity": 6.0}, 64), ({"sun_radius": 0.05, "scale": 1.0}, 2048),
                                       ({"sun_illuminance": 0.0}, 512)])
def test_light_from_sky_is_the_skys_sun(host, kw, height):
    sp = sky_ref.params(**kw)
    cp = state.SkyParams.of(**sp)
    d, e = np.full(3, 7, F), np.full(3, 7, F)
    assert host.fog_light_from_sky(C.byref(cp), height, ptr(d), ptr(e)) == 0
    want_d, want_e = fog_ref.light_from_sky(sp, height)
    k = sky_ref.prepare(sp, height)
    assert same(d, want_d) and same(e, want_e) and same(d, np.asarray(k["sun_dir"], F))  # the direction: sky_ref's sun, bit for bit
    omega = 4 * np.pi * np.sin(float(k["r_eff"]) / 2) ** 2
    want64 = np.asarray(k["sun_radiance"], np.float64) * omega
    assert np.allclose(e, want64, rtol=1e-6, atol=0) and (want64 > 0).all() == (sp["sun_illuminance"] > 0)
    lp = fog_ref.params(light_dir=tuple(float(x) for x in d), light_irradiance=tuple(float(x) for x in e))
    assert fog_ref.params_ok(lp) and host.fog_params_ok(C.byref(c_params(lp)))
    # the package's own entry (librsrt_host.so) gives the same bits
    got = R.host.fog_light_from_sky(height, **sp)
    assert same(np.array(got["light_dir"], F), d) and same(np.array(got["light_irradiance"], F), e)
    # widening cancels: a coarse map's wide disc carries the irradiance of a fine map's true disc
    if sp["sun_illuminance"] > 0 and sp["sun_radius"] < 0.01:
        fine = fog_ref.light_from_sky(sp, 1 << 14)[1]
        assert np.allclose(e, fine, rtol=1e-5)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "fog_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "fog_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_fog_compiles(tmp_path):
    build_cpp_demo(tmp_path)
