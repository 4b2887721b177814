"""The environment edge cases of tests/edge_envs.py without a GPU: the host alias-table builder against the checker's on every
library-built map, the checker's environment functions against the independent float64 reading of test_independent_shading.py on
EVERY case (that test reads the synthetic 64x32 sky at random directions only) with the poles, the seam and every texel corner and
centre of the small maps among the directions, and the finiteness of every reference the GPU tests compare with."""
import ctypes as C

import numpy as np
import pytest

import edge_envs as V
import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from test_independent_shading import Skip, bilinear, dir_to_uv, env_pdf, normalize, ptr, sample_env, uv_to_dir

UV_TOL = 2e-5  # test_environment_functions_agree_with_an_independent_float64_reading's tolerance on u and v


@pytest.mark.parametrize("name", V.LIBRARY_NAMES)
def test_host_builder_is_the_checkers_table(name):
    env = V.case(name).env
    got, left = R.AliasTable.build_by_luminance(env.rgba[:, :, :3])
    want, oleft = oracle.alias_table(env.rgba[:, :, :3])
    assert util.fields_equal(got, want) and left == oleft == env.leftover
    assert util.fields_equal(env.alias, want)
    n = len(got)
    if name == "black":  # sum 0: every p is NaN, nothing is small or large, every entry keeps its default
        assert np.array_equal(got["probability"], np.ones(n, np.float32)) and np.array_equal(got["alias_index"], np.arange(n))
        assert np.array_equal(got["pmf"], np.full(n, np.float32(1) / np.float32(n))) and left == n
    if name == "spike":  # every small entry is paired with the one lit texel
        lit = 1 * 5 + 1
        assert all(got["alias_index"][i] == lit for i in range(n) if i != lit)


def test_caller_tables_are_what_the_case_table_says():
    n = V.CALLER_W * V.CALLER_H
    i = np.arange(n)
    pmf = ((i + 1) / 120.0).astype(np.float32)
    u, c, s = (V.case(k).env for k in ("uniform", "chain", "never_self"))
    assert np.array_equal(u.rgba, c.rgba) and np.array_equal(u.rgba, s.rgba) and u.rgba.shape == (3, 5, 4)
    assert np.array_equal(u.alias["alias_index"], i) and (u.alias["probability"] == 1).all() and (u.alias["pmf"] == np.float32(1) / np.float32(15)).all()
    assert np.array_equal(c.alias["alias_index"], (i + 1) % n) and (c.alias["probability"] == 0.5).all() and np.array_equal(c.alias["pmf"], pmf)
    assert np.array_equal(s.alias["alias_index"], (i + 7) % n) and (s.alias["probability"] == 0).all() and np.array_equal(s.alias["pmf"], pmf)
    assert len(set(pmf.tolist())) == n  # a wrong entry's pmf is another number
    assert not any(V.case(k).library for k in ("uniform", "chain", "never_self")) and all(V.case(k).library for k in V.LIBRARY_NAMES)
    assert [k.name for k in V.cases()] == V.NAMES


def directed(env):
    """The poles, the seam with both signs of the zero, +x likewise, +-z, and for maps of at most 64 texels the direction of every texel
    corner and every texel centre (float64 uv_to_dir, rounded to f32)."""
    out = [(0, 1, 0), (0, -1, 0), (1, 0, 0.0), (-1, 0, 0.0), (1, 0, -0.0), (-1, 0, -0.0), (0, 0, 1), (0, 0, -1)]
    w, h = env.width, env.height
    if w * h <= 64:
        out += [uv_to_dir(i / w, j / h) for j in range(h + 1) for i in range(w + 1)]
        out += [uv_to_dir((i + 0.5) / w, (j + 0.5) / h) for j in range(h) for i in range(w)]
    return [np.asarray(d, np.float64).astype(np.float32) for d in out]


def radiance_bound(rgba, value):
    """sky_light and the sampled radiance are piecewise linear in (u, v); u and v may each be off by UV_TOL, which moves the value by at
    most UV_TOL * (w * the largest horizontal neighbour difference + h * the largest vertical one), per channel — on top of the
    existing test's rtol 2e-3 and atol 1e-3."""
    h, w = rgba.shape[:2]
    rgb = rgba[:, :, :3].astype(np.float64)
    dx = np.abs(np.diff(rgb, axis=1)).max(axis=(0, 1)) if w > 1 else np.zeros(3)
    dy = np.abs(np.diff(rgb, axis=0)).max(axis=(0, 1)) if h > 1 else np.zeros(3)
    return UV_TOL * (w * dx + h * dy) + 2e-3 * np.abs(value) + 1e-3


@pytest.mark.parametrize("name", V.NAMES)
def test_environment_functions_agree_with_the_float64_reading_on_every_case(name):
    """Seam convention: rsrt_atan2f does not distinguish signed zeros, y = -0 behaves as +0 (include/rsrt_detmath.h), so the direction
    (-1, 0, -0) maps to u = 1 like (-1, 0, +0), not to u = 0 as IEEE atan2 has it — and under the clamp-to-edge sampler the map is
    discontinuous exactly there.  Nor is x = -0 told from +0: the corner directions of the first and last row are (-0, +-1, -0), where
    IEEE atan2 gives pi and rsrt_atan2f 0 (WGSL leaves atan2 at the origin open).  The float64 reading follows the documented
    convention: every -0 of the direction is read as +0 (`+ 0.0`).
    Skip is raised where test_independent_shading raises it (a truncation within eps of an integer, a coin within the guard); corner
    directions raise it by design, so completion is counted on the random directions and draws alone: 85 % of them at least."""
    L = oracle.lib()
    L.orc_environment_direction_pdf.restype = C.c_float
    L.orc_sample_environment.restype = C.c_float
    env = V.case(name).env
    oenv = util.oracle_env(env)
    rng = np.random.default_rng(V.NAMES.index(name) + 40)
    n_random = 600
    dirs = [(normalize(rng.normal(size=3)).astype(np.float32), True) for _ in range(n_random)] + [(d, False) for d in directed(env)]
    pdf_done = sample_done = 0
    for trial, (d, is_random) in enumerate(dirs):
        d64 = d.astype(np.float64) + 0.0  # the convention: -0 is +0
        uv = np.zeros(2, np.float32)
        L.orc_direction_to_uv(ptr(d), ptr(uv))
        u, v = dir_to_uv(d64)
        assert np.allclose(uv, (u, v), atol=UV_TOL), (name, trial, d, uv, (u, v))
        sky = np.zeros(3, np.float32)
        L.orc_sky_light(C.byref(oenv.c), ptr(d), ptr(sky))
        want_sky = bilinear(env.rgba, u, v)
        assert np.all(np.abs(sky - want_sky) <= radiance_bound(env.rgba, want_sky)), (name, trial, d, sky, want_sky)
        try:
            want = env_pdf(env, d64)
            got = L.orc_environment_direction_pdf(C.byref(oenv.c), ptr(d))
            assert abs(got - want) <= 1e-3 * max(1.0, abs(want)), (name, trial, d, got, want)
            pdf_done += is_random
        except Skip:
            pass
        if not is_random:
            continue
        seed = int(rng.integers(0, 2 ** 32))
        st = C.c_uint32(seed)
        dir_out, rad = np.zeros(3, np.float32), np.zeros(3, np.float32)
        got_pdf = L.orc_sample_environment(C.byref(oenv.c), C.byref(st), ptr(dir_out), ptr(rad))
        try:
            w_dir, w_rad, w_pdf, w_state = sample_env(env, seed)
        except Skip:
            continue
        assert st.value == w_state, (name, trial, "four draws per environment sample")
        assert np.allclose(dir_out, w_dir, atol=1e-4), (name, trial, dir_out, w_dir)
        assert np.all(np.abs(rad - w_rad) <= radiance_bound(env.rgba, w_rad)), (name, trial, rad, w_rad)
        assert abs(got_pdf - w_pdf) <= 1e-3 * max(1.0, abs(w_pdf)), (name, trial, got_pdf, w_pdf)
        sample_done += 1
    print("%s: pdf completed on %d, draws on %d of %d random ones" % (name, pdf_done, sample_done, n_random))
    assert 100 * pdf_done >= 85 * n_random and 100 * sample_done >= 85 * n_random, (name, pdf_done, sample_done)


def test_signed_zero_at_the_seam_is_read_as_plus_zero():
    """The convention the reading above follows, at the one direction where it matters: both zeros give u = 1 (the map's last column)."""
    L = oracle.lib()
    got = []
    for z in (0.0, -0.0):
        d, uv = np.float32([-1, 0, z]), np.zeros(2, np.float32)
        L.orc_direction_to_uv(ptr(d), ptr(uv))
        got.append(uv.copy())
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and abs(float(got[0][0]) - 1.0) <= UV_TOL and got[0][1] == 0.5


@pytest.mark.parametrize("name", V.NAMES)
def test_references_are_finite(name):
    """What test_env_edges_gpu.py compares bit for bit has no NaN and no inf (edge_envs.reference asserts it; a case that stops being
    finite fails here and there).  Only `wild`, with its negative texels, may have negative pixels."""
    for scene in V.SCENES:
        img, st = V.reference(name, scene)
        assert np.isfinite(img).all() and st["paths"] == V.W * V.H * V.SPP
        assert st["escapes"] > 0 and st["nee_events"] > 0, (name, scene)  # the environment is both looked up and sampled
        if name != "wild":
            assert (img >= 0).all(), (name, scene)


def test_rebuilt_table_is_another_table_with_a_finite_reference():
    """The repacking test replaces `chain` by the library's table of the same texels: the two differ in every field, and so do the pictures."""
    chain, host = V.case("chain").env, V.rebuilt("chain")
    assert np.array_equal(chain.rgba, host.rgba)
    assert not any(np.array_equal(chain.alias[f], host.alias[f]) for f in ("probability", "alias_index", "pmf"))
    for scene in V.SCENES:
        a, b = V.reference("chain", scene)[0], V.reference("rebuilt:chain", scene)[0]
        assert np.isfinite(b).all() and not np.array_equal(a, b)


@pytest.mark.parametrize("camera", sorted(V.SKY_CAMERAS))
def test_open_sky_cameras_look_where_they_say(camera):
    cam = V.SKY_CAMERAS[camera]
    want = {"pole_up": (0, 1, 0), "pole_down": (0, -1, 0), "seam": (-1, 0, 0)}[camera]
    assert np.array_equal(E.centre_ray(cam[0]), np.float32(want))
    rot = np.asarray(cam["rot_transform"][0], np.float64)[:, :3]
    assert np.array_equal(rot @ rot.T, np.eye(3)) and np.linalg.det(rot) == 1.0
    for name in ("quad", "strip", "pillar", "odd_noise"):
        img, st = V.reference(name, "cube", camera)
        assert np.isfinite(img).all() and st["escapes"] > 0
        if camera == "pole_up":  # nothing but sky: every camera ray escapes at once
            assert st["escapes"] == st["ext_rays"] == st["paths"]
        else:  # the cube is in the picture: some paths bounce off it before they escape
            assert st["ext_rays"] > st["paths"] and st["nee_events"] > 0
