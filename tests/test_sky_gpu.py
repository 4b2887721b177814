"""The procedural daylight sky on the device: rsrt_environment_sky's texels against the CPU fill and the numpy restatement
(tests/sky_ref.py; tests/test_sky.py shows without a GPU that the two agree) bit for bit, the alias table the device builds over them
against the host builder, a slot filled by the sky against a slot the same texels and the host's table were uploaded to (the
accumulators must be the same bits), rsrt_environment_download for skies, uploads and empty slots, replacement across sizes, every
refusal with what it must leave alone and the one thing it drops, a moving sun, tools/render_png.py sky= and the C++ State.
Frames are house at 32 x 32, 4 spp, 3 bounces; maps are at most 256 x 128."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import sky_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host as H, types as T

pytestmark = pytest.mark.gpu
INVALID, NOT_READY = 1, 4
F = np.float32
W, HH, SPP, BOUNCES = 32, 32, 4, 3
SIZES = sky_ref.SIZES + [(1, 1)]
TURNED = sky_ref.CASES["turned"]


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def raises(status, call):
    with pytest.raises(R.RsrtError) as e:
        call()
    assert e.value.status == status, e.value


_scene = []


def context(envs=None):
    """house at 32 x 32 with the 64 x 32 synthetic map in slot 0 (or `envs`)."""
    if not _scene:
        _scene.append(R.Scene.load_toml(util.scene_path("house")))
    st = R.State.new(_scene[0], [util.small_env(64, 32)] if envs is None else envs, W, HH)
    st.max_bounces = BOUNCES
    return st


def render(st, slot):
    st.environment_index = slot
    st.clear()
    st.render_range(0, SPP)
    return st.download()


def twin_picture(slot, env):
    """What a fresh context renders with `env` — texels and the host's alias table — uploaded to `slot` beside the synthetic slot 0."""
    st = context()
    try:
        if slot != 0:
            assert same(render(st, 0), synthetic_picture())
        st.upload_environment(slot, env)
        return render(st, slot)
    finally:
        st.close()


_pictures = {}


def synthetic_picture():
    if "synthetic" not in _pictures:
        st = context()
        try:
            _pictures["synthetic"] = render(st, 0)
        finally:
            st.close()
    return _pictures["synthetic"]


@pytest.fixture(scope="module")
def live():
    st = context()
    yield st
    st.close()


# ---------------------------------------------------------------------------------------------------- a: the texels
@pytest.mark.parametrize("case", sorted(sky_ref.CASES))
def test_device_fill_equals_the_cpu_fill_bit_for_bit(live, case):
    kw = sky_ref.CASES[case]
    for w, h in SIZES:  # 37: no multiple of a wave or of the workgroup; 256: a whole workgroup; 1 x 1
        live.environment_sky(2, w, h, **kw)
        got = live.environment_download(2)
        assert got.shape == (h, w, 4) and not got[..., 3].any()
        assert same(got, H.sky_fill(w, h, **kw)), (case, w, h, int((util.bits(got) != util.bits(H.sky_fill(w, h, **kw))).sum()))
        assert same(got, sky_ref.reference(case, w, h)), (case, w, h)


def test_wide_and_tall_maps_cover_every_texel(live):
    """More than one workgroup along a row (600 columns: two whole ones and a part), and a map of one column."""
    for w, h in ((600, 3), (1, 70), (257, 2)):
        live.environment_sky(2, w, h, **TURNED)
        assert same(live.environment_download(2), H.sky_fill(w, h, **TURNED)), (w, h)


@pytest.mark.parametrize("w,h", [(37, 19), (64, 32), (1, 1)])
def test_alias_table_of_a_sky_equals_the_host_builder(live, w, h):
    L = R.state.lib()
    L.rsrt_environment_build_alias.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    live.environment_sky(3, w, h, **TURNED)
    texels = live.environment_download(3)
    out, left = np.zeros(w * h, T.ALIAS_ENTRY), C.c_uint32(0xffffffff)
    assert L.rsrt_environment_build_alias(live._ctx, 3, out.ctypes.data_as(C.c_void_p), w * h, C.byref(left)) == 0, L.rsrt_last_error(live._ctx)
    want, leftover = R.AliasTable.build_by_luminance(texels[:, :, :3])
    for f in ("probability", "alias_index", "pmf"):
        assert np.array_equal(out[f].view(np.uint32), want[f].view(np.uint32)), f
    assert left.value == leftover
    assert same(live.environment_download(3), texels)  # (the packed pmf copies in the texels' alpha stay the library's own)


# ---------------------------------------------------------------------------------------------------- b: slot wiring
def test_a_sky_slot_renders_as_its_upload_twin():
    env = R.Environment.sky(64, 32, **TURNED)
    want = twin_picture(1, env)
    st = context()
    try:
        st.environment_sky(1, 64, 32, **TURNED)
        got = render(st, 1)
        assert same(got, want), int((util.bits(got) != util.bits(want)).sum())
        assert same(render(st, 0), synthetic_picture())  # slot 0 renders as before
        assert not same(got, synthetic_picture()) and np.isfinite(got).all() and got[..., :3].max() > 0
    finally:
        st.close()


def test_download_returns_what_a_slot_holds(live):
    env = util.small_env(64, 32)
    got = live.environment_download(0)
    assert same(got, env.rgba) and not got[..., 3].any()  # an uploaded map: the uploaded bits, its table's pmf copies not among them
    raises(NOT_READY, lambda: live.environment_download(9))       # beyond every filled slot
    live.environment_sky(6, 8, 4)
    raises(NOT_READY, lambda: live.environment_download(5))       # an empty slot below a filled one
    L, out = live._L, np.zeros(8 * 4 * 4 + 1, F)
    for n in (8 * 4 * 4 - 1, 8 * 4 * 4 + 1, 0):
        assert L.rsrt_environment_download(live._ctx, 6, out.ctypes.data_as(C.c_void_p), n) == INVALID
    assert L.rsrt_environment_download(live._ctx, 6, None, 8 * 4 * 4) == INVALID
    assert L.rsrt_environment_download(live._ctx, 6, out.ctypes.data_as(C.c_void_p), 8 * 4 * 4) == 0
    assert same(out[:-1].reshape(4, 8, 4), H.sky_fill(8, 4)) and out[-1] == 0


def test_replacement_across_sizes():
    """A sky of 64 x 32 over an uploaded 8 x 4 slot, then a sky of 8 x 4 over that: each renders as its upload twin."""
    st = context([R.Environment.synthetic(8, 4)])
    try:
        assert same(render(st, 0), twin_picture(0, R.Environment.synthetic(8, 4)))
        for w, h, kw in ((64, 32, TURNED), (8, 4, {}), (37, 19, {"turbidity": 10.0})):
            st.environment_sky(0, w, h, **kw)
            assert same(st.environment_download(0), H.sky_fill(w, h, **kw))
            assert same(render(st, 0), twin_picture(0, R.Environment.sky(w, h, **kw))), (w, h)
        st.upload_environment(0, util.small_env(64, 32))  # and an upload over a sky
        assert same(render(st, 0), synthetic_picture()) and same(st.environment_download(0), util.small_env(64, 32).rgba)
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- c: refusals
@pytest.fixture(scope="module")
def guarded():
    """Slot 0 the synthetic map, slot 1 a sky; their texels and pictures, which no refusal may change."""
    st = context()
    st.environment_sky(1, 64, 32, **TURNED)
    st.kept = {"tex0": st.environment_download(0), "tex1": st.environment_download(1), "pic1": render(st, 1)}
    yield st
    st.close()


def sky_call(st, slot=1, w=64, h=32, **kw):
    return lambda: st.environment_sky(slot, w, h, **dict(sky_ref.DEFAULTS, **kw))


def null_params(st):
    def call():
        st._check(st._L.rsrt_environment_sky(st._ctx, 1, 64, 32, None), "rsrt_environment_sky")
    return call


OTHER_REFUSALS = {"slot_64": lambda st: sky_call(st, slot=64), "zero_width": lambda st: sky_call(st, w=0), "zero_height": lambda st: sky_call(st, h=0),
                  "too_many_texels": lambda st: sky_call(st, w=65536, h=32768), "null_params": null_params,
                  "empty_slot_refused": lambda st: sky_call(st, slot=7, turbidity=1.0)}


@pytest.mark.parametrize("name", sorted(sky_ref.REFUSED) + sorted(OTHER_REFUSALS))
def test_a_refused_call_changes_nothing_but_the_temporal_history(guarded, name):
    st = guarded
    st.environment_index = 1
    st.render_temporal(1)  # a history to lose, and an accumulator with a sample in it
    assert st.download_temporal()[..., 3].any()
    acc = st.download()
    call = OTHER_REFUSALS[name](st) if name in OTHER_REFUSALS else sky_call(st, **sky_ref.REFUSED[name])
    raises(INVALID, call)
    raises(NOT_READY, st.download_temporal)  # dropped first thing, as a refused upload drops it
    assert same(st.download(), acc)          # the accumulator is not touched
    assert same(st.environment_download(0), st.kept["tex0"]) and same(st.environment_download(1), st.kept["tex1"])
    raises(NOT_READY, lambda: st.environment_download(7))
    assert same(render(st, 1), st.kept["pic1"])


def test_an_accepted_call_drops_the_history_and_leaves_the_accumulator(guarded):
    st = guarded
    st.environment_index = 1
    st.render_temporal(1)
    acc = st.download()
    st.environment_sky(4, 8, 4)
    raises(NOT_READY, st.download_temporal)
    assert same(st.download(), acc)
    assert same(render(st, 1), st.kept["pic1"])


# ---------------------------------------------------------------------------------------------------- d: a moving sun
def test_moving_the_sun_on_one_slot():
    first, second = dict(TURNED), dict(TURNED, sun_azimuth=-0.4)
    st = context()
    try:
        st.environment_sky(1, 64, 32, **first)
        before = render(st, 1)
        st.environment_sky(1, 64, 32, **second)
        assert same(st.environment_download(1), H.sky_fill(64, 32, **second))
        moved = render(st, 1)
    finally:
        st.close()
    fresh = context()
    try:
        fresh.environment_sky(1, 64, 32, **second)
        assert same(moved, render(fresh, 1))
    finally:
        fresh.close()
    assert not same(moved, before)


# ---------------------------------------------------------------------------------------------------- e: the tool and the C++ State
def test_render_png_with_a_sky(tmp_path):
    pics = []
    for k in range(2):
        out = str(tmp_path / ("out%d.png" % k))
        cmd = [sys.executable, os.path.join(util.ROOT, "tools", "render_png.py"), "house", "96", "54", "4", "3", out, "sky=35,120", "exposure=auto"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        assert "sky: sun at elevation 35" in r.stdout and "metered exposure" in r.stdout, r.stdout
        pics.append(np.array(Image.open(out)))
    a = pics[0][..., :3]
    assert pics[0].shape == (54, 96, 4) and np.array_equal(pics[0], pics[1])
    assert a.min() != a.max() and (a < 255).mean() > 0.5 and len(np.unique(a.reshape(-1, 3), axis=0)) > 100  # not constant, not all white


def test_cpp_state_fills_a_sky_like_the_python_state(tmp_path):
    import test_sky
    exe = test_sky.build_cpp_demo(tmp_path)
    r = subprocess.run([exe, util.scene_path("house"), str(W), str(HH), str(BOUNCES), "64", "32", str(SPP), "35", "120"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    rad = F(sky_ref.PIF / F(180))
    kw = {"sun_elevation": float(F(F(35) * rad)), "sun_azimuth": float(F(F(120) * rad))}
    st = context()
    try:
        st.environment_sky(1, 64, 32, **kw)
        sky = st.environment_download(1)
        assert same(sky, H.sky_fill(64, 32, **kw))
        assert ["sky", "64", "32", "%016x" % sky_ref.fnv1a(sky)] in lines, r.stdout
        assert ["host", "%016x" % sky_ref.fnv1a(sky)] in lines and ["slot0", "kept"] in lines
        st.environment_index = 1
        st.render_samples(SPP)
        assert ["render", "%016x" % sky_ref.fnv1a(st.download())] in lines
        kw["sun_azimuth"] = float(F(F(kw["sun_azimuth"]) + F(1)))
        st.environment_sky(1, 64, 32, **kw)
        assert ["moved", "%016x" % sky_ref.fnv1a(st.environment_download(1))] in lines
        assert ["refused", "yes"] in lines
    finally:
        st.close()
