"""Volumetric fog on the GPU (rsrt_fog_render, rsrt_fog_apply and their buffers): the records against the numpy restatement
(tests/fog_ref.py: the checker's hits and shadow queries), bit for bit, on the scenes and the shapes where the march kernel can go wrong;
split calls, the clear and a caller's buffer; the compose step; the fog image as a source of the lens, the shutter, the meter and the
displays; nothing else written; the documented refusals and what they leave; the C++ State; one picture-level check of the shafts."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import dof_ref
import exposure_ref
import fog_ref
import motion_ref
import sky_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_temporal_gpu import accumulate
from test_bloom_gpu import denoised, everything, fnv1a, raises, upsampled

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
LIGHT = fog_ref.unit((0.4, 0.6, -0.7))
BASE = dict(light_dir=LIGHT, light_irradiance=(4.0, 3.0, 2.0), ambient=(0.02, 0.03, 0.05), albedo=(0.9, 0.8, 0.7), max_distance=20.0)
CASES = {"default": (64, 48, 5), "house": (80, 45, 8), "suzanne": (48, 32, 8)}


def equal(a, b):
    return a.shape == b.shape and np.array_equal(util.bits(a), util.bits(b))


@functools.lru_cache(maxsize=None)
def loaded(name):
    sc = R.Scene.load_toml(util.scene_path(name))
    return sc, util.oracle_scene(sc)


@functools.lru_cache(maxsize=None)
def reference(name, w, h, steps, flags, begin=3, count=2):
    """The restatement of one case, computed once: (records, lit)."""
    sc, osc = loaded(name)
    cam = np.array(sc.camera_uniform()).view(R.state.T.CAMERA).reshape(1)[0]
    return fog_ref.records(osc, cam, w, h, begin, count, fog_ref.params(steps=steps, flags=flags, **BASE))


def new_state(name, w, h):
    return R.State.new(loaded(name)[0], util.small_env(), w, h)


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_records_equal_the_restatement_bit_for_bit(name, jitter):
    w, h, steps = CASES[name]
    want, lit = reference(name, w, h, steps, jitter)
    # a comparison where everything is lit or everything is dark shows nothing (jitter off: default 0.177, house 0.290, suzanne 0.098)
    share = 1.0 - lit.mean()
    mixed = (lit[0].any(axis=-1) & ~lit[0].all(axis=-1)).mean()
    print("%s jitter %d: occluded share %.3f, mixed pixels %.3f" % (name, jitter, share, mixed))
    assert 0.05 <= share <= 0.95 and mixed > 0.1
    st = new_state(name, w, h)
    try:
        p = dict(BASE, steps=steps, flags=jitter)
        st.render_fog(2, 3, **p)
        got = st.download_fog()
        assert equal(got, want)
        assert st.fog_sample_count == 2 and (st.fog_width, st.fog_height) == (w, h)
        st.clear_fog()
        assert not st.download_fog().any() and st.fog_sample_count == 0
        st.render_fog(1, 3, **p)  # [3, 4) then [4, 5) gives the bits of [3, 5)
        st.render_fog(1, 4)       # (the remembered parameters)
        assert equal(st.download_fog(), want)
        mine = DeviceArray(np.zeros((h, w, 4), F))  # a bound caller buffer receives the same bits
        st.bind_fog(mine.data_ptr(), w, h)
        st.render_fog(2, 3, **p)
        st.synchronize()
        assert equal(mine.numpy(), want) and equal(st.download_fog(), want)
        st.bind_fog(None, 0, 0)
    finally:
        st.close()


@pytest.mark.parametrize("w,h,steps", [(1, 1, 5), (67, 5, 1), (67, 5, 64)])
def test_small_and_ragged_frames_and_both_ends_of_the_step_range(w, h, steps):
    """1 x 1; 67 x 5: fewer than a wave in the last row and a width that is no multiple of 64; steps 1 and 64."""
    want, _ = reference("default", w, h, steps, 1, 7, 1)
    st = new_state("default", w, h)
    try:
        st.render_fog(1, 7, **dict(BASE, steps=steps))
        assert equal(st.download_fog(), want) and want[..., 3].all()
    finally:
        st.close()


def test_a_scene_too_large_for_lds_runs_the_global_memory_form(tmp_path):
    sc = R.Scene.load_toml(util.big_scene(tmp_path, 4))
    assert len(sc.triangles) == 15488
    w, h = 32, 20
    cam = np.array(sc.camera_uniform()).view(R.state.T.CAMERA).reshape(1)[0]
    want, lit = fog_ref.records(util.oracle_scene(sc), cam, w, h, 0, 1, fog_ref.params(steps=4, **BASE))
    assert lit.any() and not lit.all()
    st = R.State.new(sc, util.small_env(), w, h)
    try:
        st.render_fog(1, 0, **dict(BASE, steps=4))
        assert equal(st.download_fog(), want)
    finally:
        st.close()


def test_a_frame_with_more_pixels_than_the_grid_has_lanes():
    """1024 x 520 = 532480 pixels against CUs x 8 workgroups x 256 lanes (524288 on 256 CUs): the stride loop's second trip.  Checked on
    the first two rows and the last eight."""
    w, h = 1024, 520
    rows = [0, 1] + list(range(h - 8, h))
    sc, osc = loaded("default")
    cam = np.array(sc.camera_uniform()).view(R.state.T.CAMERA).reshape(1)[0]
    want, _ = fog_ref.records(osc, cam, w, h, 0, 1, fog_ref.params(steps=2, **BASE), rows=rows)
    st = new_state("default", w, h)
    try:
        st.render_fog(1, 0, **dict(BASE, steps=2))
        got = st.download_fog()
        assert equal(got[rows], want[rows]) and got[..., 3].all()  # (every pixel was visited: each record holds a transmittance > 0)
    finally:
        st.close()


@pytest.fixture(scope="module")
def rendered():
    """An 80 x 45 house frame with every image the library can hold and fog records of two samples: (state, {source: (its download,
    total, its records)}, the fog records, the fog parameters)."""
    w, h = 80, 45
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)  # accumulator + AOV (4 spp), the guide, the denoised and the upsampled (160 x 90) image
    accumulate(st, 4)                       # a first temporal frame of the same accumulator and AOV buffer
    st.exposure_meter()
    aov, guide = st.download_aov(), st.download_guide()
    images = {"mean": (st.download(), 4, aov), "denoised": (denoised(st), 1, aov), "temporal": (st.download_temporal(), 1, aov),
              "upsampled": (upsampled(st), 1, guide)}
    p = dict(BASE, steps=8, flags=0, density=0.2)
    st.render_fog(2, 3, **p)
    rec = st.download_fog()
    yield st, images, rec, p
    st.close()


def test_compose_equals_numpy_and_a_clear_medium_is_the_source(rendered):
    st, images, rec, p = rendered
    assert equal(rec, reference_with(p, 80, 45))
    before = everything(st) + [rec]
    fogged = {}
    for source in ("mean", "denoised"):
        img, total, _ = images[source]
        st.fog(source)
        got = st.fog_download()
        assert equal(got, fog_ref.compose(fog_ref.source_colour(img, total), rec, 2)), source
        assert (got[..., 3] == 1).all() and not equal(got[..., :3], fog_ref.source_colour(img, total))
        fogged[source] = got
    assert not equal(fogged["mean"], fogged["denoised"])
    st.fog("denoised", sample_total=0)  # sample_total is ignored for all sources but the mean
    assert equal(st.fog_download(), fogged["denoised"])
    mine = DeviceArray(np.zeros((45, 80, 4), F))  # into a caller's buffer, which the later passes then read
    st.fog("mean", out_ptr=mine.data_ptr())
    st.synchronize()
    assert equal(mine.numpy(), fogged["mean"]) and equal(st.fog_download(), fogged["mean"])
    st.fog("mean")
    # records of another size than the source
    raises(INVALID, lambda: st.fog("upsampled"))
    assert equal(st.fog_download(), fogged["mean"])
    for a, b in zip(before, everything(st) + [st.download_fog()]):
        assert equal(a, b)
    # density 0: every record is (0, 0, 0, 1) a sample and the fog image is the source bit for bit
    st.clear_fog()
    st.render_fog(2, 3, **dict(p, density=0.0))
    clear = st.download_fog()
    assert not clear[..., :3].any() and (clear[..., 3] == 2).all()
    for source in ("mean", "denoised"):
        img, total, _ = images[source]
        st.fog(source)
        assert equal(st.fog_download()[..., :3], fog_ref.source_colour(img, total)), source
    st.clear_fog()
    st.render_fog(2, 3, **p)
    assert equal(st.download_fog(), rec)


def reference_with(p, w, h):
    sc, osc = loaded("house")
    cam = np.array(sc.camera_uniform()).view(R.state.T.CAMERA).reshape(1)[0]
    return fog_ref.records(osc, cam, w, h, 3, 2, fog_ref.params(**p))[0]


def test_the_fog_image_is_a_source_of_the_later_passes(rendered):
    st, images, rec, p = rendered
    img, total, aov = images["mean"]
    st.fog("mean")
    fog = st.fog_download()
    assert equal(fog, fog_ref.compose(fog_ref.source_colour(img, total), rec, 2))
    st.exposure_meter("fog")
    hist, _ = st.exposure_download()
    assert np.array_equal(hist, exposure_ref.histogram(fog, 1))
    e = 1.7
    shown = st.display_exposed_srgb8("fog", e)
    assert shown.shape == fog.shape and np.array_equal(shown, exposure_ref.display(fog, 1, e))
    # the lens and the shutter read the fog image with the records of the image it was built from
    cam = dof_ref.Camera.from_record(st.camera)
    st.depth_of_field("fog", 3.0, 0.15, 5)
    lens = st.dof_download()
    assert util.same_bits_or_nan(lens, dof_ref.dof(fog, 1, aov, cam, 3.0, 0.15, 5)[0]) and not equal(lens, fog)
    previous = R.state.camera_earlier(st.camera, 0.05, 0.1)
    mcam, mprev = motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous)
    st.motion_blur("fog", previous, 0.5, 8, 8)
    assert util.same_bits_or_nan(st.motion_download(), motion_ref.motion(fog, 1, aov, mcam, mprev, 0.5, 8, 8)[0])
    st.motion_blur("lens", previous, 0.5, 8, 8)  # the lens image of the fog image carries the same records on
    assert util.same_bits_or_nan(st.motion_download(), motion_ref.motion(lens, 1, aov, mcam, mprev, 0.5, 8, 8)[0])
    # the fog of the upsampled image: records of the guide's size, and the guide for the lens
    st.render_fog(1, 0, size=(160, 90), **p)
    assert st.download_fog().shape == (90, 160, 4) and st.fog_sample_count == 1
    st.fog("upsampled")
    fog_up = st.fog_download()
    assert equal(fog_up, fog_ref.compose(fog_ref.source_colour(images["upsampled"][0]), st.download_fog(), 1))
    assert st.display_exposed_srgb8("fog", e).shape == (90, 160, 4)
    st.depth_of_field("fog", 3.0, 0.15, 5)
    assert util.same_bits_or_nan(st.dof_download(), dof_ref.dof(fog_up, 1, images["upsampled"][2], cam, 3.0, 0.15, 5)[0])
    # each pass goes on refusing its own output and what comes after it; 7 is still an unknown source everywhere
    good_d, good_m = R.state.DofParams(1.0, 0.01, 8, 0), R.state.MotionParams(0.5, 8, 8, 0)
    cam_p, prev_p = R.state._p(st.camera), R.state._p(previous)
    for source in (4, 5, 6, 7):
        raises(INVALID, lambda: st.fog(source))
    raises(INVALID, lambda: st._check(st._L.rsrt_dof(st._ctx, 5, 4, cam_p, C.byref(good_d), None, None), "rsrt_dof"))
    for call in (lambda: st._check(st._L.rsrt_dof(st._ctx, 7, 4, cam_p, C.byref(good_d), None, None), "rsrt_dof"),
                 lambda: st._check(st._L.rsrt_motion_blur(st._ctx, 7, 4, cam_p, prev_p, C.byref(good_m), None, None), "rsrt_motion_blur"),
                 lambda: st.exposure_meter(7), lambda: st.display_exposed_srgb8(7, 1.0), lambda: st.bloom(7, 1.0), lambda: st.local_exposure(7),
                 lambda: st.white_meter(7), lambda: st.fog(7)):
        with pytest.raises(R.RsrtError) as err:
            call()
        assert err.value.status == INVALID and "unknown source 7" in str(err.value)
    # back to the fixture's records
    st.render_fog(2, 3, size=(80, 45), **p)
    assert equal(st.download_fog(), rec)


def test_refusals_leave_records_and_image_as_they_were(rendered):
    st, images, rec, p = rendered
    st.fog("mean")
    fog = st.fog_download()
    before = everything(st) + [rec, fog]
    L, cam_p = st._L, R.state._p(st.camera)
    good = R.state.FogParams.of(**p)
    render = lambda cam, w, h, b, n, prm: st._check(L.rsrt_fog_render(st._ctx, cam, w, h, b, n, prm, None), "rsrt_fog_render")  # noqa: E731
    apply = lambda s, n, nf: st._check(L.rsrt_fog_apply(st._ctx, s, n, nf, None, None), "rsrt_fog_apply")  # noqa: E731
    raises(INVALID, lambda: render(None, 80, 45, 0, 1, C.byref(good)))       # NULL camera
    raises(INVALID, lambda: render(cam_p, 80, 45, 0, 1, None))               # NULL params
    for kw in ({"density": -1.0}, {"density": float("nan")}, {"albedo": 1.5}, {"anisotropy": 0.99}, {"light_dir": (0.0, 2.0, 0.0)}, {"light_irradiance": -1.0},
               {"ambient": float("inf")}, {"max_distance": 0.0}, {"steps": 0}, {"steps": 65}, {"flags": 2}):
        bad = R.state.FogParams.of(**dict(p, **kw))
        raises(INVALID, lambda: render(cam_p, 80, 45, 0, 1, C.byref(bad)))
    raises(INVALID, lambda: render(cam_p, 0, 45, 0, 1, C.byref(good)))       # a bad resolution
    raises(INVALID, lambda: render(cam_p, 80, 0, 0, 1, C.byref(good)))
    raises(INVALID, lambda: render(cam_p, 0x10000, 0x10000, 0, 1, C.byref(good)))
    raises(INVALID, lambda: render(cam_p, 80, 45, 0xffffffff, 2, C.byref(good)))  # the sample range overflows
    raises(INVALID, lambda: apply(0, 4, 0))                                  # fog_sample_total 0
    raises(INVALID, lambda: apply(0, 0, 2))                                  # sample_total 0 under the mean
    raises(INVALID, lambda: apply(3, 4, 2))                                  # records of another size than the source
    raises(INVALID, lambda: st._check(L.rsrt_fog_apply(st._ctx, 0, 4, 2, C.c_void_p(8), None), "rsrt_fog_apply"))  # a misaligned output
    for source in (4, 5, 6, 7):
        raises(INVALID, lambda: apply(source, 4, 2))
    raises(INVALID, lambda: st._check(L.rsrt_fog_download(st._ctx, None, 0), "rsrt_fog_download"))
    raises(INVALID, lambda: st._check(L.rsrt_fog_image_download(st._ctx, None, 0), "rsrt_fog_image_download"))
    st.set_partition(0, 2)  # whole frame only
    try:
        raises(INVALID, lambda: render(cam_p, 80, 45, 0, 1, C.byref(good)))
        raises(INVALID, lambda: apply(0, 4, 2))
    finally:
        st.set_partition(0, 1)
    for a, b in zip(before, everything(st) + [st.download_fog(), st.fog_download()]):
        assert equal(a, b)
    # NOT_READY: no scene, no records, no such source
    bare = R.State()
    try:
        raises(NOT_READY, lambda: bare._check(L.rsrt_fog_render(bare._ctx, cam_p, 8, 8, 0, 1, C.byref(good), None), "rsrt_fog_render"))
        raises(NOT_READY, lambda: bare._check(L.rsrt_fog_clear(bare._ctx), "rsrt_fog_clear"))
        raises(NOT_READY, lambda: bare._check(L.rsrt_fog_apply(bare._ctx, 0, 1, 1, None, None), "rsrt_fog_apply"))
    finally:
        bare.close()
    fresh = new_state("default", 16, 8)
    try:
        fresh.render_samples(1)
        raises(NOT_READY, lambda: fresh.fog("mean", fog_sample_total=1))     # no records
        raises(NOT_READY, lambda: fresh.download_fog())
        fresh.render_fog(1, 0, **dict(BASE, steps=2))
        raises(NOT_READY, lambda: fresh.fog("denoised"))                     # no such source
        raises(NOT_READY, lambda: fresh.fog_download())                      # no fog image yet
        raises(NOT_READY, lambda: fresh.exposure_meter("fog"))
        raises(NOT_READY, lambda: fresh.depth_of_field("fog"))
        fresh.fog("mean")
        assert fresh.fog_download().shape == (8, 16, 4)
        fresh.resize(24, 8)  # what drops the lens image drops the fog image; the records have a size of their own
        raises(NOT_READY, lambda: fresh.exposure_meter("fog"))
        assert fresh.download_fog().shape == (8, 16, 4)
        fresh.fog_reset()
        raises(NOT_READY, lambda: fresh.download_fog())
        assert fresh.fog_sample_count == 0 and fresh.fog_params is None
    finally:
        fresh.close()


def test_cpp_state_fogs_like_the_python_state(tmp_path):
    import test_fog
    exe = test_fog.build_cpp_demo(tmp_path)
    w, h, samples, steps, density = 64, 36, 3, 6, 0.2
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", str(samples), str(steps), str(density)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        light = st.fog_light_from_sky(height=512, sun_azimuth=2.0, sun_elevation=0.9)
        bits = lambda v: ["%08x" % int(x) for x in util.bits(np.array(v, F))]  # noqa: E731
        assert lines[0] == ["light"] + bits(light["light_dir"]) + bits(light["light_irradiance"])
        st.render_samples(samples, aov=True)
        st.render_fog(1, steps=steps, density=density, ambient=0.05, **light)
        st.render_fog(samples - 1)
        rec = st.download_fog()
        assert lines[1] == ["records", str(samples), "%016x" % fnv1a(rec.tobytes())]
        st.fog()
        img = st.fog_download()
        assert lines[2] == ["fog", str(img.size), "%016x" % fnv1a(img.tobytes())]
        st.depth_of_field("fog")
        assert lines[3] == ["lens", "%016x" % fnv1a(st.dof_download().tobytes())]
        e = st.auto_exposure("fog")["exposure"]
        assert lines[4] == ["exposure", bits([e])[0]]
        st.bloom("fog")
        shown = st.display_bloomed_srgb8("fog")
        assert lines[5] == ["display", str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        assert lines[6] == ["reset", "yes"]
    finally:
        st.close()


SUN = {"sun_azimuth": 1.0584, "sun_elevation": 0.2145}  # a low sun through house's openings: 6410 pixels at least 3/4 lit, 6471 at most 1/4 (of 14400)


def test_shafts_are_brighter_than_shade():
    """house 160 x 90 under environment_sky with the light from fog_light_from_sky, 16 spp, 16 steps, density 0.15: the mean inscatter
    over pixels whose march is at least three-quarters lit exceeds that over pixels at most one-quarter lit (the classes are the
    restatement's)."""
    w, h, n = 160, 90, 16
    sc, st = state("house", w, h)
    try:
        st.environment_sky(0, 256, 128, **SUN)
        light = st.fog_light_from_sky(**SUN)
        d, e = fog_ref.light_from_sky(sky_ref.params(**SUN), 128)
        assert equal(np.array(light["light_dir"], F), d) and equal(np.array(light["light_irradiance"], F), e)
        st.render_fog(n, 0, density=0.15, steps=16, **light)
        got = st.download_fog()
        osc = util.oracle_scene(sc)
        want, lit = fog_ref.records(osc, st.camera[0], w, h, 0, n, fog_ref.params(density=0.15, steps=16, **light))
        assert equal(got, want)
        share = lit.mean(axis=(0, 3))
        hi, lo = share >= 0.75, share <= 0.25
        inscatter = got[..., :3].mean(axis=-1) / F(n)
        print("lit pixels %d, shaded %d, inscatter %.3g against %.3g" % (hi.sum(), lo.sum(), inscatter[hi].mean(), inscatter[lo].mean()))
        assert hi.any() and lo.any()
        assert inscatter[hi].mean() > inscatter[lo].mean()
    finally:
        st.close()
