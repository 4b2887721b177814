"""The fog rebuild on the GPU (rsrt_fog_apply_upsampled): the fog image against the numpy restatement (tests/fog_upsample_ref.py), bit
for bit, on the sources, the ratios and the frame shapes where the kernels can go wrong; a clear medium; the fog image as a source of
the later passes with the right first-hit records; the documented refusals and what they leave; the C++ State; one picture-level check
of half-size fog against full-size fog of the same cost."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import dof_ref
import exposure_ref
import fog_ref
import fog_upsample_ref as ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_temporal_gpu import accumulate
from test_bloom_gpu import denoised, everything, fnv1a, raises, upsampled
from test_fog_gpu import BASE, equal, loaded

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32


def constants(p):
    return fog_ref.prepare(fog_ref.params(**p))


@pytest.fixture(scope="module")
def rendered():
    """An 80 x 45 house frame with the accumulator and the AOV buffer (4 spp), the denoised and the upsampled (160 x 90) image and its
    guide, and 40 x 23 fog records of 2 samples from index 3, jitter on: (state, {source: (its download, total, its first-hit records,
    their sample total)}, the fog records, the fog parameters)."""
    w, h = 80, 45
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)
    accumulate(st, 4)  # (a temporal frame, so that every image exists for the "nothing else was written" comparisons)
    st.exposure_meter()
    aov, guide = st.download_aov(), st.download_guide()
    images = {"mean": (st.download(), 4, aov, st.aov_sample_count), "denoised": (denoised(st), 1, aov, st.aov_sample_count),
              "upsampled": (upsampled(st), 1, guide, st.guide_sample_count)}
    p = dict(BASE, steps=8, flags=1, density=0.2)
    st.render_fog(2, 3, size=(40, 23), **p)
    rec = st.download_fog()
    yield st, images, rec, p
    st.close()


def want_image(images, source, rec, n, p):
    img, total, g, T = images[source]
    return ref.rebuild(fog_ref.source_colour(img, total), rec, n, g, T, constants(p))[0]


def test_the_fog_image_equals_the_restatement_bit_for_bit(rendered):
    st, images, rec, p = rendered
    # the low records themselves: the restatement's, with lit and shaded march points among them
    sc, osc = loaded("house")
    want_rec, lit = fog_ref.records(osc, st.camera[0], 40, 23, 3, 2, fog_ref.params(**p))
    share = 1.0 - lit.mean()
    print("occluded share of the 40 x 23 records %.3f" % share)
    assert 0.05 <= share <= 0.95
    assert equal(rec, want_rec) and rec.shape == (23, 40, 4)
    assert images["mean"][3] == 4 and images["upsampled"][3] == 4 and images["upsampled"][0].shape == (90, 160, 4)
    before = everything(st) + [rec]
    got = {}
    for source in ("mean", "denoised", "upsampled"):  # (the last: 160 x 90 from 40 x 23, the guide as first-hit records)
        st.fog(source, upsample=True)
        got[source] = st.fog_download()
        colour = fog_ref.source_colour(images[source][0], images[source][1])
        assert equal(got[source], want_image(images, source, rec, 2, p)), source
        assert got[source].shape == images[source][0].shape and (got[source][..., 3] == 1).all() and not equal(got[source][..., :3], colour)
    assert not equal(got["mean"], got["denoised"])
    st.fog("denoised", sample_total=0, upsample=True)  # sample_total is ignored for all sources but the mean
    assert equal(st.fog_download(), got["denoised"])
    mine = DeviceArray(np.zeros((45, 80, 4), F))  # into a caller's buffer, which the later passes then read
    st.fog("mean", out_ptr=mine.data_ptr(), upsample=True)
    st.synchronize()
    assert equal(mine.numpy(), got["mean"]) and equal(st.fog_download(), got["mean"])
    # rsrt_fog_apply itself goes on refusing records of another size, and leaves the image
    st.fog("mean", upsample=True)
    raises(INVALID, lambda: st.fog("mean"))
    assert equal(st.fog_download(), got["mean"])
    for a, b in zip(before, everything(st) + [st.download_fog()]):  # nothing else was written
        assert equal(a, b)


@pytest.mark.parametrize("w,h,W,H", [(1, 1, 1, 1), (34, 3, 67, 5), (2, 2, 7, 7), (21, 9, 21, 9), (512, 260, 1024, 520)])
def test_ratios_small_ragged_and_large_frames(w, h, W, H):
    """1 x 1; 67 x 5 from 34 x 3: a ragged last block and ratios just under 2; 7 x 7 from 2 x 2: ratio 3.5; equal sizes: the 3 x 3
    tent; 1024 x 520 = 532480 pixels: more than the fog march's grid has lanes in one pass (524288 on 256 CUs), 2080 blocks here."""
    st = R.State.new(loaded("default")[0], util.small_env(), W, H)
    try:
        st.render_samples(1, aov=True)
        p = dict(BASE, steps=2, density=0.2)
        st.render_fog(1, 0, size=(w, h), **p)
        rec, g = st.download_fog(), st.download_aov()
        assert rec.shape == (h, w, 4) and rec[..., 3].all()
        st.fog("mean", upsample=True)
        got = st.fog_download()
        want = ref.rebuild(fog_ref.source_colour(st.download(), 1), rec, 1, g, 1, constants(p))[0]
        assert equal(got, want) and np.isfinite(got).all()
        if (w, h) == (W, H) and w > 1:  # not the identity
            st.fog("mean")
            assert not equal(st.fog_download(), got)
    finally:
        st.close()


def test_a_clear_medium_is_the_source(rendered):
    st, images, rec, p = rendered
    try:
        st.clear_fog()
        st.render_fog(2, 3, size=(40, 23), **dict(p, density=0.0))
        clear = st.download_fog()
        assert not clear[..., :3].any() and (clear[..., 3] == 2).all()
        for source in ("mean", "denoised", "upsampled"):
            img, total = images[source][:2]
            st.fog(source, upsample=True)
            assert equal(st.fog_download()[..., :3], fog_ref.source_colour(img, total)), source
    finally:
        st.clear_fog()
        st.render_fog(2, 3, size=(40, 23), **p)
    assert equal(st.download_fog(), rec)


def test_the_rebuilt_image_is_a_source_of_the_later_passes(rendered):
    st, images, rec, p = rendered
    cam = dof_ref.Camera.from_record(st.camera)
    e = 1.7
    for source in ("mean", "upsampled"):  # the lens reads the AOV buffer for the first, the guide for the second
        img, total, g, T = images[source]
        st.fog(source, upsample=True)
        fog = st.fog_download()
        assert equal(fog, want_image(images, source, rec, 2, p))
        shown = st.display_exposed_srgb8("fog", e)
        assert shown.shape == fog.shape and np.array_equal(shown, exposure_ref.display(fog, 1, e))
        st.depth_of_field("fog", 3.0, 0.15, 5)
        lens = st.dof_download()
        assert util.same_bits_or_nan(lens, dof_ref.dof(fog, 1, g, cam, 3.0, 0.15, 5)[0]) and not equal(lens, fog), source
    st.exposure_meter("fog")
    assert np.array_equal(st.exposure_download()[0], exposure_ref.histogram(fog, 1))
    st.exposure_meter()  # (the fixture's histogram)


def test_refusals_leave_records_and_image_as_they_were(rendered):
    st, images, rec, p = rendered
    st.fog("mean", upsample=True)
    fog = st.fog_download()
    before = everything(st) + [rec, fog]
    L = st._L
    good = R.state.FogParams.of(**p)
    apply = lambda s, n, nf, nr, prm=C.byref(good), out=None: st._check(L.rsrt_fog_apply_upsampled(st._ctx, s, n, nf, nr, prm, out, None),  # noqa: E731
                                                                         "rsrt_fog_apply_upsampled")
    apply(0, 4, 2, 4)  # (the call the refusals below vary)
    assert equal(st.fog_download(), fog)
    for source in (4, 5, 6, 7):
        raises(INVALID, lambda: apply(source, 4, 2, 4))
    raises(INVALID, lambda: apply(0, 4, 2, 4, None))                          # NULL params
    for kw in ({"density": -1.0}, {"density": float("nan")}, {"albedo": 1.5}, {"anisotropy": 0.99}, {"light_dir": (0.0, 2.0, 0.0)}, {"light_irradiance": -1.0},
               {"ambient": float("inf")}, {"max_distance": 0.0}, {"steps": 0}, {"steps": 65}, {"flags": 2}):
        bad = R.state.FogParams.of(**dict(p, **kw))
        raises(INVALID, lambda: apply(0, 4, 2, 4, C.byref(bad)))
    raises(INVALID, lambda: apply(0, 4, 0, 4))                                # fog_sample_total 0
    raises(INVALID, lambda: apply(0, 4, 2, 0))                                # record_sample_total 0
    raises(INVALID, lambda: apply(0, 0, 2, 4))                                # sample_total 0 under the mean
    raises(INVALID, lambda: apply(0, 4, 2, 4, C.byref(good), C.c_void_p(8)))  # a misaligned output
    st.set_partition(0, 2)  # whole frame only
    try:
        raises(INVALID, lambda: apply(0, 4, 2, 4))
    finally:
        st.set_partition(0, 1)
    for a, b in zip(before, everything(st) + [st.download_fog(), st.fog_download()]):
        assert equal(a, b)
    # fog records wider or taller than the source; the upsampled image (160 x 90) takes what the mean (80 x 45) refuses
    try:
        for size in ((81, 23), (40, 46), (160, 90)):
            st.render_fog(1, 0, size=size, **p)
            raises(INVALID, lambda: st.fog("mean", upsample=True))
            assert equal(st.fog_download(), fog)
        st.fog("upsampled", upsample=True)
        assert st.fog_download().shape == (90, 160, 4)
    finally:
        st.render_fog(2, 3, size=(40, 23), **p)
    assert equal(st.download_fog(), rec)
    st.fog("mean", upsample=True)
    assert equal(st.fog_download(), fog)
    # NOT_READY: no records, no first-hit records, no source, no remembered parameters; first-hit records of another size
    bare = R.State()
    try:
        raises(NOT_READY, lambda: bare._check(L.rsrt_fog_apply_upsampled(bare._ctx, 0, 1, 1, 1, C.byref(good), None, None), "rsrt_fog_apply_upsampled"))
    finally:
        bare.close()
    fresh = R.State.new(loaded("default")[0], util.small_env(), 16, 8)
    try:
        fresh.render_samples(1)
        with pytest.raises(R.RsrtError):
            fresh.fog("mean", upsample=True)                                   # no parameters remembered: the state's own refusal
        fresh.fog_params = good
        raises(NOT_READY, lambda: fresh.fog("mean", upsample=True, fog_sample_total=1, record_sample_total=1))  # no fog records
        fresh.fog_params = None
        fresh.render_fog(1, 0, size=(8, 4), **dict(BASE, steps=2))
        raises(NOT_READY, lambda: fresh.fog("mean", upsample=True, record_sample_total=1))      # no AOV buffer
        raises(NOT_READY, lambda: fresh.fog("upsampled", upsample=True, record_sample_total=1))  # no upsampled image
        raises(NOT_READY, lambda: fresh.fog_download())                        # ... and none of them left a fog image
        other = DeviceArray(np.zeros((8, 8, 8), F))
        fresh.bind_aov(other.data_ptr(), 8, 8)                                 # first-hit records of another size than the source
        raises(INVALID, lambda: fresh.fog("mean", upsample=True, record_sample_total=1))
        fresh.bind_aov(None, 0, 0)
        fresh.render_aov(0, 1)
        raises(NOT_READY, lambda: fresh.fog("denoised", upsample=True))        # no such source
        fresh.fog("mean", upsample=True)
        assert fresh.fog_download().shape == (8, 16, 4)
        fresh.fog_reset()
        raises(NOT_READY, lambda: fresh.exposure_meter("fog"))
    finally:
        fresh.close()


def test_cpp_state_rebuilds_like_the_python_state(tmp_path):
    import test_fog_upsample
    exe = test_fog_upsample.build_cpp_demo(tmp_path)
    w, h, samples, steps, density = 64, 37, 3, 6, 0.2
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", str(samples), str(steps), str(density)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        st.render_samples(samples, aov=True)
        st.render_fog(1, 0, size=(32, 19), steps=steps, density=density, ambient=0.05, light_dir=(0.0, 0.6, -0.8), light_irradiance=(4.0, 3.0, 2.0))
        st.render_fog(samples - 1, size=(32, 19))
        rec = st.download_fog()
        assert lines[0] == ["records", str(samples), str(rec.size), "%016x" % fnv1a(rec.tobytes())]
        assert lines[1] == ["plain", "refused"]
        st.fog(upsample=True)
        img = st.fog_download()
        assert lines[2] == ["fog", str(img.size), "%016x" % fnv1a(img.tobytes())]
        st.depth_of_field("fog")
        assert lines[3] == ["lens", "%016x" % fnv1a(st.dof_download().tobytes())]
        shown = st.display_exposed_srgb8("fog", 1.5)
        assert lines[4] == ["display", str(shown.size), "%016x" % fnv1a(shown.tobytes())]
    finally:
        st.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_half_size_fog_beats_full_size_fog_of_the_same_cost():
    """house 96 x 54, BASE at density 0.15, 8 steps, jitter on.  The truth: 64 full-size fog samples from index 100.  A: 48 x 27 records
    of 16 samples from index 0, rebuilt with 16 AOV samples; B: full-size records of 4 samples (the same number of march rays); C: the
    plain tent upsample of A's records, without the demodulation (numpy).  The metric is the RMSE of 0.5 T + I over all pixels and
    channels — the fog image of a mid-grey source; A's (I, T) are the restatement's, which the device image is first shown to equal bit
    for bit.  Measured on an MI355X: A 0.0150, B 0.0332, C 0.0318 (ratios 0.451 and 0.471)."""
    W, H, w, h = 96, 54, 48, 27
    p = dict(BASE, density=0.15, steps=8, flags=1)
    metric = lambda r: 0.5 * np.asarray(r, np.float64)[..., 3:4] + np.asarray(r, np.float64)[..., :3]  # noqa: E731
    sc, st = state("house", W, H)
    try:
        st.render_fog(64, 100, **p)
        truth = metric(st.download_fog() / F(64))
        st.clear_fog()
        st.render_fog(4, 0, **p)
        b = metric(st.download_fog() / F(4))
        st.render_samples(16, aov=True)
        st.render_fog(16, 0, size=(w, h), **p)
        low = st.download_fog()
        st.fog("mean", upsample=True)
        image, r = ref.rebuild(fog_ref.source_colour(st.download(), 16), low, 16, st.download_aov(), 16, constants(p))
        assert equal(st.fog_download(), image)
        a, c = metric(r), metric(ref.tent_raw(low, 16, H, W))
        err_a, err_b, err_c = rmse(a, truth), rmse(b, truth), rmse(c, truth)
        print("RMSE of 0.5 T + I against 64 full-size samples: A (half size, 16 samples, rebuilt) %.4f, B (full size, 4 samples) %.4f, "
              "C (A's records, plain tent) %.4f; A / B %.3f, A / C %.3f" % (err_a, err_b, err_c, err_a / err_b, err_a / err_c))
        assert err_a < 0.75 * err_b and err_a < 0.75 * err_c
    finally:
        st.close()
