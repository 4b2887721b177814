"""The finished display on the GPU (rsrt_display_finished_srgb8): the device's bytes against the numpy restatement (tests/finish_ref.py)
applied to the downloaded source image and the downloaded grid, bloom image and LUT, byte for byte — both kernel variants, both flags,
grain and dither on, two seeds, frames of one pixel, exactly one tile, one past a tile both ways and a real render, a source of another
size than the accumulator, local exposure, bloom and a LUT all at once; the identity with the colour display; every refusal and what it
leaves; the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import colour_ref
import finish_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_exposure_gpu import denoised, fnv1a, raises, upsampled
from test_finish import colour_params, finish_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
# (h, w): one pixel; two; exactly one 32 x 8 tile; one past a tile both ways, so that every tile has a clamped ring side; 67 x 5
FRAMES = [(1, 1), (1, 2), (8, 32), (9, 33), (5, 67)]
# both kernel variants (sharpness 0 / > 0), both flags, grain and dither on and off, two seeds
SETTINGS = [dict(sharpness=0.0, grain=0.0, dither=1.0, seed=0, flags=0),
            dict(sharpness=0.0, grain=1.0, dither=1.0, seed=0x9e3779b9, flags=finish_ref.NOISE_AWARE),
            dict(sharpness=0.5, grain=0.0, dither=0.0, seed=0, flags=0),
            dict(sharpness=0.5, grain=0.25, dither=1.0, seed=0, flags=0),
            dict(sharpness=1.0, grain=0.25, dither=1.0, seed=0x9e3779b9, flags=0),
            dict(sharpness=1.0, grain=1.0, dither=1.0, seed=0, flags=finish_ref.NOISE_AWARE),
            dict(sharpness=1.0, grain=0.0, dither=0.0, seed=0x9e3779b9, flags=finish_ref.NOISE_AWARE)]
ZERO = dict(sharpness=0.0, grain=0.0, dither=0.0)
LOCAL = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}


def shown(st, source, exposure, kw, total=None, **chain):
    return st.display_finished_srgb8(source, exposure, sample_total=total, noise_aware=bool(kw.get("flags", 0)),
                                     **{k: v for k, v in kw.items() if k != "flags"}, **chain)


def check_everything_on(st, img, total, source, exposure=0.37, white=(1.3, 0.95, 0.6), settings=SETTINGS):
    """Local exposure, bloom and a 17^3 LUT at once on `source`, whose downloaded image is img: the device's bytes against the restatement
    over the downloaded grid, bloom image and LUT; then each of the three alone off."""
    n = None if source != "mean" else total
    st.bloom(source, exposure, 3, sample_total=n)
    st.local_exposure(source, 8, sample_total=n)
    st.colour_lut(*colour_ref.CDLS["warm"], size=17)
    b, (grid, cell), lut = st.bloom_download(), st.local_exposure_download(), st.colour_lut_download()
    assert cell == 8 and lut.shape == (17, 17, 17, 3)
    gain = local_ref.gains(img, total, exposure, grid, cell, **LOCAL)
    for kw in settings:
        got = shown(st, source, exposure, kw, n, white=white, lut_strength=0.5, bloom_intensity=0.5, **LOCAL)
        assert got.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, finish_ref.display(img, total, exposure, white, lut, 0.5, gain, 0.5, b, **kw)), (source, kw)
        got = shown(st, source, exposure, kw, n, white=white, lut_strength=0.0)
        assert np.array_equal(got, finish_ref.display(img, total, exposure, white, **kw)), (source, kw)
    # with all three parameters 0: the colour display's bytes for the same arguments
    for chain in ({"white": white, "lut_strength": 0.5, "bloom_intensity": 0.5, **LOCAL}, {"white": (1.0, 1.0, 1.0), "lut_strength": 0.0}, {"white": white, "lut_strength": 1.0}):
        assert np.array_equal(shown(st, source, exposure, ZERO, n, **chain), st.display_colour_srgb8(source, exposure, sample_total=n, **chain)), chain
        assert np.array_equal(shown(st, source, exposure, dict(ZERO, seed=5, flags=1), n, **chain), st.display_colour_srgb8(source, exposure, sample_total=n, **chain))


@pytest.mark.parametrize("h,w", FRAMES)
def test_synthetic_frames_equal_the_numpy_restatement_byte_for_byte(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=2000 * h + w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        check_everything_on(st, sums, 3, "mean")
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


@pytest.fixture(scope="module")
def house():
    """House at 96 x 54 and 4 spp with the denoised and the upsampled (192 x 108) image."""
    w, h = 96, 54
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)
    yield st, {"mean": (st.download(), 4), "upsampled": (upsampled(st), 1)}
    st.close()


def held(st):
    return [st.download(), st.download_aov(), st.download_guide(), denoised(st), upsampled(st)]


def test_a_render_and_a_source_of_another_size(house):
    st, images = house
    before = held(st)
    assert images["mean"][0].shape == (54, 96, 4) and images["upsampled"][0].shape == (108, 192, 4)
    for source, (img, total) in images.items():
        check_everything_on(st, img, total, source, exposure=1.5, settings=SETTINGS[1::2])
    grid, b, lut = st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()
    for kw in SETTINGS[3:5]:  # the same seed gives the same bytes, another does not
        a = shown(st, "mean", 1.5, kw)
        assert np.array_equal(a, shown(st, "mean", 1.5, kw)) and not np.array_equal(a, shown(st, "mean", 1.5, dict(kw, seed=kw["seed"] + 1)))
    kw = SETTINGS[3]  # a seed of any size or sign: its low 32 bits (a long-running frame counter wraps, it is not refused)
    assert np.array_equal(shown(st, "mean", 1.5, dict(kw, seed=3)), shown(st, "mean", 1.5, dict(kw, seed=(1 << 32) + 3)))
    assert np.array_equal(shown(st, "mean", 1.5, dict(kw, seed=-1)), shown(st, "mean", 1.5, dict(kw, seed=0xFFFFFFFF)))
    soft, sharp = shown(st, "upsampled", 1.5, dict(ZERO)), shown(st, "upsampled", 1.5, dict(ZERO, sharpness=1.0))
    lap = lambda g: np.abs(4.0 * g[1:-1, 1:-1, :3] - g[:-2, 1:-1, :3] - g[2:, 1:-1, :3] - g[1:-1, :-2, :3] - g[1:-1, 2:, :3]).mean()  # noqa: E731
    assert lap(sharp.astype(np.float64)) > lap(soft.astype(np.float64))  # sharper
    for a, c in zip(before + [grid, b, lut], held(st) + [st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()]):
        assert util.same_bits_or_nan(a, c)  # nothing the context holds was written


def test_refusals_return_their_status_and_leave_everything(house):
    st, images = house
    img, total = images["mean"]
    L, S = st._L, R.state
    st.bloom("mean", 1.5, 3)
    st.local_exposure("mean", 8)
    st.colour_lut(*colour_ref.CDLS["crush"], size=3)
    everything = lambda: held(st) + [st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()]  # noqa: E731
    before = everything()
    fp, cp = finish_params, colour_params
    buf = np.full((54, 96, 4), 7, np.uint8)
    lp = lambda: S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)  # noqa: E731
    show = lambda source, n, e, c, f, local=None, i=0.0, b=buf, nb=None: st._check(  # noqa: E731
        L.rsrt_display_finished_srgb8(st._ctx, source, n, e, C.byref(local) if local is not None else None, i, C.byref(c) if c is not None else None,
                                      C.byref(f) if f is not None else None, S._p(b) if b is not None else None, buf.size if nb is None else nb),
        "rsrt_display_finished_srgb8")
    show(0, 4, 1.5, cp((2, 1, 0.5), 1.0), fp(), local=lp(), i=0.5)
    good = buf.copy()
    assert np.array_equal(good, finish_ref.display(img, total, 1.5, (2, 1, 0.5), before[-1], 1.0, local_ref.gains(img, total, 1.5, before[-3], 8), 0.5, before[-2]))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None))  # a NULL finish
    nan, inf = float("nan"), float("inf")
    for kw in [{k: v} for k in ("sharpness", "grain", "dither") for v in (-0.001, 1.001, nan, inf)] + [{"flags": 2}, {"flags": 0x80000001}]:  # each bad field
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(**kw)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(), nb=buf.size - 4))  # a wrong n_bytes, a NULL buffer
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(), b=None))
    raises(INVALID, lambda: show(9, 4, 1.5, cp(), fp()))  # source 9 unknown
    raises(INVALID, lambda: show(0, 0, 1.5, cp(), fp()))  # what the colour display refuses: sample_total 0, a bad exposure, colour, local, intensity
    raises(INVALID, lambda: show(0, 4, 0.0, cp(), fp()))
    raises(INVALID, lambda: show(0, 4, 1.5, None, fp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(strength=1.5), fp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(), local=S.LocalParams(-0.1, 0.5, 0.18, 4.0, 0, 0)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(), i=-0.5))
    raises(NOT_READY, lambda: show(2, 4, 1.5, cp(), fp()))  # no temporal image in this context
    st.set_partition(0, 2)  # a partition set
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp()))
    raises(INVALID, lambda: st.display_finished_srgb8("mean", 1.5))
    st.set_partition(0, 1)
    assert np.array_equal(buf, good)  # no refused call wrote the host buffer
    for a, c in zip(before, everything()):
        assert util.same_bits_or_nan(a, c)
    # a missing grid, bloom image or LUT: needed only when asked for
    st.local_exposure_reset()
    st.bloom_reset()
    st.colour_lut_reset()
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), fp(), local=lp()))
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), fp(), i=0.5))
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(strength=0.5), fp()))
    assert np.array_equal(buf, good)
    show(0, 4, 1.5, cp(), fp())
    assert np.array_equal(buf, finish_ref.display(img, total, 1.5))
    st.local_exposure("upsampled", 8)
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), fp(), local=lp()))  # a grid of another size than the source
    for a, c in zip(before[:5], held(st)):
        assert util.same_bits_or_nan(a, c)


def test_cpp_state_finishes_like_the_python_state(tmp_path):
    import test_finish
    exe = test_finish.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", "4", "17"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        st.colour_lut((1.1, 1.0, 1.0), None, None, 1.25, size=17)
        lut = st.colour_lut_download()
        img = st.download()
        got = st.display_finished_srgb8()
        assert np.array_equal(got, finish_ref.display(img, 4, e, lut=lut, strength=1.0))
        assert next(f for f in lines if f[0] == "default")[1:] == [str(got.size), "%016x" % fnv1a(got.tobytes())]
        for seed in (7, 8):
            got = st.display_finished_srgb8(sharpness=1.0, grain=0.5, dither=1.0, seed=seed, noise_aware=True)
            assert np.array_equal(got, finish_ref.display(img, 4, e, lut=lut, strength=1.0, sharpness=1.0, grain=0.5, dither=1.0, seed=seed, flags=1))
            assert next(f for f in lines if f[0] == "seed%d" % seed)[1:] == [str(got.size), "%016x" % fnv1a(got.tobytes())]
        assert ["off", "yes"] in lines and ["again", "yes"] in lines and ["defaults", "%08x" % (128 << 16 | 1), "0"] in lines
    finally:
        st.close()
