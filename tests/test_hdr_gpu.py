"""The HDR display on the GPU (rsrt_display_hdr): the device's words and light levels against the numpy restatement (tests/hdr_ref.py)
applied to the downloaded source image and the downloaded grid and bloom image, word for word — all four kernel variants (both
encodings, with and without the levels), dither on and off at two seeds, frames of one pixel, exactly one tile, one past a tile both
ways and a real render, a source of another size than the accumulator, local exposure, bloom and a white point at once and each off in
turn; the linear colour it shares with the colour display; every refusal and what it leaves; the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import colour_ref
import hdr_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_exposure_gpu import denoised, fnv1a, raises, upsampled
from test_hdr import colour_params, hdr_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
PQ10, SCRGB16F = hdr_ref.PQ10, hdr_ref.SCRGB16F
# (h, w): one pixel; two; exactly one 32 x 8 tile; one past a tile both ways (four workgroups, three of them mostly outside); 67 x 5
FRAMES = [(1, 1), (1, 2), (8, 32), (9, 33), (5, 67)]
# both encodings, dither off and on, two seeds, the defaults and two corners of the curve
SETTINGS = [dict(encoding=PQ10),
            dict(encoding=PQ10, dither=1.0, seed=0),
            dict(encoding=PQ10, dither=0.5, seed=0x9e3779b9, paper_white=100.0, peak=100.0, knee=0.95),
            dict(encoding=SCRGB16F),
            dict(encoding=SCRGB16F, paper_white=80.0, peak=10000.0, knee=0.0),
            dict(encoding=PQ10, dither=1.0, seed=0x9e3779b9, paper_white=1.0, peak=10000.0, knee=0.25)]
LOCAL = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}
NAMES = {PQ10: "pq10", SCRGB16F: "scrgb16f"}


def shown(st, source, exposure, kw, total=None, levels=True, **chain):
    """State.display_hdr with hdr_ref's names: the words as unsigned integers (uint32 [h, w] or uint16 [h, w, 4]) and the levels."""
    kw = dict(kw, encoding=NAMES[kw.get("encoding", PQ10)])
    got = st.display_hdr(source, exposure, sample_total=total, levels=levels, **kw, **chain)
    img, lv = got if levels else (got, None)
    assert img.dtype == (np.uint32 if kw["encoding"] == "pq10" else np.float16)
    return (img if kw["encoding"] == "pq10" else img.view(np.uint16)), lv


def check_everything_on(st, img, total, source, exposure=0.37, white=(1.3, 0.95, 0.6), settings=SETTINGS):
    """Local exposure (cell 8), bloom (3 levels) and a white point at once on `source`, whose downloaded image is img: the device's words
    and levels against the restatement over the downloaded grid and bloom image; then each of the three off in turn."""
    n = None if source != "mean" else total
    st.bloom(source, exposure, 3, sample_total=n)
    st.local_exposure(source, 8, sample_total=n)
    b, (grid, cell) = st.bloom_download(), st.local_exposure_download()
    assert cell == 8
    gain = local_ref.gains(img, total, exposure, grid, cell, **LOCAL)
    for kw in settings:
        for wh, g, intensity in ((white, gain, 0.5), (white, None, 0.5), (white, gain, 0.0), ((1.0, 1.0, 1.0), gain, 0.5), ((1.0, 1.0, 1.0), None, 0.0)):
            chain = dict(white=wh, bloom_intensity=intensity, **(LOCAL if g is not None else {}))
            got, lv = shown(st, source, exposure, kw, n, **chain)
            want, want_lv = hdr_ref.display(img, total, exposure, wh, g, intensity, b, **kw)
            assert got.shape == want.shape and np.array_equal(got, want), (source, kw, intensity, g is None)
            assert lv == want_lv, (source, kw, lv, want_lv)
            assert np.array_equal(shown(st, source, exposure, kw, n, levels=False, **chain)[0], got)  # the variant without the levels: the same words


@pytest.mark.parametrize("h,w", FRAMES)
def test_synthetic_frames_equal_the_numpy_restatement_word_for_word(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=2000 * h + w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        check_everything_on(st, sums, 3, "mean")
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


def test_the_levels_of_272_workgroups_and_of_a_sum_past_32_bits():
    """136 x 512: 17 x 16 = 272 workgroups, so rt_hdr_levels_kernel's loop over the pairs takes a second, partial trip (lanes 0 .. 15).
    (a) every pixel at a peak of 10000 cd/m^2: sum q = 69632 x 640000 = 4.46e10, which carries out of the low half of the 64-bit sum on
    its way down the shuffles; (b) tests/frame_chain.py's lognormal frame at the default settings: pairs that differ from workgroup to
    workgroup, and the frame's only pixel at the peak in workgroup 271, which only the second trip reads.  No local exposure, no bloom."""
    import frame_chain as FC
    bright, (lognormal, (y, x)) = FC.levels_bright(), FC.levels_lognormal()
    h, w = FC.LEVELS_H, FC.LEVELS_W
    st = R.State()
    devs = []  # (both frames' device memory lives until the context is closed)
    try:
        for sums, total, hdr in ((bright, 3, FC.LEVELS_BRIGHT), (lognormal, 1, {})):
            dev = DeviceArray(sums)
            devs.append(dev)
            st.bind_accumulator(dev.data_ptr(), w, h)
            for enc in (PQ10, SCRGB16F):
                kw = dict(hdr, encoding=enc)
                want, want_lv = hdr_ref.display(sums, total, 1.0, **kw)
                if sums is bright:
                    assert want_lv["sum_q"] > 2 ** 32 and want_lv["max_fall"] == want_lv["max_cll"] == 10000.0
                else:
                    assert FC.workgroup_of(y, x) == 271 and want_lv["max_q"] == int(hdr_ref.level_q(hdr_ref.nits_of(hdr_ref.linear(sums, 1, 1.0), encoding=enc))[y, x])
                got, lv = shown(st, "mean", 1.0, kw, total)
                assert got.shape == want.shape and np.array_equal(got, want), kw
                assert lv == want_lv, (kw, lv, want_lv)
                assert np.array_equal(shown(st, "mean", 1.0, kw, total, levels=False)[0], got)  # the variant without the levels: the same words
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
    grid, b = st.local_exposure_download()[0], st.bloom_download()
    kw = SETTINGS[1]  # the same seed gives the same words, another does not; a seed of any size or sign: its low 32 bits
    a = shown(st, "mean", 1.5, kw)[0]
    assert np.array_equal(a, shown(st, "mean", 1.5, kw)[0]) and not np.array_equal(a, shown(st, "mean", 1.5, dict(kw, seed=1))[0])
    assert np.array_equal(shown(st, "mean", 1.5, dict(kw, seed=3))[0], shown(st, "mean", 1.5, dict(kw, seed=(1 << 32) + 3))[0])
    assert np.array_equal(shown(st, "mean", 1.5, dict(kw, seed=-1))[0], shown(st, "mean", 1.5, dict(kw, seed=0xFFFFFFFF))[0])
    words, lv = st.display_hdr("mean", 1.5, levels=True)  # the defaults: PQ10, 203 / 1000 cd/m^2, no dither
    codes = R.state.hdr_unpack_pq10(words)
    assert codes.shape == (54, 96, 3) and codes.max() <= 769 and (words >> 30 == 3).all() and 0 < lv["max_fall"] <= lv["max_cll"] <= 1000.0
    for a, c in zip(before + [grid, b], held(st) + [st.local_exposure_download()[0], st.bloom_download()]):
        assert util.same_bits_or_nan(a, c)  # nothing the context holds was written


def test_the_linear_colour_is_the_colour_displays(house, monkeypatch):
    """display_hdr and display_colour_srgb8 with the same arguments over the same downloaded inputs: both device results equal their
    restatements, and the two restatements start from the same linear colour — hdr_ref's step 1 is what colour_ref hands its tone map."""
    st, images = house
    img, total = images["mean"]
    exposure, white, intensity = 1.5, (1.3, 0.95, 0.6), 0.5
    st.bloom("mean", exposure, 3)
    st.local_exposure("mean", 8)
    b, (grid, cell) = st.bloom_download(), st.local_exposure_download()
    gain = local_ref.gains(img, total, exposure, grid, cell, **LOCAL)
    seen = []
    tone_map = colour_ref.tone_map
    monkeypatch.setattr(colour_ref, "tone_map", lambda hdr: seen.append(hdr.copy()) or tone_map(hdr))
    want_bytes = colour_ref.display(img, total, exposure, white, None, 0.0, gain, intensity, b)
    assert len(seen) == 1 and util.same_bits_or_nan(hdr_ref.linear(img, total, exposure, white, gain, intensity, b), seen[0])
    chain = dict(white=white, bloom_intensity=intensity, **LOCAL)
    assert np.array_equal(st.display_colour_srgb8("mean", exposure, lut_strength=0.0, **chain), want_bytes)
    for kw in (SETTINGS[0], SETTINGS[3]):
        assert np.array_equal(shown(st, "mean", exposure, kw, **chain)[0], hdr_ref.display(img, total, exposure, white, gain, intensity, b, **kw)[0])


def test_refusals_return_their_status_and_leave_everything(house):
    st, images = house
    img, total = images["mean"]
    L, S = st._L, R.state
    st.bloom("mean", 1.5, 3)
    st.local_exposure("mean", 8)
    st.colour_lut(*colour_ref.CDLS["crush"], size=3)
    everything = lambda: held(st) + [st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()]  # noqa: E731
    before = everything()
    hp, cp = hdr_params, colour_params
    buf = np.full((54, 96), 0x07070707, np.uint32)
    wide = np.full((54, 96, 4), 0x0707, np.uint16)
    lv = S.HdrLevels(7, 7, 7.0, 7.0, 7)
    lp = lambda: S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)  # noqa: E731
    show = lambda source, n, e, c, h, local=None, i=0.0, b=buf, nb=None, levels=lv: st._check(  # noqa: E731
        L.rsrt_display_hdr(st._ctx, source, n, e, C.byref(local) if local is not None else None, i, C.byref(c) if c is not None else None,
                           C.byref(h) if h is not None else None, S._p(b) if b is not None else None, (b.nbytes if b is not None else buf.nbytes) if nb is None else nb,
                           C.byref(levels) if levels is not None else None), "rsrt_display_hdr")
    show(0, 4, 1.5, cp((2, 1, 0.5)), hp(), local=lp(), i=0.5)
    good, good_lv = buf.copy(), (lv.sum_q, lv.max_q, lv.max_cll, lv.max_fall)
    want, want_lv = hdr_ref.display(img, total, 1.5, (2, 1, 0.5), local_ref.gains(img, total, 1.5, before[-3], 8), 0.5, before[-2])
    assert np.array_equal(good, want) and good_lv == (want_lv["sum_q"], want_lv["max_q"], want_lv["max_cll"], want_lv["max_fall"])
    unwritten = lambda: np.array_equal(buf, good) and (wide == 0x0707).all() and (lv.sum_q, lv.max_q, lv.max_cll, lv.max_fall) == good_lv  # noqa: E731
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None))  # a NULL hdr
    nan, inf = float("nan"), float("inf")
    bad = [{"paper_white": v} for v in (0.5, 10001.0, nan, inf)] + [{"peak": v} for v in (202.0, 10001.0, nan, inf)] + [{"knee": v} for v in (-0.001, 0.96, nan)] + \
          [{"dither": v} for v in (-0.001, 1.001, nan)] + [{"encoding": 2}, {"flags": 1}, {"encoding": SCRGB16F, "dither": 0.5}]
    for kw in bad:  # each bad field
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(**kw), b=wide if kw.get("encoding") == SCRGB16F else buf))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(strength=0.5), hp()))  # the LUT does not apply, though the context holds one
    raises(INVALID, lambda: show(0, 4, 1.5, cp(strength=1.0), hp(encoding=SCRGB16F), b=wide))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), nb=buf.nbytes - 4))  # a wrong n_bytes: the other encoding's, one word short; a NULL buffer
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), nb=buf.nbytes * 2))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(encoding=SCRGB16F), b=wide, nb=buf.nbytes))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), b=None))
    raises(INVALID, lambda: show(9, 4, 1.5, cp(), hp()))  # source 9 unknown (and 7: no pass writes an HDR image)
    raises(INVALID, lambda: show(7, 4, 1.5, cp(), hp()))
    raises(INVALID, lambda: show(0, 0, 1.5, cp(), hp()))  # what the colour display refuses: sample_total 0, a bad exposure, colour, local, intensity
    raises(INVALID, lambda: show(0, 4, 0.0, cp(), hp()))
    raises(INVALID, lambda: show(0, 4, 1.5, None, hp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp((0.0, 1.0, 1.0)), hp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), local=S.LocalParams(-0.1, 0.5, 0.18, 4.0, 0, 0)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), i=-0.5))
    raises(NOT_READY, lambda: show(2, 4, 1.5, cp(), hp()))  # no temporal image in this context
    st.set_partition(0, 2)  # a partition set
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp()))
    raises(INVALID, lambda: st.display_hdr("mean", 1.5))
    st.set_partition(0, 1)
    assert unwritten()  # no refused call wrote the host buffer or the levels
    for a, c in zip(before, everything()):
        assert util.same_bits_or_nan(a, c)
    # a missing grid or bloom image: needed only when asked for
    st.local_exposure_reset()
    st.bloom_reset()
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), hp(), local=lp()))
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), hp(), i=0.5))
    assert unwritten()
    show(0, 4, 1.5, cp(), hp(), levels=None)
    assert np.array_equal(buf, hdr_ref.display(img, total, 1.5)[0]) and (lv.sum_q, lv.max_q) == good_lv[:2]  # (NULL levels: not written)
    show(0, 4, 1.5, cp(), hp(encoding=SCRGB16F), b=wide)
    assert np.array_equal(wide, hdr_ref.display(img, total, 1.5, encoding=SCRGB16F)[0])
    st.local_exposure("upsampled", 8)
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), local=lp()))  # a grid of another size than the source
    for a, c in zip(before[:5], held(st)):
        assert util.same_bits_or_nan(a, c)


def test_cpp_state_shows_hdr_like_the_python_state(tmp_path):
    import test_hdr
    exe = test_hdr.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        img = st.download()
        for name, kw in (("pq10", {}), ("dithered", {"dither": 1.0, "seed": 7}), ("scrgb16f", {"encoding": "scrgb16f"})):
            got, lv = st.display_hdr(levels=True, **kw)
            want, want_lv = hdr_ref.display(img, 4, e, **dict(kw, encoding=hdr_ref.ENCODINGS[kw.get("encoding", "pq10")]))
            assert np.array_equal(got.view(want.dtype), want) and lv == want_lv
            fields = next(f for f in lines if f[0] == name)
            assert fields[1:5] == [str(got.nbytes), "%016x" % fnv1a(got.tobytes()), str(lv["max_q"]), str(lv["sum_q"])]
            assert (np.float32(fields[5]), np.float32(fields[6])) == (np.float32(lv["max_cll"]), np.float32(lv["max_fall"]))
        assert ["without", "yes"] in lines and ["defaults", "203", "1000", "0.5", "0", "0", "0", "0"] in lines
    finally:
        st.close()
