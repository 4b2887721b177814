"""The video pass on the GPU (rsrt_display_video): the device's frames and light levels against the numpy restatement (tests/video_ref.py)
applied to the downloaded source image and the downloaded grid, bloom image and LUT, byte for byte — every kernel variant (both
standards, both depths, the three sitings, with and without the levels), both layouts and ranges, dither off and on, frames of one
pixel, one quad cut by the edge either way, exactly one tile, one past a tile both ways and a real render with its denoised and its
upsampled image; local exposure, bloom, a white point and a LUT at once and each off in turn; the levels against display_hdr's; every
refusal and what it leaves; the C++ State and tools/render_y4m.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref
import hdr_ref
import local_ref
import util
import video_ref as V
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_exposure_gpu import denoised, fnv1a, raises, upsampled
from test_video import COMBOS, HDR, colour_params, hdr_params, read_y4m, video_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
# (h, w): one pixel; a quad cut by the right edge, by the lower; exactly one 32 x 8 tile; one past a tile both ways (four workgroups, quads cut by
# both edges, aprons that read across workgroups, plane rows no word is aligned in); 67 x 5
FRAMES = [(1, 1), (1, 2), (2, 1), (8, 32), (9, 33), (5, 67)]
LOCAL = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}
NAMES = {v: k for k, v in V.STANDARDS.items()}


def shown(st, source, exposure, kw, total=None, levels=False, hdr=None, **chain):
    """State.display_video with video_ref's enumerators: (the frame's bytes, the levels or None)."""
    q = dict(kw, standard=NAMES[kw["standard"]], **({} if hdr is None else hdr))
    got = st.display_video(source, exposure, sample_total=total, levels=levels, **q, **chain)
    frame, lv = got if levels else (got, None)
    h, w = frame.height, frame.width
    assert frame.data.dtype == np.uint8 and frame.data.size == V.frame_bytes(h, w, kw["depth"]) and frame.y.shape == (h, w) and frame.cb.shape == frame.cr.shape == ((h + 1) // 2, (w + 1) // 2)
    return frame, lv


def check_everything_on(st, img, total, source, exposure=0.37, white=(1.3, 0.95, 0.6), combos=COMBOS, dithers=((0.0, 0), (1.0, 0x9e3779b9))):
    """Local exposure (cell 8), bloom (3 levels), a white point and, for BT.709, the context's LUT at once on `source`, whose downloaded
    image is img: the device's bytes and levels against the restatement over the downloaded grid, bloom image and LUT; then each off in turn."""
    n = None if source != "mean" else total
    st.bloom(source, exposure, 3, sample_total=n)
    st.local_exposure(source, 8, sample_total=n)
    b, (grid, cell), lut = st.bloom_download(), st.local_exposure_download(), st.colour_lut_download()
    assert cell == 8
    gain = local_ref.gains(img, total, exposure, grid, cell, **LOCAL)
    h, w = img.shape[:2]
    for wh, g, intensity, strength in ((white, gain, 0.5, 0.75), (white, None, 0.5, 0.75), (white, gain, 0.0, 0.75), ((1.0, 1.0, 1.0), gain, 0.5, 0.75),
                                       (white, gain, 0.5, 0.0), ((1.0, 1.0, 1.0), None, 0.0, 0.0)):
        for standard in sorted({kw["standard"] for kw in combos}):
            hdr = HDR if standard == V.HDR10 else None
            if hdr is not None and strength == 0 and g is not None:
                continue  # (HDR10 takes no LUT: the chain with only the LUT off is its first)
            s = 0.0 if hdr is not None else strength
            x = V.source(img, total, exposure, wh, lut, s, g, intensity, b, hdr)  # the restatement's steps 1 to 3, once a chain
            yc = V.ycc(V.signal(x, standard), standard)
            chain = dict(white=wh, bloom_intensity=intensity, lut_strength=s, **(LOCAL if g is not None else {}))
            want_lv = None
            if hdr is not None:  # the very integers display_hdr gives for the same parameters, and hdr_ref's
                want_lv = hdr_ref.levels(x)
                assert want_lv == st.display_hdr(source, exposure, sample_total=n, levels=True, **hdr, **{k: v for k, v in chain.items() if k != "lut_strength"})[1]
            for kw in (c for c in combos if c["standard"] == standard):
                for dither, seed in dithers:
                    q = dict(kw, dither=dither, seed=seed)
                    frame, lv = shown(st, source, exposure, q, n, levels=hdr is not None, hdr=hdr, **chain)
                    codes = V.codes_of(yc, **q)
                    assert np.array_equal(frame.data, V.pack(*codes, **q)), (source, q, intensity, g is None, s)
                    assert all(np.array_equal(a, c) for a, c in zip((frame.y, frame.cb, frame.cr), codes))
                    if hdr is not None:
                        assert lv == want_lv, (source, q, lv, want_lv)
                        assert np.array_equal(shown(st, source, exposure, q, n, hdr=hdr, **chain)[0].data, frame.data)  # the variant without the levels: the same frame


@pytest.mark.parametrize("h,w", FRAMES)
def test_synthetic_frames_equal_the_numpy_restatement_byte_for_byte(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=2000 * h + w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.colour_lut(*colour_ref.CDLS["warm"], size=3)
        check_everything_on(st, sums, 3, "mean")
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


@pytest.fixture(scope="module")
def house():
    """House at 96 x 54 and 4 spp with the denoised and the upsampled (192 x 108) image, and a 17^3 LUT."""
    w, h = 96, 54
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)
    st.colour_lut(*colour_ref.CDLS["warm"], size=17)
    yield st, {"mean": (st.download(), 4), "denoised": (denoised(st), 1), "upsampled": (upsampled(st), 1)}
    st.close()


def held(st):
    return [st.download(), st.download_aov(), st.download_guide(), denoised(st), upsampled(st)]


def test_a_render_its_denoised_and_its_upsampled_image(house):
    st, images = house
    before = held(st)
    assert images["mean"][0].shape == images["denoised"][0].shape == (54, 96, 4) and images["upsampled"][0].shape == (108, 192, 4)
    # every kernel variant once: the three standards x depths at the three sitings, layouts and ranges taking turns
    turn = lambda c: (3 * [(V.BT709, 8), (V.BT709, 10), (V.HDR10, 10)].index((c["standard"], c["depth"])) + c["siting"]) % 4  # noqa: E731
    combos = [c for c in COMBOS if (c["layout"], c["range"]) == (turn(c) % 2, turn(c) // 2)]
    assert len({(c["standard"], c["depth"], c["siting"]) for c in combos}) == 9 and len({(c["layout"], c["range"]) for c in combos}) == 4
    for source, (img, total) in images.items():
        check_everything_on(st, img, total, source, exposure=1.5, combos=combos, dithers=((0.5, 3),))
    grid, b = st.local_exposure_download()[0], st.bloom_download()
    kw = dict(COMBOS[0], dither=1.0)  # the same seed gives the same bytes, another does not; a seed of any size or sign: its low 32 bits
    a = shown(st, "mean", 1.5, dict(kw, seed=0))[0].data
    assert np.array_equal(a, shown(st, "mean", 1.5, dict(kw, seed=0))[0].data) and not np.array_equal(a, shown(st, "mean", 1.5, dict(kw, seed=1))[0].data)
    assert np.array_equal(shown(st, "mean", 1.5, dict(kw, seed=3))[0].data, shown(st, "mean", 1.5, dict(kw, seed=(1 << 32) + 3))[0].data)
    f = st.display_video("mean", 1.5, lut_strength=0.0)  # the defaults: BT.709 NV12, limited range, left siting, no dither
    assert (f.params.standard, f.params.depth, f.params.layout, f.params.range, f.params.siting) == (0, 8, 0, 0, 0) and f.data.size == 96 * 54 * 3 // 2
    assert 16 <= f.y.min() and f.y.max() <= 235 and 16 <= min(f.cb.min(), f.cr.min()) and max(f.cb.max(), f.cr.max()) <= 240
    # against the colour display of the same call: a luma code is the BT.709 luma of the sRGB bytes to a code and a half (half a byte a channel through
    # the weights, the continuous code's distance and the quantiser's half)
    rgb = st.display_colour_srgb8("mean", 1.5, lut_strength=0.0)[..., :3].astype(np.float64) / 255
    luma = 16 + 219 * (rgb @ np.array([0.2126, 0.7152, 0.0722]))
    assert np.abs(f.y - luma).max() <= 0.5 * 219 / 255 + 0.5 + 0.01
    g = st.display_video("mean", 1.5, standard="hdr10")
    assert (g.params.standard, g.params.depth, g.params.layout) == (1, 10, 0) and g.data.size == 96 * 54 * 3 and g.y.max() <= 940
    for a, c in zip(before + [grid, b], held(st) + [st.local_exposure_download()[0], st.bloom_download()]):
        assert util.same_bits_or_nan(a, c)  # nothing the context holds was written


def test_refusals_return_their_status_and_leave_everything(house):
    st, images = house
    img, total = images["mean"]
    L, S = st._L, R.state
    st.bloom("mean", 1.5, 3)
    st.local_exposure("mean", 8)
    everything = lambda: held(st) + [st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()]  # noqa: E731
    before = everything()
    vp, hp, cp = video_params, hdr_params, colour_params
    n8, n10 = V.frame_bytes(54, 96, 8), V.frame_bytes(54, 96, 10)
    buf = np.full(n10, 0x07, np.uint8)
    lv = S.HdrLevels(7, 7, 7.0, 7.0, 7)
    lp = lambda: S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)  # noqa: E731
    ref = lambda p: C.byref(p) if p is not None else None  # noqa: E731
    show = lambda source, n, e, c, h, v, local=None, i=0.0, b=buf, nb=None, levels=None: st._check(  # noqa: E731
        L.rsrt_display_video(st._ctx, source, n, e, ref(local), i, ref(c), ref(h), ref(v), S._p(b) if b is not None else None,
                             (n10 if v is None or v.depth == 10 else n8) if nb is None else nb, ref(levels)), "rsrt_display_video")
    hdr10 = lambda **kw: vp(standard=V.HDR10, depth=10, **kw)  # noqa: E731
    show(0, 4, 1.5, cp((2, 1, 0.5)), hp(), hdr10(siting=V.TOPLEFT), local=lp(), i=0.5, levels=lv)
    good, good_lv = buf.copy(), (lv.sum_q, lv.max_q, lv.max_cll, lv.max_fall)
    want, _, want_lv = V.display(img, total, 1.5, (2, 1, 0.5), None, 0.0, local_ref.gains(img, total, 1.5, before[-3], 8), 0.5, before[-2], hdr=HDR,
                                 standard=V.HDR10, depth=10, siting=V.TOPLEFT)
    assert np.array_equal(good, want) and good_lv == (want_lv["sum_q"], want_lv["max_q"], want_lv["max_cll"], want_lv["max_fall"])
    unwritten = lambda: np.array_equal(buf, good) and (lv.sum_q, lv.max_q, lv.max_cll, lv.max_fall) == good_lv  # noqa: E731
    nan, inf = float("nan"), float("inf")
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), vp(standard=V.HDR10, depth=8)))  # HDR10 at 8 bits
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, hdr10()))  # HDR10 with a NULL hdr
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), vp()))  # hdr given with BT.709
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), vp(depth=10)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(encoding=hdr_ref.SCRGB16F), hdr10()))  # hdr->encoding scRGB
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(peak=100.0), hdr10()))  # an hdr rsrt_hdr_params_ok refuses
    raises(INVALID, lambda: show(0, 4, 1.5, cp(strength=0.5), hp(), hdr10()))  # the LUT with HDR10, though the context holds one
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(), levels=lv))  # levels_out with BT.709
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(depth=10), levels=lv))
    for nb in (n8 - 1, n8 + 1, n10, 96 * 54 * 4, 0):  # a wrong n_bytes: one off, the other depth's, the RGBA display's
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(), nb=nb))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), hp(), hdr10(), nb=n8))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(), b=None))  # a NULL host_out
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, None))  # a NULL video
    for bad in [{"dither": v} for v in (-0.001, 1.001, nan, inf)] + [{"siting": 3}, {"standard": 2}, {"depth": 12}, {"layout": 2}, {"range": 2}, {"flags": 1}]:
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(**bad)))  # a bad dither, an unknown siting, each other bad field
    raises(INVALID, lambda: show(9, 4, 1.5, cp(), None, vp()))  # source 9 unknown (no pass writes a video image)
    raises(INVALID, lambda: show(0, 0, 1.5, cp(), None, vp()))  # what the colour display refuses: sample_total 0, a bad exposure, colour, local, intensity
    raises(INVALID, lambda: show(0, 4, 0.0, cp(), None, vp()))
    raises(INVALID, lambda: show(0, 4, 1.5, None, None, vp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp((0.0, 1.0, 1.0)), None, vp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(), local=S.LocalParams(-0.1, 0.5, 0.18, 4.0, 0, 0)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp(), i=-0.5))
    raises(NOT_READY, lambda: show(2, 4, 1.5, cp(), None, vp()))  # no temporal image in this context
    st.set_partition(0, 2)  # a context under a partition
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None, vp()))
    raises(INVALID, lambda: st.display_video("mean", 1.5))
    st.set_partition(0, 1)
    with pytest.raises(ValueError):
        st.display_video("mean", 1.5, layout="nv12", depth=10)
    with pytest.raises(ValueError):
        st.display_video("mean", 1.5, peak=600.0)
    assert unwritten()  # no refused call wrote the host buffer or the levels
    for a, c in zip(before, everything()):
        assert util.same_bits_or_nan(a, c)
    empty = R.State()  # no accumulator
    try:
        raises(NOT_READY, lambda: empty._check(L.rsrt_display_video(empty._ctx, 0, 4, 1.5, None, 0.0, ref(cp()), None, ref(vp()), S._p(buf), n8, None), "rsrt_display_video"))
    finally:
        empty.close()
    # a missing grid or bloom image: needed only when asked for
    st.local_exposure_reset()
    st.bloom_reset()
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), None, vp(), local=lp()))
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), None, vp(), i=0.5))
    assert unwritten()
    show(0, 4, 1.5, cp(), None, vp())  # a good call afterwards still works
    assert np.array_equal(buf[:n8], V.display(img, total, 1.5)[0]) and np.array_equal(buf[n8:], good[n8:]) and (lv.sum_q, lv.max_q) == good_lv[:2]  # (NULL levels: not written)
    show(0, 4, 1.5, cp(), hp(), hdr10(layout=V.PLANAR, range=V.FULL, siting=V.CENTRE), levels=lv)
    want, _, want_lv = V.display(img, total, 1.5, hdr=HDR, standard=V.HDR10, depth=10, layout=V.PLANAR, range=V.FULL, siting=V.CENTRE)
    assert np.array_equal(buf, want) and (lv.sum_q, lv.max_q) == (want_lv["sum_q"], want_lv["max_q"])
    for a, c in zip(before[:5], held(st)):
        assert util.same_bits_or_nan(a, c)


def test_cpp_state_shows_video_like_the_python_state(tmp_path):
    import test_video
    exe = test_video.build_cpp_demo(tmp_path)
    w, h = 64, 36
    path = str(tmp_path / "demo.y4m")
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", "4", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        img = st.download()
        calls = (("nv12", {}, {}), ("i420", dict(layout="i420", range="full", siting="centre", dither=1.0, seed=7), {}), ("i420p10", dict(layout="i420p10"), {}),
                 ("hdr10", dict(standard="hdr10", siting="topleft"), dict(levels=True)))
        frames = {}
        for name, kw, extra in calls:
            got = st.display_video(**kw, **extra)
            frame, lv = got if extra else (got, None)
            q = dict(kw)
            lay = q.pop("layout", "p010" if name == "hdr10" else "nv12")
            ref_kw = dict(standard=V.STANDARDS[q.pop("standard", "bt709")], layout=V.LAYOUTS[lay][0], depth=V.LAYOUTS[lay][1], range=V.RANGES[q.pop("range", "limited")],
                          siting=V.SITINGS[q.pop("siting", "left")], **q)
            want, _, want_lv = V.display(img, 4, e, hdr=HDR if name == "hdr10" else None, **ref_kw)
            assert np.array_equal(frame.data, want) and lv == want_lv
            assert next(f for f in lines if f[0] == name)[1:] == [str(frame.data.nbytes), "%016x" % fnv1a(frame.data.tobytes())]
            frames[name] = frame
            if lv:
                fields = next(f for f in lines if f[0] == "levels")
                assert fields[1:3] == [str(lv["max_q"]), str(lv["sum_q"])] and (F(fields[3]), F(fields[4])) == (F(lv["max_cll"]), F(lv["max_fall"]))
        assert ["defaults", "0", "8", "0", "0", "0", "0", "0", "0"] in lines
        fields, got = read_y4m(path)
        assert fields == ["YUV4MPEG2", "W64", "H36", "F25:1", "Ip", "A1:1", "C420jpeg", "XCOLORRANGE=FULL", "XRSRT_SITING=CENTRE", "XRSRT_STANDARD=BT709"] and len(got) == 2
        for planes in got:
            assert all(np.array_equal(a, b) for a, b in zip(planes, (frames["i420"].y, frames["i420"].cb, frames["i420"].cr)))
    finally:
        st.close()


def test_render_y4m_writes_a_sequence_that_reads_back(tmp_path):
    path = str(tmp_path / "pan.y4m")
    tool = os.path.join(util.ROOT, "tools", "render_y4m.py")
    r = subprocess.run([sys.executable, tool, "house", "48", "26", "2", "4", path, "frames=2", "pan=3,0", "fps=24"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    fields, frames = read_y4m(path)
    assert fields[:7] == ["YUV4MPEG2", "W48", "H26", "F24:1", "Ip", "A1:1", "C420mpeg2"] and "XCOLORRANGE=LIMITED" in fields and len(frames) == 2
    for y, cb, cr in frames:
        assert y.shape == (26, 48) and cb.shape == cr.shape == (13, 24) and 16 <= y.min() and y.max() <= 235 and y.max() - y.min() > 40
        assert 16 <= min(cb.min(), cr.min()) and max(cb.max(), cr.max()) <= 240
    assert not np.array_equal(frames[0][0], frames[1][0])  # the camera moved
    # the first frame is what the State gives for the same scene, environment, size and samples
    st = R.State.new(R.Scene.load_toml(util.scene_path("house")), R.Environment.synthetic(2048, 1024), 48, 26)
    st.max_bounces = 4
    try:
        st.render_samples(2)
        f = st.display_video(layout="i420")
        assert all(np.array_equal(a, b) for a, b in zip(frames[0], (f.y, f.cb, f.cr)))
    finally:
        st.close()
