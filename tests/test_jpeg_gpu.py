"""The JPEG pass on the GPU (rsrt_display_jpeg, rsrt_display_jpeg_coefficients, rsrt_jpeg_encode_coefficients): the device's coefficients and
files against the numpy restatement (tests/jpeg_ref.py) applied to the downloaded source image and the downloaded grid, bloom image and LUT,
byte for byte — pictures of one pixel, one block, partial MCUs either way, exactly one MCU, and more than one workgroup; both subsamplings;
qualities 1, 50, 90 and 100; local exposure, bloom, a white point and a LUT at once and each off in turn; the crafted coefficient sets of
tests/test_jpeg.py through the device's scan and packer; a real render with its denoised and its upsampled image; Pillow's libjpeg on
every file; every refusal and what it leaves; the C++ State and tools/render_jpeg.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref
import jpeg_ref as J
import local_ref
import util
import video_ref as V
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_exposure_gpu import denoised, fnv1a, raises, upsampled
from test_jpeg import NAMES, SUBS, check_avi, crafted, decode, libjpeg_file, params, psnr
from test_video import colour_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
# (h, w): one pixel; one block; partial MCUs both ways; exactly one 4:2:0 MCU; one past it both ways; a narrow strip; 3 x 2 MCUs at 4:2:0 and 6 x 4 at
# 4:4:4: more than one workgroup, block offsets over many words
FRAMES = [(1, 1), (8, 8), (17, 9), (16, 16), (33, 17), (67, 5), (48, 32)]
LOCAL = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}


def check_file(data, w, h, rgba8=None, quality=None, sub=None):
    """libjpeg decodes the file to the right size; against the colour display's bytes of the same call it is no more than 1.5 dB behind
    libjpeg's own file of those bytes."""
    im = decode(data)
    assert im.size == (w, h) and im.mode == "RGB"
    if rgba8 is not None:
        rgb8 = np.ascontiguousarray(rgba8[..., :3])
        ref = decode(libjpeg_file(rgb8, quality, sub))
        assert im.quantization == ref.quantization
        ours, theirs = psnr(np.asarray(im), rgb8), psnr(np.asarray(ref), rgb8)
        print("%dx%d %s q%d: %.2f dB, libjpeg %.2f dB" % (w, h, NAMES[sub], quality, ours, theirs))
        return ours, theirs
    return None


def pooled(h, w):
    """Whether a frame's PSNR is taken over pictures that make 1024 pixels instead of file by file.  tests/test_jpeg.py says why for
    1 x 1 and 8 x 8.  The synthetic accumulators are harsher than its smooth pictures — clipped dots, a window 64 times brighter, the
    special values — and at quality 100 and 4:4:4, where every divisor is 1 and the reference codes the very bytes it is judged
    against, a single 9 x 17 frame of 153 pixels measured 1.62 dB behind libjpeg on the device (restated on the CPU over other exposures
    of the same frame: 1.58 at 9 x 17, 1.08 at 16 x 16, 0.74 at 17 x 33, 0.64 at 5 x 67, 0.49 at 32 x 48, the spread shrinking with the
    pixel count, while every pool of 1024 pixels stays within 0.62).  So every frame below 1024 pixels is pooled, and every file of
    a frame from 1024 pixels upward is held to the bound by itself."""
    return h * w < 1024


def check_everything_on(st, img, total, source, exposure=0.37, white=(1.3, 0.95, 0.6), qualities=(1, 50, 90, 100)):
    """Local exposure (cell 8), bloom (3 levels), a white point and the context's LUT at once on `source`, whose downloaded image is img:
    the device's coefficients and files against the restatement over the downloaded grid, bloom image and LUT; then each off in turn.
    Every file is decoded by libjpeg and, in a frame of 1024 pixels or more, held by itself to the PSNR bound against the colour
    display's bytes of the same call."""
    n = None if source != "mean" else total
    st.bloom(source, exposure, 3, sample_total=n)
    st.local_exposure(source, 8, sample_total=n)
    b, (grid, cell), lut = st.bloom_download(), st.local_exposure_download(), st.colour_lut_download()
    assert cell == 8
    gain = local_ref.gains(img, total, exposure, grid, cell, **LOCAL)
    h, w = img.shape[:2]
    for first, (wh, g, intensity, strength) in enumerate(((white, gain, 0.5, 0.75), (white, None, 0.5, 0.75), (white, gain, 0.0, 0.75), ((1.0, 1.0, 1.0), gain, 0.5, 0.75),
                                                          (white, gain, 0.5, 0.0), ((1.0, 1.0, 1.0), None, 0.0, 0.0))):
        sdr = V.source(img, total, exposure, wh, lut, strength, g, intensity, b)  # the restatement's step 1, once a chain
        chain = dict(white=wh, bloom_intensity=intensity, lut_strength=strength, **(LOCAL if g is not None else {}))
        rgba8 = st.display_colour_srgb8(source, exposure, sample_total=n, **chain)
        for sub in SUBS:
            for quality in (qualities if first == 0 else qualities[2:3]):
                want = J.coefficients(sdr, quality=quality, subsampling=sub)
                got = st.jpeg_coefficients(source, exposure, sample_total=n, quality=quality, subsampling=NAMES[sub], **chain)
                assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want), (source, h, w, sub, quality, np.argwhere(got != want)[:4])
                data = st.display_jpeg(source, exposure, sample_total=n, quality=quality, subsampling=NAMES[sub], **chain)
                assert data == J.from_coefficients(want, w, h, quality=quality, subsampling=sub), (source, h, w, sub, quality)
                assert st.jpeg_encode(got, w, h, quality, NAMES[sub]) == data
                figures = check_file(data, w, h, rgba8, quality, sub)
                if not pooled(h, w):
                    assert figures[0] >= figures[1] - 1.5, (source, h, w, sub, quality, figures)


def check_pooled_psnr(st, sums, total):
    """The PSNR bound of a frame below 1024 pixels, for every subsampling and quality: the bound accumulator shown at as many exposures (three
    decades about its median) and white points, drawn from fixed seeds, as make 1024 pixels; the squared errors of the device's files
    and of libjpeg's, each against the colour display's bytes of the same call, are pooled."""
    h, w = sums.shape[:2]
    m = sums[..., :3] / F(total)
    median = float(np.median(m[np.isfinite(m) & (m > 0)]))
    shown = []
    for k in range(-(-1024 // (h * w))):
        rng = np.random.default_rng(7919 + k)
        e, wh = float(10.0 ** rng.uniform(-2.5, 0.5) / median), tuple(float(v) for v in rng.uniform(0.6, 1.4, 3))
        shown.append((e, wh, np.ascontiguousarray(st.display_colour_srgb8("mean", e, white=wh, lut_strength=0.0, sample_total=total)[..., :3])))
    for sub in SUBS:
        for quality in (1, 50, 90, 100):
            ours, theirs = [], []
            for e, wh, rgb8 in shown:
                data = st.display_jpeg("mean", e, white=wh, lut_strength=0.0, sample_total=total, quality=quality, subsampling=NAMES[sub])
                ours.append(np.asarray(decode(data)).reshape(-1))
                theirs.append(np.asarray(decode(libjpeg_file(rgb8, quality, sub))).reshape(-1))
            truth = np.concatenate([rgb8.reshape(-1) for _, _, rgb8 in shown])
            a, b = psnr(np.concatenate(ours), truth), psnr(np.concatenate(theirs), truth)
            print("%dx%d %s q%d over %d pictures: %.2f dB, libjpeg %.2f dB" % (w, h, NAMES[sub], quality, len(shown), a, b))
            assert a >= b - 1.5, (h, w, sub, quality, a, b)


@pytest.mark.parametrize("h,w", FRAMES)
def test_synthetic_frames_equal_the_numpy_restatement_byte_for_byte(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=3000 * h + w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.colour_lut(*colour_ref.CDLS["warm"], size=3)
        check_everything_on(st, sums, 3, "mean")
        if pooled(h, w):
            check_pooled_psnr(st, sums, 3)
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


def test_crafted_coefficients_through_the_devices_scan_and_packer():
    st = R.State()
    try:
        for name, w, h, sub, c in crafted():
            for quality in (90, 1):
                got = st.jpeg_encode(c, w, h, quality, NAMES[sub])
                assert got == R.host.jpeg_from_coefficients(c, w, h, quality, NAMES[sub]), (name, quality)
                assert got == J.from_coefficients(c, w, h, quality, sub)
                check_file(got, w, h)
        # many worst-case blocks: 1658 bits each, every word of the scan touched by two blocks or written whole
        rng = np.random.default_rng(5)
        c = np.where(rng.random((J.n_blocks(160, 96, J.S420), 64)) < 0.5, -1023, 1023).astype(np.int16)
        c[:, 0] = np.where(np.arange(len(c)) % 2, 1023, -1024)
        got = st.jpeg_encode(c, 160, 96, 90, "420")
        assert got == R.host.jpeg_from_coefficients(c, 160, 96, 90, "420") and len(got) > 200 * len(c)
        # random sparse blocks
        c = (rng.integers(-1023, 1024, (J.n_blocks(100, 60, J.S444), 64)) * (rng.random((J.n_blocks(100, 60, J.S444), 64)) < 0.1)).astype(np.int16)
        assert st.jpeg_encode(c, 100, 60, 50, "444") == R.host.jpeg_from_coefficients(c, 100, 60, 50, "444")
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
    for source, (img, total) in images.items():
        check_everything_on(st, img, total, source, exposure=1.5, qualities=(50, 90, 90))
    grid, b = st.local_exposure_download()[0], st.bloom_download()
    a = st.display_jpeg("mean", 1.5, lut_strength=0.0)  # the defaults: quality 90, 4:2:0
    assert a == st.display_jpeg("mean", 1.5, lut_strength=0.0) == st.display_jpeg("mean", 1.5, lut_strength=0.0, quality=90, subsampling="420")  # two calls, the same bytes
    assert a == J.display(images["mean"][0], 4, 1.5)[0] and a != st.display_jpeg("mean", 1.5, lut_strength=0.0, quality=89)
    assert a[:4] == b"\xff\xd8\xff\xe0" and a[-2:] == b"\xff\xd9" and len(a) < 96 * 54 * 3 // 2  # smaller than the NV12 frame
    for x, y in zip(before + [grid, b], held(st) + [st.local_exposure_download()[0], st.bloom_download()]):
        assert util.same_bits_or_nan(x, y)  # nothing the context holds was written


def test_refusals_return_their_status_and_leave_everything(house):
    st, images = house
    img, total = images["mean"]
    L, S = st._L, R.state
    st.bloom("mean", 1.5, 3)
    st.local_exposure("mean", 8)
    everything = lambda: held(st) + [st.local_exposure_download()[0], st.bloom_download(), st.colour_lut_download()]  # noqa: E731
    before = everything()
    cp, jp = colour_params, params
    room = S.jpeg_max_bytes(96, 54)
    buf = np.full(room, 0x07, np.uint8)
    n_out = C.c_size_t(7)
    lp = lambda: S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)  # noqa: E731
    ref = lambda p: C.byref(p) if p is not None else None  # noqa: E731
    show = lambda source, n, e, c, j, local=None, i=0.0, b=buf, cap=room, nb=n_out: st._check(  # noqa: E731
        L.rsrt_display_jpeg(st._ctx, source, n, e, ref(local), i, ref(c), ref(j), S._p(b) if b is not None else None, cap, ref(nb)), "rsrt_display_jpeg")
    show(0, 4, 1.5, cp((2, 1, 0.5)), jp(75, J.S444), local=lp(), i=0.5)
    want, _ = J.display(img, total, 1.5, (2, 1, 0.5), None, 0.0, local_ref.gains(img, total, 1.5, before[-3], 8), 0.5, before[-2], quality=75, subsampling=J.S444)
    size = n_out.value
    assert buf[:size].tobytes() == want and (buf[size:] == 7).all()
    good = buf.copy()
    unwritten = lambda: np.array_equal(buf, good) and n_out.value == size  # noqa: E731
    # the capacity protocol: the size needed comes back, the buffer is untouched, and the call with that room succeeds
    for cap in (0, 1, size - 1):
        n_out.value = 7
        raises(INVALID, lambda: show(0, 4, 1.5, cp((2, 1, 0.5)), jp(75, J.S444), local=lp(), i=0.5, cap=cap))
        assert n_out.value == size and np.array_equal(buf, good)
    exact = np.full(size, 9, np.uint8)
    show(0, 4, 1.5, cp((2, 1, 0.5)), jp(75, J.S444), local=lp(), i=0.5, b=exact, cap=size)
    assert exact.tobytes() == want and n_out.value == size
    assert st.display_jpeg("mean", 1.5, white=(2, 1, 0.5), lut_strength=0.0, quality=100, subsampling="444") == J.display(img, total, 1.5, (2, 1, 0.5), quality=100, subsampling=J.S444)[0]  # (the State's guess is too small at quality 100: its second call)
    nan = float("nan")
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), None))  # a NULL jpeg
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp(), b=None))  # a NULL host_out
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp(), nb=None))  # a NULL n_bytes_out
    for bad in ({"quality": 0}, {"quality": 101}, {"subsampling": 2}, {"flags": 1}, {"reserved": 1}):
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp(**bad)))
    raises(INVALID, lambda: show(9, 4, 1.5, cp(), jp()))  # source 9 unknown
    raises(INVALID, lambda: show(0, 0, 1.5, cp(), jp()))  # what the colour display refuses: sample_total 0, a bad exposure, colour, local, intensity
    raises(INVALID, lambda: show(0, 4, 0.0, cp(), jp()))
    raises(INVALID, lambda: show(0, 4, nan, cp(), jp()))
    raises(INVALID, lambda: show(0, 4, 1.5, None, jp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp((0.0, 1.0, 1.0)), jp()))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp(), local=S.LocalParams(-0.1, 0.5, 0.18, 4.0, 0, 0)))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp(), i=-0.5))
    raises(NOT_READY, lambda: show(2, 4, 1.5, cp(), jp()))  # no temporal image in this context
    # the coefficients' entry point: its count, its NULLs
    n_values = 64 * J.n_blocks(96, 54, J.S420)
    cbuf = np.full(n_values + 64, 7, np.int16)
    coefs = lambda j, n=n_values, b=cbuf: st._check(L.rsrt_display_jpeg_coefficients(st._ctx, 0, 4, 1.5, None, 0.0, ref(cp()), ref(j), S._p(b) if b is not None else None, n),  # noqa: E731
                                                    "rsrt_display_jpeg_coefficients")
    for n in (n_values - 1, n_values + 1, 0, 64 * J.n_blocks(96, 54, J.S444)):
        raises(INVALID, lambda: coefs(jp(), n))
    raises(INVALID, lambda: coefs(jp(), b=None))
    raises(INVALID, lambda: coefs(None))
    raises(INVALID, lambda: coefs(jp(quality=0)))
    assert (cbuf == 7).all()
    coefs(jp())
    assert np.array_equal(cbuf[:n_values].reshape(-1, 64), J.display(img, total, 1.5)[1]) and (cbuf[n_values:] == 7).all()
    # the coder's entry point: an out-of-range coefficient is found before anything is launched
    c = cbuf[:n_values].copy()
    enc = lambda cc, w=96, h=54, j=jp(), n=None, b=buf, cap=room, nb=n_out: st._check(  # noqa: E731
        L.rsrt_jpeg_encode_coefficients(st._ctx, w, h, ref(j), S._p(cc) if cc is not None else None, cc.size if n is None else n, S._p(b) if b is not None else None, cap, ref(nb)),
        "rsrt_jpeg_encode_coefficients")
    n_out.value = size
    for at, value in ((5, 1024), (5, -1024), (64, 1024), (64, -1025), (n_values - 1, 2000)):
        bad = c.copy()
        bad[at] = value
        raises(INVALID, lambda: enc(bad))
    bad = c.copy()
    bad[64] = -1024  # (a DC may be)
    raises(INVALID, lambda: enc(c, n=n_values - 64))
    raises(INVALID, lambda: enc(c, w=0))
    raises(INVALID, lambda: enc(c, w=65536))
    raises(INVALID, lambda: enc(c, j=None))
    raises(INVALID, lambda: enc(c, j=jp(quality=101)))
    raises(INVALID, lambda: enc(c, b=None))
    raises(INVALID, lambda: enc(c, nb=None))
    raises(INVALID, lambda: enc(np.zeros(64 * 6, np.int16), w=65535, h=65535))  # a worst case of 2^32 bits and more
    assert unwritten()
    raises(INVALID, lambda: enc(c, cap=100))
    assert n_out.value == len(J.display(img, total, 1.5)[0]) and np.array_equal(buf, good)
    n_out.value = size
    st.set_partition(0, 2)  # a context under a partition
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), jp()))
    raises(INVALID, lambda: coefs(jp()))
    raises(INVALID, lambda: enc(c))
    raises(INVALID, lambda: st.display_jpeg("mean", 1.5))
    st.set_partition(0, 1)
    assert unwritten()  # no refused call wrote the host buffer or the size
    for a, b in zip(before, everything()):
        assert util.same_bits_or_nan(a, b)
    empty = R.State()  # no accumulator
    try:
        raises(NOT_READY, lambda: empty._check(L.rsrt_display_jpeg(empty._ctx, 0, 4, 1.5, None, 0.0, ref(cp()), ref(jp()), S._p(buf), room, ref(n_out)), "rsrt_display_jpeg"))
        assert empty.jpeg_encode(bad.reshape(-1, 64), 96, 54) == R.host.jpeg_from_coefficients(bad, 96, 54)  # the coder needs no picture and no scene
    finally:
        empty.close()
    # a missing grid, bloom image or LUT: needed only when asked for
    st.local_exposure_reset()
    st.bloom_reset()
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), jp(), local=lp()))
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), jp(), i=0.5))
    assert unwritten()
    show(0, 4, 1.5, cp(), jp())  # a good call afterwards still works
    assert buf[:n_out.value].tobytes() == J.display(img, total, 1.5)[0]
    for a, b in zip(before[:5], held(st)):
        assert util.same_bits_or_nan(a, b)


def test_cpp_state_shows_jpeg_like_the_python_state(tmp_path):
    import test_jpeg
    exe = test_jpeg.build_cpp_demo(tmp_path)
    w, h = 64, 36
    path = str(tmp_path / "demo.jpg")
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", "4", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        img = st.download()
        for name, kw in (("default", {}), ("q50_444", dict(quality=50, subsampling="444")), ("q100", dict(quality=100))):
            data = st.display_jpeg(**kw)
            assert data == J.display(img, 4, e, quality=kw.get("quality", 90), subsampling=J.SUBSAMPLINGS[kw.get("subsampling", "420")])[0]
            assert next(f for f in lines if f[0] == name)[1:] == [str(len(data)), "%016x" % fnv1a(data)]
        assert ["defaults", "90", "0", "0", "0"] in lines
        assert open(path, "rb").read() == st.display_jpeg() and decode(open(path, "rb").read()).size == (w, h)
    finally:
        st.close()


def test_render_jpeg_writes_a_still_and_a_clip(tmp_path):
    tool = os.path.join(util.ROOT, "tools", "render_jpeg.py")
    still, clip = str(tmp_path / "still.jpg"), str(tmp_path / "pan.avi")
    r = subprocess.run([sys.executable, tool, "house", "48", "27", "2", "4", still, "quality=85"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    im = decode(open(still, "rb").read())
    assert im.size == (48, 27) and np.asarray(im).std() > 10
    r = subprocess.run([sys.executable, tool, "house", "48", "27", "2", "4", clip, "frames=3", "pan=3,0", "fps=24"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    a = check_avi(clip, 3, 48, 27, (24, 1))
    assert a["frames"][0] != a["frames"][1]  # the camera moved
    # the first frame is what the State gives for the same scene, environment, size and samples
    st = R.State.new(R.Scene.load_toml(util.scene_path("house")), R.Environment.synthetic(2048, 1024), 48, 27)
    st.max_bounces = 4
    try:
        st.render_samples(2)
        assert a["frames"][0] == st.display_jpeg()
    finally:
        st.close()
