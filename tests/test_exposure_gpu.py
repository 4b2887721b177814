"""Auto-exposure on the GPU (rsrt_exposure_meter, rsrt_exposure_download, rsrt_display_exposed_srgb8): the histogram kernel against
its numpy restatement, word for word, special pixels, a constant frame and an all-skipped frame included; every source metered where
it lives, with no effect on any image; the exposed display byte for byte; the documented errors; adaptation through the State;
render_to_noise with an exposure; the C++ State against the Python one."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import exposure_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_temporal_gpu import accumulate
from test_exposure import FRAMES, PARAM_SETS, TOTALS, bits, same_result

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def raises(status, call):
    with pytest.raises(R.RsrtError) as e:
        call()
    assert e.value.status == status, e.value


def result_f32(r):
    return dict(r, **{k: F(r[k]) for k in ("exposure", "target", "average_luminance")})


def constant(h, w):
    s = np.ones((h, w, 4), F)
    s[..., :3] = (0.8, 0.4, 0.1)
    return s


# the CPU test's frames; one that spans several workgroups and is no multiple of a wave (64), a workgroup (256) or a workgroup's pixels
# per trip (1024); one constant colour (every lane of every full wave in one bin); all zeros (everything skipped)
# ... and a frame of more trips than one launch has workgroups, as the FIRST call of a fresh context (every case makes its own): the
# histograms' one-time zeroing must have landed before the kernel adds
CASES = [("synthetic", h, w) for h, w in FRAMES] + [("synthetic", 65, 1031), ("constant", 33, 257), ("zeros", 9, 130), ("synthetic", 540, 1100)]


def frame(kind, h, w):
    if kind == "synthetic":
        return exposure_ref.synthetic(h, w, seed=1000 * h + w)[0]
    return constant(h, w) if kind == "constant" else np.zeros((h, w, 4), F)


@pytest.mark.parametrize("kind,h,w", CASES)
def test_kernel_equals_the_numpy_restatement_word_for_word(kind, h, w):
    sums = frame(kind, h, w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        for total in TOTALS:
            st.exposure_meter(sample_total=total)
            got, r = st.exposure_download()
            want = exposure_ref.histogram(sums, total)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (kind, total)
            assert int(got.astype(np.int64).sum()) == h * w
            for kw in PARAM_SETS:
                assert same_result(result_f32(st.exposure_download(**kw)[1]), exposure_ref.from_histogram(want, **kw)), kw
        if kind == "constant":
            assert np.count_nonzero(got) == 1 and got.max() == h * w
        if kind == "zeros":
            assert got[256] == h * w and r["metered"] == 0 and r["exposure"] == 1.0 and r["average_luminance"] == 0.0
        # two meter calls in a row: the second call's histogram, not the sum
        st.exposure_meter(sample_total=1)
        st.exposure_meter(sample_total=3)
        assert np.array_equal(st.exposure_download()[0], exposure_ref.histogram(sums, 3))
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernel reads only
    finally:
        st.close()


@pytest.fixture(scope="module")
def rendered():
    """A small real render with every image the library can hold: (state, {source: (its download, total)}, the other images)."""
    w, h = 64, 36
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)  # accumulator + AOV (4 spp), the guide, the denoised and the upsampled (128 x 72) image
    accumulate(st, 4)                       # a first temporal frame of the same accumulator and AOV buffer
    images = {"mean": (st.download(), 4), "denoised": (denoised(st), 1), "temporal": (st.download_temporal(), 1),
              "upsampled": (upsampled(st), 1)}
    yield st, images
    st.close()


def denoised(st):
    out = np.empty((st.height, st.width, 4), F)
    st._check(st._L.rsrt_denoised_download(st._ctx, R.state._p(out), out.size), "rsrt_denoised_download")
    return out


def upsampled(st):
    out = np.empty((st.guide_height, st.guide_width, 4), F)
    st._check(st._L.rsrt_upsampled_download(st._ctx, R.state._p(out), out.size), "rsrt_upsampled_download")
    return out


def everything(st):
    return [st.download(), st.download_aov(), st.download_guide(), st.download_temporal(), denoised(st), upsampled(st)]


def test_each_source_is_metered_where_it_lives(rendered):
    st, images = rendered
    before = everything(st)
    assert images["upsampled"][0].shape == (72, 128, 4) and images["mean"][0].shape == (36, 64, 4)
    hists = {}
    for source, (img, total) in images.items():
        st.exposure_meter(source)
        got, r = st.exposure_download()
        assert np.array_equal(got, exposure_ref.histogram(img, total)), source
        assert int(got.astype(np.int64).sum()) == img.shape[0] * img.shape[1] and r["metered"] > 0
        hists[source] = got
    assert int(hists["upsampled"].astype(np.int64).sum()) == 128 * 72  # the guide's pixel count
    assert not np.array_equal(hists["mean"], hists["denoised"])
    st.exposure_meter("temporal", sample_total=0)  # sample_total is ignored for all sources but the mean
    assert np.array_equal(st.exposure_download()[0], hists["temporal"])
    for a, b in zip(before, everything(st)):
        assert util.same_bits_or_nan(a, b)


def test_exposed_display_equals_the_numpy_restatement_byte_for_byte(rendered):
    st, images = rendered
    before = everything(st)
    for source, (img, total) in images.items():
        for e in (1.0, 0.37, 4.0):
            got = st.display_exposed_srgb8(source, e)
            assert got.shape == img.shape and got.dtype == np.uint8
            assert np.array_equal(got, exposure_ref.display(img, total, e)), (source, e)
    assert np.array_equal(st.display_exposed_srgb8("mean", 1.0), st.display_srgb8())
    assert np.array_equal(st.display_exposed_srgb8("denoised", 1.0), st.denoised_display_srgb8())
    assert np.array_equal(st.display_exposed_srgb8("upsampled", 1.0), st.upsampled_display_srgb8())
    assert not np.array_equal(st.display_exposed_srgb8("mean", 4.0), st.display_srgb8())
    for a, b in zip(before, everything(st)):
        assert util.same_bits_or_nan(a, b)


def test_exposed_display_of_special_pixels():
    h, w = 37, 70
    sums, _ = exposure_ref.synthetic(h, w, seed=1000 * h + w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        for total in TOTALS:
            for e in (1.0, 0.37, 4.0):
                assert np.array_equal(st.display_exposed_srgb8("mean", e, sample_total=total), exposure_ref.display(sums, total, e)), (total, e)
            assert np.array_equal(st.display_exposed_srgb8("mean", 1.0, sample_total=total), st.display_srgb8(sample_total=total))
        assert util.same_bits_or_nan(dev.numpy(), sums)
    finally:
        st.close()


def test_errors_and_what_a_refused_call_leaves():
    st = R.State()
    try:  # nothing exists yet
        raises(NOT_READY, lambda: st.exposure_meter(sample_total=1))
        for source in ("denoised", "temporal", "upsampled"):
            raises(NOT_READY, lambda: st.exposure_meter(source))
            raises(NOT_READY, lambda: st.display_exposed_srgb8(source, 1.0))
        raises(NOT_READY, st.exposure_download)
        raises(NOT_READY, st.display_exposed_srgb8)  # no remembered exposure
    finally:
        st.close()
    sc, st = state("default", 32, 16)
    try:
        P = R.state.ExposureParams
        raw_dl = lambda params, hist, n, out=None: st._check(st._L.rsrt_exposure_download(st._ctx, params, hist, n, out), "rsrt_exposure_download")  # noqa: E731
        raises(NOT_READY, st.exposure_download)  # download before meter
        st.render_samples(4)
        raises(NOT_READY, lambda: st.exposure_meter("denoised"))
        raises(NOT_READY, lambda: st.exposure_meter("temporal"))
        raises(NOT_READY, lambda: st.exposure_meter("upsampled"))
        acc = st.download()
        st.exposure_meter()
        hist, r = st.exposure_download()
        assert np.array_equal(hist, exposure_ref.histogram(acc, 4))
        # refused calls: nothing is launched, the last histogram and the accumulator stay what they were
        raises(INVALID, lambda: st.exposure_meter(7))                 # unknown source
        raises(INVALID, lambda: st.exposure_meter(sample_total=0))    # sample_total 0 under the mean
        raises(INVALID, lambda: raw_dl(None, None, 0))                # NULL params
        for kw in ({"low_permille": 950}, {"high_permille": 1001}, {"key": 0.0}, {"key": float("nan")}, {"min_exposure": -1.0},
                   {"max_exposure": float("inf")}, {"min_exposure": 2.0, "max_exposure": 1.0}, {"blend": 1.5}, {"blend": -0.5},
                   {"previous_exposure": -1.0}, {"previous_exposure": float("nan")}):
            raises(INVALID, lambda: st.exposure_download(**kw))
        d = exposure_ref.DEFAULTS
        flagged = P(d["low_permille"], d["high_permille"], d["key"], d["min_exposure"], d["max_exposure"], d["blend"], d["previous_exposure"], 1)
        raises(INVALID, lambda: raw_dl(C.byref(flagged), None, 0))    # flags
        good = P(d["low_permille"], d["high_permille"], d["key"], d["min_exposure"], d["max_exposure"], d["blend"], d["previous_exposure"], 0)
        short = np.zeros(256, np.uint32)
        raises(INVALID, lambda: raw_dl(C.byref(good), R.state._p(short), short.size))  # n_words not 257
        for e in (0.0, -1.0, float("nan"), float("inf")):
            raises(INVALID, lambda: st.display_exposed_srgb8("mean", e))
        raises(INVALID, lambda: st.display_exposed_srgb8("mean", 1.0, sample_total=0))
        raises(INVALID, lambda: st.display_exposed_srgb8(9, 1.0))
        small = np.zeros(16, np.uint8)
        raises(INVALID, lambda: st._check(st._L.rsrt_display_exposed_srgb8(st._ctx, 0, 4, 1.0, R.state._p(small), small.size), "rsrt_display_exposed_srgb8"))
        st.set_partition(0, 2)
        raises(INVALID, st.exposure_meter)
        raises(INVALID, st.exposure_download)
        raises(INVALID, lambda: st.display_exposed_srgb8("mean", 1.0))
        st.set_partition(0, 1)
        h2, r2 = st.exposure_download()
        assert np.array_equal(h2, hist) and r2 == r and same(st.download(), acc)
        # the histogram alone (out NULL), the result alone (host_hist NULL, n_words ignored)
        only = np.zeros(257, np.uint32)
        raw_dl(C.byref(good), R.state._p(only), only.size)
        assert np.array_equal(only, hist)
        res = R.state.ExposureResult()
        raw_dl(C.byref(good), None, 12345, C.byref(res))
        assert (res.exposure, res.metered, res.skipped) == (r["exposure"], r["metered"], r["skipped"])
        # a reset drops the histogram and the remembered exposure; the images stay
        st.auto_exposure()
        assert st.exposure is not None and st.display_exposed_srgb8().shape == (16, 32, 4)
        st.exposure_reset()
        assert st.exposure is None
        raises(NOT_READY, st.exposure_download)
        raises(NOT_READY, st.display_exposed_srgb8)
        assert same(st.download(), acc)
        st.exposure_meter()
        assert np.array_equal(st.exposure_download()[0], hist)
    finally:
        st.close()


def test_auto_exposure_adapts_through_previous_exposure_and_blend():
    h, w = 37, 70
    sums, _ = exposure_ref.synthetic(h, w, seed=11)
    bright = (sums * F(4)).astype(F)
    st = R.State()
    try:
        a, b = DeviceArray(sums), DeviceArray(bright)
        st.bind_accumulator(a.data_ptr(), w, h)
        st.sample_count = 1
        t = exposure_ref.from_histogram(exposure_ref.histogram(sums, 1))["target"]
        for _ in range(3):  # the first takes the target; after that the previous value equals the target: t, t, t
            r = st.auto_exposure(blend=0.5)
            assert bits(r["exposure"]) == bits(t) == bits(r["target"]) == bits(st.exposure)
        st.bind_accumulator(b.data_ptr(), w, h)  # the frame times 4 in between
        st.sample_count = 1
        t4 = exposure_ref.from_histogram(exposure_ref.histogram(bright, 1))["target"]
        prev = F(t)
        for _ in range(3):
            r = st.auto_exposure(blend=0.5)
            want = F(prev + F(F(t4 - prev) * F(0.5)))
            assert bits(r["target"]) == bits(t4) and bits(r["exposure"]) == bits(want) == bits(st.exposure)
            assert same_result(result_f32(r), exposure_ref.from_histogram(exposure_ref.histogram(bright, 1), blend=0.5, previous_exposure=float(prev)))
            prev = want
        assert t4 < prev < t
        st.exposure_reset()
        assert bits(st.auto_exposure(blend=0.5)["exposure"]) == bits(t4)  # a first call again
    finally:
        st.close()


@pytest.mark.parametrize("exposure", [4.0, 0.25, "auto"])
def test_render_to_noise_with_an_exposure(exposure):
    """threshold T at exposure E takes the rounds of threshold T / sqrt(E) (an f32 division by an f32 square root) at no exposure."""
    w, h = 64, 36
    T = 3.0
    sc, st = state("spheres_only", w, h)
    _, plain = state("spheres_only", w, h)
    try:
        total, rounds = st.render_to_noise(T, min_samples=8, max_samples=64, exposure=exposure)
        if exposure == "auto":
            plain.render_samples(8)
            plain.exposure_meter()
            e = plain.exposure_download()[1]["exposure"]
            assert bits(st.exposure) == bits(e) and e > 0
        else:
            e = exposure
            assert st.exposure is None
        scaled = float(F(T) / np.sqrt(F(e)))
        ptotal, prounds = plain.render_to_noise(scaled, min_samples=8, max_samples=64)
        assert (total, rounds) == (ptotal, prounds) and total == st.sample_count
        assert same(st.download(), plain.download())
        if exposure == "auto":
            total2, rounds2 = plain.render_to_noise(T, min_samples=8, max_samples=64, exposure=e)  # ... equals passing the metered value
            assert (total2, rounds2) == (total, rounds)
    finally:
        st.close()
        plain.close()


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    return h


def test_cpp_state_meters_and_displays_like_the_python_state(tmp_path):
    import test_exposure
    exe = test_exposure.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "4", "0.5"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    cpp_results = [f[1:] for f in lines if f and f[0] == "result"]
    sc, st = state("spheres_only", w, h)
    try:
        st.render_samples(4)
        py_results = []
        for _ in range(2):
            q = st.auto_exposure(blend=0.5)
            py_results.append(["%08x" % int(bits(q[k])) for k in ("exposure", "target", "average_luminance")] + [str(q["metered"]), str(q["skipped"])])
            st.render_samples(4)
        assert cpp_results == py_results and py_results[0][:3] != py_results[1][:3]
        hist, _ = st.exposure_download()
        assert next(f for f in lines if f[0] == "hist")[1:] == ["257", "%016x" % fnv1a(hist.tobytes())]
        shown = st.display_exposed_srgb8()
        assert next(f for f in lines if f[0] == "display")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes()), "%08x" % int(bits(st.exposure))]
        assert ["reset", "yes"] in lines
    finally:
        st.close()
