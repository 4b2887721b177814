"""Bloom on the GPU (rsrt_bloom, rsrt_bloom_download, rsrt_display_bloomed_srgb8): the bloom image and the bloomed display against the
numpy restatement (tests/bloom_ref.py), bit for bit, on frames around the first-level kernel's tile and with special pixels; every
source where it lives, with no effect on any other image; intensity 0 against the exposed display; the documented refusals and what
they leave; the drop rule; a caller's stream; stale scratch; the Python and the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bloom_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, hip_runtime_path, state
from test_temporal_gpu import accumulate
from test_bloom import FRAMES, LEVELS, same, tile_constants

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
TW, TH = tile_constants()
# the CPU test's frames; one texel under and over the source texels an output tile covers (2 TW x 2 TH) and the texels a workgroup
# stages in LDS ((2 TW + 4) x (2 TH + 4)), in each dimension; a frame of several tiles each way that is no multiple of anything
CASES = list(dict.fromkeys(FRAMES + [(2 * TH - 1, 2 * TW - 1), (2 * TH + 1, 2 * TW + 1), (2 * TH + 3, 2 * TW + 3), (2 * TH + 5, 2 * TW + 5),
                                     (4 * TH + 7, 6 * TW + 5)]))


def raises(status, call):
    with pytest.raises(R.RsrtError) as e:
        call()
    assert e.value.status == status, e.value


@pytest.mark.parametrize("h,w", CASES)
def test_device_bloom_equals_the_numpy_restatement_bit_for_bit(h, w):
    sums, _ = bloom_ref.synthetic(h, w, seed=1000 * h + w)
    total, exposure = 3, 0.37
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        plain = st.display_exposed_srgb8("mean", exposure, sample_total=total)
        for levels in LEVELS:
            for karis in (True, False):
                for threshold in ((0.0, 1.0) if levels == 6 else (1.0,)):
                    case = (levels, karis, threshold)
                    st.bloom("mean", exposure, levels, threshold, karis, sample_total=total)
                    got = st.bloom_download()
                    want = bloom_ref.bloom(sums, total, exposure, levels, threshold, karis)
                    assert got.shape == want.shape and same(got, want), case
                    assert np.isfinite(got).all() and (got >= 0).all()
                    for intensity in (0.1, 2.0):
                        assert np.array_equal(st.display_bloomed_srgb8("mean", exposure, intensity, sample_total=total),
                                              bloom_ref.display(sums, total, exposure, intensity, want)), (case, intensity)
                    assert np.array_equal(st.display_bloomed_srgb8("mean", exposure, 0.0, sample_total=total), plain), case
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
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
    return [st.download(), st.download_aov(), st.download_guide(), st.download_temporal(), denoised(st), upsampled(st), st.exposure_download()[0]]


@pytest.fixture(scope="module")
def rendered():
    """A small real render with every image the library can hold: (state, {source: (its download, total)})."""
    w, h = 48, 32
    sc, st = state("default", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)  # accumulator + AOV (4 spp), the guide, the denoised and the upsampled (96 x 64) image
    accumulate(st, 4)                       # a first temporal frame of the same accumulator and AOV buffer
    st.exposure_meter()
    images = {"mean": (st.download(), 4), "denoised": (denoised(st), 1), "temporal": (st.download_temporal(), 1), "upsampled": (upsampled(st), 1)}
    yield st, images
    st.close()


def test_each_source_blooms_where_it_lives_and_nothing_else_changes(rendered):
    st, images = rendered
    before = everything(st)
    assert images["upsampled"][0].shape == (64, 96, 4) and images["mean"][0].shape == (32, 48, 4)
    blooms = {}
    for source, (img, total) in images.items():
        for exposure, threshold in ((1.0, 0.25), (2.5, 1.0)):
            st.bloom(source, exposure, levels=4, threshold=threshold)
            got = st.bloom_download()
            want = bloom_ref.bloom(img, total, exposure, 4, threshold, True)
            assert got.shape == want.shape and same(got, want), (source, exposure)
            shown = st.display_bloomed_srgb8(source, exposure, 0.5)
            assert shown.shape == img.shape and np.array_equal(shown, bloom_ref.display(img, total, exposure, 0.5, want)), (source, exposure)
            assert np.array_equal(st.display_bloomed_srgb8(source, exposure, 0.0), st.display_exposed_srgb8(source, exposure)), source
        blooms[source] = got
        assert got[..., :3].max() > 0, source  # something does bloom
    assert blooms["upsampled"].shape == (32, 48, 4) and blooms["mean"].shape == (16, 24, 4)
    assert not same(blooms["mean"], blooms["denoised"])
    st.bloom("temporal", 2.5, levels=4, sample_total=0)  # sample_total is ignored for all sources but the mean
    assert same(st.bloom_download(), blooms["temporal"])
    for a, b in zip(before, everything(st)):
        assert util.same_bits_or_nan(a, b)


def test_refusals_return_their_status_and_leave_the_bloom_image(rendered):
    st, images = rendered
    fresh = R.State()
    try:  # nothing exists yet
        for source in ("mean", "denoised", "temporal", "upsampled"):
            raises(NOT_READY, lambda: fresh.bloom(source, 1.0, sample_total=1))
        raises(NOT_READY, fresh.bloom_download)
    finally:
        fresh.close()
    P = R.state.BloomParams
    raw = lambda source, total, e, params, stream=None: st._check(st._L.rsrt_bloom(st._ctx, source, total, e, params, stream), "rsrt_bloom")  # noqa: E731
    st.bloom("mean", 1.5, levels=3)
    b0 = st.bloom_download()
    assert same(b0, bloom_ref.bloom(images["mean"][0], 4, 1.5, 3))
    good = P(3, 1, 1.0, 0.0)
    for levels in (0, 9):
        raises(INVALID, lambda: st.bloom(levels=levels))
    for flags in (2, 3, 0x10):
        raises(INVALID, lambda: raw(0, 4, 1.0, C.byref(P(3, flags, 1.0, 0.0))))
    for t in (-1.0, float("nan"), float("inf")):
        raises(INVALID, lambda: st.bloom(threshold=t))
    for e in (0.0, -1.0, float("nan"), float("inf")):
        raises(INVALID, lambda: st.bloom(exposure=e))
        raises(INVALID, lambda: st.display_bloomed_srgb8("mean", e))
    for i in (-0.5, float("nan"), float("inf")):
        raises(INVALID, lambda: st.display_bloomed_srgb8("mean", 1.5, i))
    raises(INVALID, lambda: raw(0, 4, 1.0, None))                      # NULL params
    raises(INVALID, lambda: raw(7, 4, 1.0, C.byref(good)))             # unknown source
    raises(INVALID, lambda: st.display_bloomed_srgb8(7, 1.5))
    raises(INVALID, lambda: st.bloom(sample_total=0))                  # sample_total 0 under the mean
    raises(INVALID, lambda: st.display_bloomed_srgb8("mean", 1.5, sample_total=0))
    small = np.zeros(16, np.uint8)
    raises(INVALID, lambda: st._check(st._L.rsrt_display_bloomed_srgb8(st._ctx, 0, 4, 1.5, 0.1, R.state._p(small), small.size), "rsrt_display_bloomed_srgb8"))
    short = np.zeros(8, F)
    raises(INVALID, lambda: st._check(st._L.rsrt_bloom_download(st._ctx, R.state._p(short), short.size, None, None), "rsrt_bloom_download"))
    raises(INVALID, lambda: st.display_bloomed_srgb8("upsampled", 1.5))  # B was built for the accumulator's size, not the guide's
    st.set_partition(0, 2)
    raises(INVALID, st.bloom)
    raises(INVALID, st.bloom_download)
    raises(INVALID, st.bloom_reset)
    raises(INVALID, lambda: st.display_bloomed_srgb8("mean", 1.5))
    st.set_partition(0, 1)
    # after all that: the same bloom image of the same size, and a display that still works
    w, h = C.c_uint32(), C.c_uint32()
    st._check(st._L.rsrt_bloom_download(st._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_bloom_download")
    assert (w.value, h.value) == (24, 16)
    st._check(st._L.rsrt_bloom_download(st._ctx, None, 0, None, C.byref(h)), "rsrt_bloom_download")  # either size pointer may be NULL
    st._check(st._L.rsrt_bloom_download(st._ctx, None, 0, C.byref(w), None), "rsrt_bloom_download")
    assert same(st.bloom_download(), b0)
    assert np.array_equal(st.display_bloomed_srgb8("mean", 1.5, 0.3), bloom_ref.display(images["mean"][0], 4, 1.5, 0.3, b0))
    # a reset drops it; the images stay
    st.bloom_reset()
    raises(NOT_READY, st.bloom_download)
    raises(NOT_READY, lambda: st.display_bloomed_srgb8("mean", 1.5))
    assert same(st.download(), images["mean"][0])
    st.bloom("mean", 1.5, levels=3)
    assert same(st.bloom_download(), b0)


def test_a_change_of_the_accumulators_size_drops_the_bloom_image():
    h, w = 20, 36
    sums, _ = bloom_ref.synthetic(h, w, seed=3)
    other, _ = bloom_ref.synthetic(h, w, seed=4)
    st = R.State()
    try:
        a, b = DeviceArray(sums), DeviceArray(other)
        st.bind_accumulator(a.data_ptr(), w, h)
        st.bloom("mean", 1.0, 3, sample_total=1)
        b0 = st.bloom_download()
        assert same(b0, bloom_ref.bloom(sums, 1, 1.0, 3))
        st.bind_accumulator(b.data_ptr(), w, h)  # the same size: B stays (it is the caller's to rebuild)
        assert same(st.bloom_download(), b0)
        assert np.array_equal(st.display_bloomed_srgb8("mean", 1.0, 0.5, sample_total=1), bloom_ref.display(other, 1, 1.0, 0.5, b0))
        st._check(st._L.rsrt_accumulator_bind(st._ctx, None, 0, 0), "rsrt_accumulator_bind")  # no accumulator any more
        raises(NOT_READY, st.bloom_download)
        st.bind_accumulator(a.data_ptr(), w, h)
        raises(NOT_READY, st.bloom_download)
        raises(NOT_READY, lambda: st.display_bloomed_srgb8("mean", 1.0, sample_total=1))
        st.bloom("mean", 1.0, 3, sample_total=1)
        assert same(st.bloom_download(), b0)
        st.bind_accumulator(a.data_ptr(), h, w)  # another size
        raises(NOT_READY, st.bloom_download)
    finally:
        st.close()
    sc, st = state("default", 32, 16)
    try:
        st.render_samples(2)
        st.bloom()
        assert st.bloom_download().shape == (8, 16, 4)
        st.resize(48, 24)
        raises(NOT_READY, st.bloom_download)
        raises(NOT_READY, st.display_bloomed_srgb8)
        st.render_samples(2)
        st.bloom()
        assert same(st.bloom_download(), bloom_ref.bloom(st.download(), 2, 1.0))
    finally:
        st.close()


def test_a_callers_stream_and_calls_in_a_row():
    h, w = 4 * TH + 7, 6 * TW + 5
    sums, _ = bloom_ref.synthetic(h, w, seed=9)
    R.state.lib()
    hip = C.CDLL(hip_runtime_path())  # a caller stream from the HIP runtime the library itself uses
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.bloom("mean", 0.5, 6, sample_total=3)
        own = st.bloom_download()
        st.bloom_reset()
        st.bloom("mean", 0.5, 6, sample_total=3, stream=stream.value)
        st.synchronize()
        assert same(st.bloom_download(), own) and same(own, bloom_ref.bloom(sums, 3, 0.5, 6))
        # two calls in a row with different levels: the second call's bits, whichever is deeper (no stale scratch)
        for first, second in ((8, 2), (1, 6), (6, 1)):
            st.bloom("mean", 0.5, first, sample_total=3)
            st.bloom("mean", 0.5, second, sample_total=3, stream=stream.value)
            assert same(st.bloom_download(), bloom_ref.bloom(sums, 3, 0.5, second)), (first, second)
    finally:
        st.close()
        hip.hipStreamDestroy(stream)


def test_the_python_state_round_trip_on_house():
    w, h = 64, 36
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        r = st.auto_exposure()
        st.bloom()
        acc = st.download()
        want = bloom_ref.bloom(acc, 4, F(r["exposure"]), **{k: bloom_ref.DEFAULTS[k] for k in ("levels", "threshold")})
        assert same(st.bloom_download(), want) and want[..., :3].max() > 0
        shown = st.display_bloomed_srgb8()
        assert np.array_equal(shown, bloom_ref.display(acc, 4, F(r["exposure"]), bloom_ref.DEFAULTS["intensity"], want))
        assert not np.array_equal(shown, st.display_exposed_srgb8())
        assert np.array_equal(st.display_bloomed_srgb8(intensity=0.0), st.display_exposed_srgb8())
        st.exposure_reset()  # no remembered exposure: 1
        st.bloom(karis=False, levels=2, threshold=0.5)
        assert same(st.bloom_download(), bloom_ref.bloom(acc, 4, 1.0, 2, 0.5, False))
    finally:
        st.close()


def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    return h


def test_cpp_state_blooms_like_the_python_state(tmp_path):
    import test_bloom
    exe = test_bloom.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "4", "5"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("spheres_only", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        assert ["exposure", "%08x" % int(np.asarray(e, F).view(np.uint32))] in lines
        st.bloom(levels=5)
        b = st.bloom_download()
        assert same(b, bloom_ref.bloom(st.download(), 4, F(e), 5))
        assert next(f for f in lines if f[0] == "bloom")[1:] == [str(w // 2), str(h // 2), "%016x" % fnv1a(b.tobytes())]
        shown = st.display_bloomed_srgb8()
        assert next(f for f in lines if f[0] == "display")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        assert ["intensity0", "yes"] in lines and ["reset", "yes"] in lines
    finally:
        st.close()
