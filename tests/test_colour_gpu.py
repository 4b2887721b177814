"""White balance and colour grading on the GPU (rsrt_white_meter, rsrt_white_download, rsrt_colour_lut_build / _upload / _download,
rsrt_display_colour_srgb8): the chroma histogram word for word, the baked LUTs bit for bit and the colour display byte for byte against
the numpy restatement (tests/colour_ref.py), special pixels included; the display identities on the device; every source where it
lives, with no effect on any other image; the documented refusals and what they leave; the Python and the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bloom_ref
import colour_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_exposure_gpu import denoised, everything, fnv1a, raises, rendered, upsampled  # noqa: F401 (rendered is a fixture)
from test_colour import FRAMES as CPU_FRAMES, WHITE_SETS, colour_params, same, same_white, seed_of, white_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
# the CPU test's frames; one that spans several workgroups and is no multiple of a wave, a workgroup or a workgroup's pixels a trip; one
# constant colour (every lane of every full wave in one word); all zeros (everything skipped); and a frame of more trips than one launch
# has workgroups, as the FIRST call of a fresh context: the histograms' one-time zeroing must have landed before the kernel adds
CASES = [("chroma", h, w) for h, w in CPU_FRAMES] + [("chroma", 65, 1031), ("constant", 33, 257), ("zeros", 9, 130), ("chroma", 540, 1100)]


def frame(kind, h, w):
    if kind == "chroma":
        return colour_ref.chroma_frame(h, w, seed=seed_of(h, w))[0]
    s = np.zeros((h, w, 4), F)
    if kind == "constant":
        s[...] = (0.8, 0.4, 0.2, 1.0)
    return s


def result_f32(r):
    return dict(r, **{k: F(r[k]) for k in ("white", "target", "illuminant", "eu", "ev")})


@pytest.mark.parametrize("kind,h,w", CASES)
def test_meter_equals_the_numpy_restatement_word_for_word(kind, h, w):
    sums = frame(kind, h, w)
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        for total in (1, 3):
            st.white_meter(sample_total=total)
            got, r = st.white_download()
            want = colour_ref.histogram(sums, total)
            assert got.dtype == np.uint32 and got.shape == (4097,) and np.array_equal(got, want), (kind, total)
            assert int(got.astype(np.int64).sum()) == h * w
            for kw in WHITE_SETS:
                assert same_white(result_f32(st.white_download(**kw)[1]), colour_ref.from_histogram(want, **kw)), kw
        if kind == "constant":
            assert np.count_nonzero(got) == 1 and got.max() == h * w and r["estimated"]
        if kind == "zeros":
            assert got[4096] == h * w and not r["estimated"] and r["white"] == (1.0, 1.0, 1.0)
        # two meter calls in a row: the second call's histogram, not the sum
        st.white_meter(sample_total=1)
        st.white_meter(sample_total=3)
        assert np.array_equal(st.white_download()[0], colour_ref.histogram(sums, 3))
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernel reads only
    finally:
        st.close()


@pytest.fixture(scope="module")
def blank():
    """A context with a small bound frame and nothing else."""
    sums, _ = local_ref.synthetic(5, 7, seed=seed_of(5, 7))
    st = R.State()
    dev = DeviceArray(sums)
    st.bind_accumulator(dev.data_ptr(), 7, 5)
    yield st, sums, dev
    st.close()


@pytest.mark.parametrize("n", [2, 3, 17, 33])
def test_baked_luts_equal_the_numpy_restatement_bit_for_bit(blank, n):
    st = blank[0]
    for name, cdl in colour_ref.CDLS.items():
        st.colour_lut(*cdl, size=n)
        got = st.colour_lut_download()
        assert got.shape == (n, n, n, 3) and same(got, colour_ref.bake(n, *cdl)), name
    rng = np.random.default_rng(n)
    nodes = rng.random((n, n, n, 3)).astype(F)
    nodes[0, 0, 0], nodes[-1, -1, -1] = 0.0, 1.0
    st.colour_lut_upload(nodes)
    assert same(st.colour_lut_download(), nodes)  # an upload followed by a download is the identity


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (37, 70)])
def test_colour_display_equals_the_numpy_restatement_byte_for_byte(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=seed_of(h, w))
    total, exposure, white = 3, 0.37, (1.3, 0.95, 0.6)
    kw = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.bloom("mean", exposure, 3, sample_total=total)
        b = st.bloom_download()
        assert same(b, bloom_ref.bloom(sums, total, exposure, 3))
        st.local_exposure("mean", 8, sample_total=total)
        gain = local_ref.gains(sums, total, exposure, local_ref.grid_of(sums, total, 8), 8, **kw)
        assert same(st.local_gain("mean", exposure, sample_total=total, **kw), gain)
        show = lambda **a: st.display_colour_srgb8("mean", exposure, sample_total=total, **a)  # noqa: E731
        for n in (2, 3, 17, 33):
            cdl = colour_ref.CDLS["warm" if n != 3 else "crush"]
            st.colour_lut(*cdl, size=n)
            lut = colour_ref.bake(n, *cdl)
            for strength in (0.0, 0.5, 1.0):
                for graded in (False, True):
                    for intensity in (0.0, 0.5):
                        case = (n, strength, graded, intensity)
                        got = show(white=white, lut_strength=strength, bloom_intensity=intensity, **(kw if graded else {}))
                        want = colour_ref.display(sums, total, exposure, white, lut, strength, gain if graded else None, intensity, b)
                        assert got.shape == (h, w, 4) and np.array_equal(got, want), case
        # the identities, on the device: white 1 and strength 0 are the local, the bloomed and the exposed display
        one = {"white": (1.0, 1.0, 1.0), "lut_strength": 0.0}
        assert np.array_equal(show(bloom_intensity=0.5, **one, **kw), st.display_local_srgb8("mean", exposure, bloom_intensity=0.5, sample_total=total, **kw))
        assert np.array_equal(show(**one, **kw), st.display_local_srgb8("mean", exposure, sample_total=total, **kw))
        assert np.array_equal(show(bloom_intensity=0.5, **one), st.display_bloomed_srgb8("mean", exposure, 0.5, sample_total=total))
        plain = st.display_exposed_srgb8("mean", exposure, sample_total=total)
        assert np.array_equal(show(**one), plain)
        for n in (2, 3, 17, 33):  # an identity LUT moves no byte by more than 1
            st.colour_lut(size=n)
            assert np.abs(show(white=(1.0, 1.0, 1.0), lut_strength=1.0).astype(int) - plain.astype(int)).max() <= 1, n
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


def test_a_power_of_two_white_point_is_the_exposed_display_of_the_tinted_frame():
    h, w = 37, 70
    mid = np.ones((h, w, 4), F)
    mid[..., :3] = np.exp(np.random.default_rng(4).normal(-1.0, 1.5, (h, w, 3))).astype(F)  # means that are normal binary16 numbers with room for the factor
    tinted = mid.copy()
    tinted[..., :3] *= F([2, 1, 0.5])
    st = R.State()
    try:
        a, b = DeviceArray(mid), DeviceArray(tinted)
        st.bind_accumulator(a.data_ptr(), w, h)
        got = st.display_colour_srgb8("mean", 1.0, white=(2.0, 1.0, 0.5), lut_strength=0.0, sample_total=1)
        st.bind_accumulator(b.data_ptr(), w, h)
        assert np.array_equal(got, st.display_exposed_srgb8("mean", 1.0, sample_total=1))
    finally:
        st.close()


@pytest.fixture(scope="module")
def sources(rendered):  # noqa: F811
    """test_exposure_gpu's small real render — house at 64 x 36 and 4 spp with the denoised, the temporal and the upsampled (128 x 72)
    image — and a lens image of the mean on top."""
    st, images = rendered
    st.depth_of_field("mean", 3.0, 0.15, 5)
    return st, dict(images, lens=(st.dof_download(), 1))


def test_each_source_is_metered_and_displayed_where_it_lives_and_nothing_else_changes(sources):
    st, images = sources
    before = everything(st) + [st.dof_download()]
    assert images["upsampled"][0].shape == (72, 128, 4) and images["mean"][0].shape == (36, 64, 4) and images["lens"][0].shape == (36, 64, 4)
    cdl = colour_ref.CDLS["warm"]
    st.colour_lut(*cdl, size=17)
    lut = colour_ref.bake(17, *cdl)
    hists = {}
    for source, (img, total) in images.items():
        st.white_meter(source)
        got, r = st.white_download()
        want = colour_ref.histogram(img, total)
        assert np.array_equal(got, want) and int(got.astype(np.int64).sum()) == img.shape[0] * img.shape[1], source
        ref = colour_ref.from_histogram(want)
        assert same_white(result_f32(r), ref) and r["estimated"], source
        hists[source] = got
        st.local_exposure(source, 8)
        gain = local_ref.gains(img, total, 1.5, local_ref.grid_of(img, total, 8), 8)
        for strength, graded in ((0.0, False), (1.0, False), (0.5, True)):
            shown = st.display_colour_srgb8(source, 1.5, white=r["white"], lut_strength=strength, **({"shadows": 0.5} if graded else {}))
            assert shown.shape == img.shape
            assert np.array_equal(shown, colour_ref.display(img, total, 1.5, ref["white"], lut, strength, gain if graded else None)), (source, strength, graded)
        assert np.array_equal(st.white_download()[0], want) and same(st.colour_lut_download(), lut)  # a display leaves both
    assert not np.array_equal(hists["mean"], hists["denoised"])
    st.white_meter("temporal", sample_total=0)  # sample_total is ignored for all sources but the mean
    assert np.array_equal(st.white_download()[0], hists["temporal"])
    for a, b in zip(before, everything(st) + [st.dof_download()]):
        assert util.same_bits_or_nan(a, b)


def test_refusals_return_their_status_and_leave_the_histogram_and_the_lut(sources):
    st, images = sources
    img, total = images["mean"]
    fresh = R.State()
    try:  # nothing exists yet
        for source in ("mean", "denoised", "temporal", "upsampled", "lens"):
            raises(NOT_READY, lambda: fresh.white_meter(source, sample_total=1))
        raises(NOT_READY, fresh.white_download)
        raises(NOT_READY, fresh.colour_lut_download)
    finally:
        fresh.close()
    L, S = st._L, R.state
    st.white_reset()
    st.colour_lut_reset()
    raises(NOT_READY, st.white_download)  # no histogram, no LUT
    raises(NOT_READY, st.colour_lut_download)
    raises(NOT_READY, lambda: st.display_colour_srgb8("mean", 1.5, lut_strength=0.5))
    assert np.array_equal(st.display_colour_srgb8("mean", 1.5, white=(1, 1, 1), lut_strength=0.0), st.display_exposed_srgb8("mean", 1.5))  # strength 0 needs none
    st.white_meter()
    h0 = st.white_download()[0]
    assert np.array_equal(h0, colour_ref.histogram(img, total))
    st.colour_lut(*colour_ref.CDLS["crush"], size=3)
    lut0 = st.colour_lut_download()
    assert same(lut0, colour_ref.bake(3, *colour_ref.CDLS["crush"]))
    byte_buf, hist_buf = np.zeros((36, 64, 4), np.uint8), np.zeros(4097, np.uint32)
    wp, cp = white_params, colour_params
    meter = lambda source, n: st._check(L.rsrt_white_meter(st._ctx, source, n, None), "rsrt_white_meter")  # noqa: E731
    down = lambda p, buf=hist_buf, n=None: st._check(  # noqa: E731
        L.rsrt_white_download(st._ctx, C.byref(p) if p is not None else None, S._p(buf) if buf is not None else None, (buf.size if buf is not None else 0) if n is None else n, None),
        "rsrt_white_download")
    show = lambda source, n, e, c, local=None, i=0.0, buf=byte_buf, nb=None: st._check(  # noqa: E731
        L.rsrt_display_colour_srgb8(st._ctx, source, n, e, C.byref(local) if local is not None else None, i, C.byref(c) if c is not None else None,
                                    S._p(buf) if buf is not None else None, byte_buf.size if nb is None else nb), "rsrt_display_colour_srgb8")
    build = lambda n, p: st._check(L.rsrt_colour_lut_build(st._ctx, n, C.byref(p) if p is not None else None, None), "rsrt_colour_lut_build")  # noqa: E731
    upload = lambda n, a, nf=None: st._check(L.rsrt_colour_lut_upload(st._ctx, n, S._p(a) if a is not None else None, (a.size if a is not None else 0) if nf is None else nf),  # noqa: E731
                                             "rsrt_colour_lut_upload")
    show(0, 4, 1.5, cp((2, 1, 0.5), 1.0))
    raises(INVALID, lambda: meter(7, 4))  # unknown source
    raises(INVALID, lambda: meter(0, 0))  # sample_total 0 under the mean
    raises(INVALID, lambda: show(7, 4, 1.5, cp()))
    raises(INVALID, lambda: show(0, 0, 1.5, cp()))
    for e in (0.0, -1.0, float("nan"), float("inf")):
        raises(INVALID, lambda: show(0, 4, e, cp()))
    raises(INVALID, lambda: down(None))  # NULL params, bad params
    for kw in ({"gate": 0}, {"gate": 32}, {"iterations": 9}, {"min_permille": 1001}, {"strength": 1.5}, {"strength": float("nan")}, {"max_stops": 4.5}, {"blend": -0.1},
               {"previous": (0.0, 1.0, 1.0)}, {"previous": (1.0, float("inf"), 1.0)}):
        raises(INVALID, lambda: down(wp(**kw)))
    bad = wp()
    bad.flags = 1
    raises(INVALID, lambda: down(bad))
    raises(INVALID, lambda: down(wp(), n=4096))  # a wrong n_words
    raises(INVALID, lambda: down(wp(), n=257))
    down(wp(), buf=None)  # (a NULL host_hist asks for nothing)
    raises(INVALID, lambda: show(0, 4, 1.5, None))  # NULL colour, bad colour
    for c in (cp((0, 1, 1)), cp((1, -1, 1)), cp((1, 1, float("nan"))), cp((float("inf"), 1, 1)), cp(strength=1.5), cp(strength=-0.5), cp(strength=float("nan")), cp(flags=1)):
        raises(INVALID, lambda: show(0, 4, 1.5, c))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), local=S.LocalParams(-0.1, 0.5, 0.18, 4.0, 0, 0)))  # bad local params
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), local=S.LocalParams(0.5, 0.5, 0.18, 4.0, 1, 0)))
    for i in (-0.5, float("nan"), float("inf")):
        raises(INVALID, lambda: show(0, 4, 1.5, cp(), i=i))
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), nb=byte_buf.size // 4))  # a wrong n_bytes, a NULL buffer
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), buf=None))
    st.local_exposure_reset()
    st.bloom_reset()
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), local=S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)))  # no grid, no bloom image: needed only when asked for
    raises(NOT_READY, lambda: show(0, 4, 1.5, cp(), i=0.5))
    show(0, 4, 1.5, cp())
    st.local_exposure("upsampled", 8)
    raises(INVALID, lambda: show(0, 4, 1.5, cp(), local=S.LocalParams(0.5, 0.5, 0.18, 4.0, 0, 0)))  # a grid of another size than the source
    ident = S.CdlParams.of()
    for n in (0, 1, 4, 16, 32, 64, 66, 0xffffffff):  # an unsupported n
        raises(INVALID, lambda: build(n, ident))
        raises(INVALID, lambda: upload(n, np.zeros(3 * 8, F)))
    raises(INVALID, lambda: build(3, None))
    for kw in ({"slope": 16.5}, {"slope": (1.0, -0.1, 1.0)}, {"offset": 1.5}, {"power": 0.2}, {"power": float("nan")}, {"saturation": 4.5}, {"flags": 1}):
        raises(INVALID, lambda: build(3, S.CdlParams.of(**kw)))
    good = np.full(3 * 8, 0.5, F)
    raises(INVALID, lambda: upload(2, good, nf=good.size - 1))  # a wrong n_floats, a NULL buffer
    raises(INVALID, lambda: upload(2, None, nf=24))
    for v in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):  # an out-of-range upload
        a = good.copy()
        a[-1] = v
        raises(INVALID, lambda: upload(2, a))
    short = np.zeros(5, F)
    raises(INVALID, lambda: st._check(L.rsrt_colour_lut_download(st._ctx, S._p(short), short.size, None), "rsrt_colour_lut_download"))
    st.set_partition(0, 2)
    for call in (st.white_meter, st.white_download, st.white_reset, st.colour_lut, st.colour_lut_download, st.colour_lut_reset, lambda: st.colour_lut_upload(lut0),
                 lambda: st.display_colour_srgb8("mean", 1.5, white=(1, 1, 1), lut_strength=0.0)):
        raises(INVALID, call)
    st.set_partition(0, 1)
    # after all that: the same histogram and the same LUT, and a display that still works
    assert np.array_equal(st.white_download()[0], h0) and same(st.colour_lut_download(), lut0)
    assert np.array_equal(st.display_colour_srgb8("mean", 1.5, white=(2, 1, 0.5), lut_strength=1.0), colour_ref.display(img, total, 1.5, (2, 1, 0.5), lut0, 1.0))
    # a reset drops each; the images stay
    st.white_reset()
    st.colour_lut_reset()
    raises(NOT_READY, st.white_download)
    raises(NOT_READY, st.colour_lut_download)
    assert same(st.download(), img)


def test_auto_white_balance_adapts_through_blend_and_white_reset_forgets():
    h, w = 40, 60
    warm = colour_ref.near_grey_frame(h, w, seed=1, tint=(1.8, 1.0, 0.5))
    cool = colour_ref.near_grey_frame(h, w, seed=2, tint=(0.6, 1.0, 1.7))
    st = R.State()
    try:
        a, b = DeviceArray(warm), DeviceArray(cool)
        st.bind_accumulator(a.data_ptr(), w, h)
        st.sample_count = 1
        assert st.white is None
        r0 = st.auto_white_balance()
        t_warm = colour_ref.from_histogram(colour_ref.histogram(warm, 1))
        assert r0["estimated"] and same(F(r0["white"]), t_warm["white"]) and same(F(st.white), t_warm["white"])  # the first call takes the target
        assert r0["white"][0] < r0["white"][1] < r0["white"][2]  # a warm cast: red down, blue up
        st.bind_accumulator(b.data_ptr(), w, h)
        hist = colour_ref.histogram(cool, 1)
        r1 = st.auto_white_balance(blend=0.25)
        want = colour_ref.from_histogram(hist, blend=0.25, previous=tuple(t_warm["white"]))
        assert same(F(r1["white"]), want["white"]) and same(F(r1["target"]), want["target"]) and same(F(st.white), want["white"])
        assert t_warm["white"][0] < want["white"][0] < want["target"][0]  # a quarter of the way
        # display_colour_srgb8 takes the remembered white point
        assert np.array_equal(st.display_colour_srgb8("mean", 1.0), colour_ref.display(cool, 1, 1.0, want["white"]))
        st.white_reset()
        assert st.white is None
        raises(NOT_READY, st.white_download)
        assert np.array_equal(st.display_colour_srgb8("mean", 1.0), st.display_exposed_srgb8("mean", 1.0))  # no white point: 1
        r2 = st.auto_white_balance(blend=0.25)  # nothing remembered: the target again, whatever the blend
        assert same(F(r2["white"]), colour_ref.from_histogram(hist)["white"])
    finally:
        st.close()


def test_cpp_state_balances_and_grades_like_the_python_state(tmp_path):
    import test_colour
    exe = test_colour.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", "4", "17"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    hexf = lambda v: ["%08x" % int(x) for x in np.asarray(v, F).view(np.uint32)]  # noqa: E731
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        assert ["exposure"] + hexf([e]) in lines
        r0 = st.auto_white_balance()
        assert next(f for f in lines if f[0] == "white")[1:] == hexf(r0["white"]) + [str(r0["gated"])]
        hist = st.white_download()[0]
        assert np.array_equal(hist, colour_ref.histogram(st.download(), 4))
        assert next(f for f in lines if f[0] == "hist")[1:] == ["4097", "%016x" % fnv1a(hist.tobytes())]
        shown = st.display_colour_srgb8()
        assert np.array_equal(shown, colour_ref.display(st.download(), 4, e, r0["white"]))
        assert next(f for f in lines if f[0] == "balanced")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        st.colour_lut((1.1, 1.0, 1.0), (0.0, 0.0, -0.03), (1.0, 1.2, 1.0), 1.25, size=17)
        lut = st.colour_lut_download()
        assert next(f for f in lines if f[0] == "lut")[1:] == ["17", "%016x" % fnv1a(lut.tobytes())]
        shown = st.display_colour_srgb8()
        assert np.array_equal(shown, colour_ref.display(st.download(), 4, e, r0["white"], lut, 1.0))
        assert next(f for f in lines if f[0] == "graded")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        r1 = st.auto_white_balance(blend=0.25)
        assert next(f for f in lines if f[0] == "blended")[1:] == hexf(r1["white"])
        assert ["white1", "yes"] in lines and ["reset", "yes"] in lines
    finally:
        st.close()
