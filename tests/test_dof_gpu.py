"""Depth of field on the GPU (rsrt_dof, rsrt_dof_download, rsrt_dof_coc_download, rsrt_dof_depth_at): the lens image and the blur radii
against the numpy restatement (tests/dof_ref.py), bit for bit, on frames around the gather kernel's tile and its halo, with special
pixels and with tiles wholly in focus beside tiles that are not; every source where it lives, with no effect on any other image; the
lens image as the source of the meter, bloom, local exposure and their displays; autofocus; the documented refusals and what they
leave; the drop rule; a caller's stream and output; stale scratch; the Python and the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bloom_ref
import dof_ref
import exposure_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, bound, hip_runtime_path, state
from test_temporal_gpu import accumulate
from test_bloom_gpu import denoised, everything, fnv1a, raises, upsampled
from test_dof import tile_constants

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
TW, TH = tile_constants()
same = util.same_bits_or_nan
FOCUS = 2.0


def frames(r):
    """One pixel under and over the tile; one over the tile and its halo; several tiles each way that are a multiple of nothing; one
    pixel; a frame smaller than the radius each way."""
    return list(dict.fromkeys([(TH - 1, TW - 1), (TH + 1, TW + 1), (TH + 2 * r + 1, TW + 2 * r + 1), (2 * TH + 7, 3 * TW + 5), (1, 1),
                               (max(1, r - 1), max(1, r - 2))]))


CASES = [(r, h, w) for r in (1, 4, 16) for h, w in frames(r)]


def bound_frame(h, w, seed):
    sums, rec, cam, _ = dof_ref.synthetic(h, w, seed, focus_distance=FOCUS, tile=TH)
    st, acc, aov = bound(h, w, sums, rec)
    st.camera = dof_ref.camera_record(cam)
    return st, acc, aov, sums, rec, cam


@pytest.mark.parametrize("radius,h,w", CASES)
def test_device_lens_image_and_radii_equal_the_numpy_restatement_bit_for_bit(radius, h, w):
    st, acc, aov, sums, rec, cam = bound_frame(h, w, seed=1000 * h + w)
    try:
        if h > 2 * TH and radius < TH:  # tiles wholly in focus beside tiles at the full radius: the loop bound shrinks and does not
            reach = np.ceil(np.abs(dof_ref.coc(rec, cam, FOCUS, 0.4, radius)))
            per_tile = [reach[y:y + TH, x:x + TW].max() for y in range(0, h, TH) for x in range(0, w, TW)]
            assert min(per_tile) <= 1 and max(per_tile) == radius
        for total, aperture in ((3, 0.4), (1, 0.05), (3, 0.0)):
            st.depth_of_field("mean", FOCUS, aperture, radius, sample_total=total)
            got, r = st.dof_download(), st.dof_coc()
            want, want_r = dof_ref.dof(sums, total, rec, cam, FOCUS, aperture, radius)
            assert r.shape == want_r.shape and same(r, want_r), (total, aperture)
            assert got.shape == want.shape and same(got, want), (total, aperture)
            if aperture == 0.0:
                assert same(got[..., :3], (sums[..., :3] / F(total)).astype(F))
        assert same(acc.numpy(), sums) and same(aov.numpy(), rec)  # the kernels read only
    finally:
        st.close()


@pytest.fixture(scope="module")
def rendered():
    """A small real render with every image the library can hold: (state, {source: (its download, total, its records)})."""
    w, h = 48, 32
    sc, st = state("default", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)  # accumulator + AOV (4 spp), the guide, the denoised and the upsampled (96 x 64) image
    accumulate(st, 4)                       # a first temporal frame of the same accumulator and AOV buffer
    st.exposure_meter()
    aov, guide = st.download_aov(), st.download_guide()
    images = {"mean": (st.download(), 4, aov), "denoised": (denoised(st), 1, aov), "temporal": (st.download_temporal(), 1, aov),
              "upsampled": (upsampled(st), 1, guide)}
    yield st, images
    st.close()


def test_each_source_is_blurred_where_it_lives_and_nothing_else_changes(rendered):
    st, images = rendered
    cam = dof_ref.Camera.from_record(st.camera)
    before = everything(st)
    assert images["upsampled"][0].shape == (64, 96, 4) and images["mean"][0].shape == (32, 48, 4)
    centre = dof_ref.depth(images["mean"][2], cam)[16, 24]
    assert np.isfinite(centre) and centre > 0
    lens = {}
    for source, (img, total, rec) in images.items():
        for focus, aperture, radius in ((1.0, 0.01, 8), (float(centre), 0.2, 6)):
            st.depth_of_field(source, focus, aperture, radius)
            got, r = st.dof_download(), st.dof_coc()
            want, want_r = dof_ref.dof(img, total, rec, cam, focus, aperture, radius)
            assert got.shape == img.shape and same(r, want_r) and same(got, want), (source, focus)
        lens[source] = got
        assert (r != 0).any() and not same(got[..., :3], (img[..., :3] / F(total)).astype(F)), source  # something is blurred
    assert not same(lens["mean"], lens["denoised"])
    st.depth_of_field("temporal", float(centre), 0.2, 6, sample_total=0)  # sample_total is ignored for all sources but the mean
    assert same(st.dof_download(), lens["temporal"])
    for a, b in zip(before, everything(st)):
        assert same(a, b)


@pytest.mark.parametrize("source", ["mean", "upsampled"])
def test_the_lens_image_is_a_source_of_the_later_passes(rendered, source):
    st, images = rendered
    img, total, rec = images[source]
    cam = dof_ref.Camera.from_record(st.camera)
    st.depth_of_field(source, 3.0, 0.15, 5)
    lens = st.dof_download()
    assert same(lens, dof_ref.dof(img, total, rec, cam, 3.0, 0.15, 5)[0]) and lens.shape == img.shape
    st.exposure_meter("lens")
    hist, _ = st.exposure_download()
    assert np.array_equal(hist, exposure_ref.histogram(lens, 1))
    e = 1.7
    shown = st.display_exposed_srgb8("lens", e)
    assert shown.shape == lens.shape and np.array_equal(shown, exposure_ref.display(lens, 1, e))
    st.bloom("lens", e, levels=3, threshold=0.5)
    b = st.bloom_download()
    assert same(b, bloom_ref.bloom(lens, 1, e, 3, 0.5))
    assert np.array_equal(st.display_bloomed_srgb8("lens", e, 0.4), bloom_ref.display(lens, 1, e, 0.4, b))
    st.local_exposure("lens", 16)
    grid, cell = st.local_exposure_download()
    want_grid = local_ref.grid_of(lens, 1, 16)
    assert cell == 16 and np.array_equal(grid, want_grid)
    gain = local_ref.gains(lens, 1, e, want_grid, 16)
    assert same(st.local_gain("lens", e), gain)
    assert np.array_equal(st.display_local_srgb8("lens", e), local_ref.display(lens, 1, e, gain))
    assert np.array_equal(st.display_local_srgb8("lens", e, bloom_intensity=0.4), local_ref.display(lens, 1, e, gain, 0.4, b))
    st.depth_of_field(source, 3.0, 0.15, 5, sample_total=total)  # the later passes wrote nothing of the pass's
    assert same(st.dof_download(), lens)
    st.bloom_reset()
    st.local_exposure_reset()


def test_focus_at_is_the_records_depth_and_is_remembered(rendered):
    st, images = rendered
    cam = dof_ref.Camera.from_record(st.camera)
    st.focus_distance = None
    for source, y, x in (("mean", 16, 24), ("mean", 31, 0), ("denoised", 5, 40), ("upsampled", 40, 70), ("upsampled", 63, 95)):
        want = dof_ref.depth(images[source][2], cam)[y, x]
        before = st.focus_distance
        got = st.focus_at(x, y, source)
        assert F(got).view(np.uint32) == want.view(np.uint32), (source, y, x)
        assert st.focus_distance == (got if np.isfinite(got) else before)
    z = dof_ref.depth(images["mean"][2], cam)
    if np.isinf(z).any():  # a sky pixel: inf, and the focus stays
        y, x = [int(v[0]) for v in np.nonzero(np.isinf(z))]
        kept = st.focus_distance
        assert st.focus_at(x, y) == np.inf and st.focus_distance == kept
    kept = st.focus_at(24, 16)
    st.depth_of_field("mean", None, 0.2, 6)  # None: the remembered focus
    assert same(st.dof_download(), dof_ref.dof(images["mean"][0], 4, images["mean"][2], cam, kept, 0.2, 6)[0])
    st.focus_distance = None
    st.depth_of_field("mean", None, 0.2, 6)  # ... else the default
    assert same(st.dof_download(), dof_ref.dof(images["mean"][0], 4, images["mean"][2], cam, 1.0, 0.2, 6)[0])
    # synthetic records: a pixel without a hit is sky, and a hit pixel's depth is the restatement's
    st2, acc, aov, sums, rec, cam2 = bound_frame(TH + 1, TW + 1, seed=5)
    try:
        z = dof_ref.depth(rec, cam2)
        (sy, sx), (hy, hx) = [[int(v[0]) for v in np.nonzero(m)] for m in (np.isinf(z), np.isfinite(z) & (z > 0))]
        st2.focus_distance = 1.25
        assert st2.focus_at(sx, sy) == np.inf and st2.focus_distance == 1.25
        assert F(st2.focus_at(hx, hy)).view(np.uint32) == z[hy, hx].view(np.uint32) and st2.focus_distance == z[hy, hx]
    finally:
        st2.close()


def test_refusals_return_their_status_and_leave_the_lens_image(rendered):
    st, images = rendered
    cam = dof_ref.Camera.from_record(st.camera)
    fresh = R.State()
    try:  # nothing exists yet
        fresh.camera = st.camera.copy()
        for source in ("mean", "denoised", "temporal", "upsampled"):
            raises(NOT_READY, lambda: fresh.depth_of_field(source, sample_total=1))
            raises(NOT_READY, lambda: fresh.focus_at(0, 0, source))
        for call in (fresh.dof_download, fresh.dof_coc, lambda: fresh.exposure_meter("lens"), lambda: fresh.display_exposed_srgb8("lens", 1.0),
                     lambda: fresh.bloom("lens", 1.0), lambda: fresh.local_exposure("lens")):
            raises(NOT_READY, call)
        fresh.resize(8, 8)  # an accumulator, no records
        raises(NOT_READY, lambda: fresh.depth_of_field(sample_total=1))
        raises(NOT_READY, lambda: fresh.focus_at(0, 0))
    finally:
        fresh.close()
    P = R.state.DofParams
    cam_p = R.state._p(st.camera)
    raw = lambda source, total, camera, params, out=None, stream=None: st._check(st._L.rsrt_dof(st._ctx, source, total, camera, params, out, stream), "rsrt_dof")  # noqa: E731
    st.depth_of_field("mean", 3.0, 0.2, 4)
    l0, r0 = st.dof_download(), st.dof_coc()
    assert same(l0, dof_ref.dof(images["mean"][0], 4, images["mean"][2], cam, 3.0, 0.2, 4)[0])
    good = P(3.0, 0.2, 4, 0)
    for radius in (0, 17):
        raises(INVALID, lambda: st.depth_of_field(max_radius=radius))
    for f in (0.0, -1.0, float("nan"), float("inf")):
        raises(INVALID, lambda: st.depth_of_field(focus_distance=f))
    for a in (-0.5, float("nan"), float("inf")):
        raises(INVALID, lambda: st.depth_of_field(aperture=a))
    raises(INVALID, lambda: raw(0, 4, cam_p, C.byref(P(3.0, 0.2, 4, 1))))   # flags
    raises(INVALID, lambda: raw(0, 4, None, C.byref(good)))                 # NULL camera
    raises(INVALID, lambda: raw(0, 4, cam_p, None))                         # NULL params
    raises(INVALID, lambda: raw(4, 4, cam_p, C.byref(good)))                # the lens image as its own source
    raises(INVALID, lambda: raw(7, 4, cam_p, C.byref(good)))                # unknown source
    raises(INVALID, lambda: st.depth_of_field(sample_total=0))              # sample_total 0 under the mean
    spare = DeviceArray(np.zeros((33, 48, 4), F))
    raises(INVALID, lambda: st.depth_of_field(out_ptr=spare.data_ptr() + 4))  # a misaligned output pointer
    z = C.c_float()
    depth_at = lambda source, camera, x, y, out: st._check(st._L.rsrt_dof_depth_at(st._ctx, source, camera, x, y, out), "rsrt_dof_depth_at")  # noqa: E731
    raises(INVALID, lambda: depth_at(0, None, 0, 0, C.byref(z)))
    raises(INVALID, lambda: depth_at(0, cam_p, 0, 0, None))
    raises(INVALID, lambda: depth_at(4, cam_p, 0, 0, C.byref(z)))
    raises(INVALID, lambda: depth_at(7, cam_p, 0, 0, C.byref(z)))
    raises(INVALID, lambda: st.focus_at(48, 0))
    raises(INVALID, lambda: st.focus_at(0, 32))
    raises(INVALID, lambda: st.focus_at(96, 0, "upsampled"))
    short = np.zeros(8, F)
    raises(INVALID, lambda: st._check(st._L.rsrt_dof_download(st._ctx, R.state._p(short), short.size, None, None), "rsrt_dof_download"))
    raises(INVALID, lambda: st._check(st._L.rsrt_dof_coc_download(st._ctx, R.state._p(short), short.size), "rsrt_dof_coc_download"))
    raises(INVALID, lambda: st._check(st._L.rsrt_dof_coc_download(st._ctx, None, 48 * 32), "rsrt_dof_coc_download"))
    # records of another size than their image
    other = DeviceArray(np.zeros((16, 24, 8), F))
    st.bind_aov(other.data_ptr(), 24, 16)
    raises(INVALID, st.depth_of_field)
    raises(INVALID, lambda: st.focus_at(0, 0))
    st.bind_aov(None, 0, 0)
    aov = DeviceArray(images["mean"][2])
    st.bind_aov(aov.data_ptr(), 48, 32)
    st.bind_guide(other.data_ptr(), 24, 16)
    raises(INVALID, lambda: st.depth_of_field("upsampled"))
    st.bind_guide(None, 0, 0)
    raises(NOT_READY, lambda: st.depth_of_field("upsampled"))
    guide = DeviceArray(images["upsampled"][2])
    st.bind_guide(guide.data_ptr(), 96, 64)
    st._bound_records = (aov, guide)  # (they live as long as the state that reads them)
    st.set_partition(0, 2)
    for call in (st.depth_of_field, st.dof_download, st.dof_coc, st.dof_reset, lambda: st.focus_at(0, 0), lambda: st.display_exposed_srgb8("lens", 1.0)):
        raises(INVALID, call)
    st.set_partition(0, 1)
    # after all that: the same lens image and radii of the same size, and passes that still take it
    w, h = C.c_uint32(), C.c_uint32()
    st._check(st._L.rsrt_dof_download(st._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_dof_download")
    assert (w.value, h.value) == (48, 32)
    st._check(st._L.rsrt_dof_download(st._ctx, None, 0, None, C.byref(h)), "rsrt_dof_download")  # either size pointer may be NULL
    st._check(st._L.rsrt_dof_download(st._ctx, None, 0, C.byref(w), None), "rsrt_dof_download")
    assert same(st.dof_download(), l0) and same(st.dof_coc(), r0)
    assert np.array_equal(st.display_exposed_srgb8("lens", 1.5), exposure_ref.display(l0, 1, 1.5))
    # a reset drops it; the images stay
    st.dof_reset()
    for call in (st.dof_download, st.dof_coc, lambda: st.exposure_meter("lens"), lambda: st.display_exposed_srgb8("lens", 1.5)):
        raises(NOT_READY, call)
    assert same(st.download(), images["mean"][0])
    st.depth_of_field("mean", 3.0, 0.2, 4)
    assert same(st.dof_download(), l0)
    st.depth_of_field("upsampled", 3.0, 0.2, 4)  # the bound guide holds the records the library's did
    assert same(st.dof_download(), dof_ref.dof(images["upsampled"][0], 1, images["upsampled"][2], cam, 3.0, 0.2, 4)[0])


def test_a_change_of_the_accumulators_size_drops_the_lens_image():
    h, w = 20, 36
    st, acc, aov, sums, rec, cam = bound_frame(h, w, seed=3)
    other, _ = bloom_ref.synthetic(h, w, seed=4)
    try:
        b = DeviceArray(other)
        st.depth_of_field("mean", FOCUS, 0.3, 5, sample_total=1)
        l0 = st.dof_download()
        assert same(l0, dof_ref.dof(sums, 1, rec, cam, FOCUS, 0.3, 5)[0])
        st.bind_accumulator(b.data_ptr(), w, h)  # the same size: the lens image stays (it is the caller's to rebuild)
        assert same(st.dof_download(), l0)
        st._check(st._L.rsrt_accumulator_bind(st._ctx, None, 0, 0), "rsrt_accumulator_bind")  # no accumulator any more
        raises(NOT_READY, st.dof_download)
        raises(NOT_READY, st.dof_coc)
        st.bind_accumulator(acc.data_ptr(), w, h)
        raises(NOT_READY, st.dof_download)
        raises(NOT_READY, lambda: st.display_exposed_srgb8("lens", 1.0))
        st.depth_of_field("mean", FOCUS, 0.3, 5, sample_total=1)
        assert same(st.dof_download(), l0)
        st.bind_accumulator(acc.data_ptr(), h, w)  # another size
        raises(NOT_READY, st.dof_download)
    finally:
        st.close()
    sc, st = state("default", 32, 16)
    try:
        st.render_samples(2, aov=True)
        st.depth_of_field(aperture=0.2)
        assert st.dof_download().shape == (16, 32, 4)
        st.resize(48, 24)
        raises(NOT_READY, st.dof_download)
        raises(NOT_READY, lambda: st.exposure_meter("lens"))
        st.render_samples(2, aov=True)
        st.depth_of_field(aperture=0.2)
        want = dof_ref.dof(st.download(), 2, st.download_aov(), dof_ref.Camera.from_record(st.camera), 1.0, 0.2, 8)[0]
        assert same(st.dof_download(), want)
    finally:
        st.close()


def test_a_callers_stream_a_callers_output_and_stale_scratch():
    h, w = 2 * TH + 7, 3 * TW + 5
    st, acc, aov, sums, rec, cam = bound_frame(h, w, seed=9)
    hip = C.CDLL(hip_runtime_path())  # a caller stream from the HIP runtime the library itself uses
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        st.depth_of_field("mean", FOCUS, 0.4, 16, sample_total=3)
        own = st.dof_download()
        assert same(own, dof_ref.dof(sums, 3, rec, cam, FOCUS, 0.4, 16)[0])
        st.dof_reset()
        out = DeviceArray(np.full((h, w, 4), 7, F))
        st.depth_of_field("mean", FOCUS, 0.4, 16, sample_total=3, stream=stream.value, out_ptr=out.data_ptr())
        st.synchronize()
        assert same(out.numpy(), own) and same(st.dof_download(), own)
        assert np.array_equal(st.display_exposed_srgb8("lens", 0.5), exposure_ref.display(own, 1, 0.5))  # read from the caller's memory
        # two calls in a row with different radii: the second call's bits, whichever is wider
        for first, second in ((16, 2), (1, 8), (8, 1)):
            st.depth_of_field("mean", FOCUS, 0.4, first, sample_total=3)
            st.depth_of_field("mean", FOCUS, 0.4, second, sample_total=3, stream=stream.value)
            assert same(st.dof_download(), dof_ref.dof(sums, 3, rec, cam, FOCUS, 0.4, second)[0]), (first, second)
        # garbage at the widest radius left in the library's buffers, then the frame at a narrower one, then a smaller frame
        junk = DeviceArray(np.full((h, w, 4), np.nan, F))
        st.bind_accumulator(junk.data_ptr(), w, h)
        st.depth_of_field("mean", FOCUS, 0.4, 16, sample_total=1)
        assert np.isnan(st.dof_download()[..., :3]).all()
        st.bind_accumulator(acc.data_ptr(), w, h)
        st.depth_of_field("mean", FOCUS, 0.4, 4, sample_total=3)
        assert same(st.dof_download(), dof_ref.dof(sums, 3, rec, cam, FOCUS, 0.4, 4)[0])
        st.bind_accumulator(junk.data_ptr(), w, h)
        st.depth_of_field("mean", FOCUS, 0.4, 16, sample_total=1)
        sh, sw = TH + 3, TW + 5
        s2, r2, _, _ = dof_ref.synthetic(sh, sw, 10, focus_distance=FOCUS, tile=TH)
        a2, v2 = DeviceArray(s2), DeviceArray(r2)
        st.bind_accumulator(a2.data_ptr(), sw, sh)
        st.bind_aov(v2.data_ptr(), sw, sh)
        st.depth_of_field("mean", FOCUS, 0.4, 4, sample_total=3)
        assert same(st.dof_download(), dof_ref.dof(s2, 3, r2, cam, FOCUS, 0.4, 4)[0])
    finally:
        st.close()
        hip.hipStreamDestroy(stream)


def test_cpp_state_blurs_like_the_python_state(tmp_path):
    import test_dof
    exe = test_dof.build_cpp_demo(tmp_path)
    w, h, radius = 64, 36, 6
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "4", str(radius)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    word = lambda v: "%08x" % int(np.asarray(v, F).view(np.uint32))  # noqa: E731
    sc, st = state("spheres_only", w, h)
    try:
        st.render_samples(4, aov=True)
        z = st.focus_at(w // 2, h // 2)
        assert ["focus", word(z), word(st.focus_distance or 0.0)] in lines
        st.depth_of_field(aperture=0.05, max_radius=radius)
        lens, coc = st.dof_download(), st.dof_coc()
        cam = dof_ref.Camera.from_record(st.camera)
        want, want_r = dof_ref.dof(st.download(), 4, st.download_aov(), cam, st.focus_distance or 1.0, 0.05, radius)
        assert same(lens, want) and same(coc, want_r) and (coc != 0).any()
        assert next(f for f in lines if f[0] == "lens")[1:] == [str(w), str(h), "%016x" % fnv1a(lens.tobytes())]
        assert next(f for f in lines if f[0] == "coc")[1:] == [str(w * h), "%016x" % fnv1a(coc.tobytes())]
        e = st.auto_exposure("lens")["exposure"]
        assert ["exposure", word(e)] in lines
        st.bloom("lens")
        shown = st.display_bloomed_srgb8("lens")
        assert next(f for f in lines if f[0] == "display")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        assert ["reset", "yes"] in lines
    finally:
        st.close()


PICTURES = {"sharp": [], "lens": ["dof=auto,0.03,12"]}


@pytest.mark.parametrize("which", sorted(PICTURES))
def test_render_png_writes_the_golden_pictures(tmp_path, which):
    """tools/render_png.py on house at 480 x 270, 64 samples, denoised and metered, without and with dof=auto: the two pictures under
    tests/golden/pictures, byte for byte (the whole chain is bit-exact: render, AOV pass, denoiser, lens blur, meter, display, and the
    PNG writer stores the bytes).  The lens run focuses on the picture's centre, the back wall."""
    import os
    import sys
    out = str(tmp_path / "out.png")
    cmd = [sys.executable, os.path.join(util.ROOT, "tools", "render_png.py"), "house", "480", "270", "64", "8", out, "--denoise", "exposure=auto"]
    r = subprocess.run(cmd + PICTURES[which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    if which == "lens":
        assert "focus distance 5.94" in r.stdout and "blur radius: mean" in r.stdout, r.stdout
    golden = os.path.join(util.ROOT, "tests", "golden", "pictures", "dof_house_480x270_%s.png" % which)
    with open(out, "rb") as f, open(golden, "rb") as g:
        assert f.read() == g.read(), which
