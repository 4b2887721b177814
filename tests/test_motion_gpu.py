"""Camera motion blur on the GPU (rsrt_motion_blur, rsrt_motion_download, rsrt_motion_velocity_download, rsrt_motion_tiles_download): the
velocities, the tiles' maxima and the motion image against the numpy restatement (tests/motion_ref.py), bit for bit, on frames below,
around and above a tile with special pixels and with copied tiles beside gathered ones; every source where it lives, with no effect on
any other image; the motion image as the source of the meters, bloom, local exposure and the displays; the documented refusals and
what they leave; the drop rule; a caller's stream and output; the Python and the C++ State; the picture tool."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bloom_ref
import exposure_ref
import local_ref
import motion_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, bound, hip_runtime_path, state
from test_temporal_gpu import accumulate
from test_bloom_gpu import denoised, everything, fnv1a, raises, upsampled

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
same = util.same_bits_or_nan
CASES = [(r, t, h, w) for h, w in ((3, 5), (17, 33), (40, 56)) for r in (1, 4, 16) for t in (2, 16)]


def bound_frame(h, w, seed):
    sums, rec, cam, prev, _ = motion_ref.synthetic(h, w, seed)
    st, acc, aov = bound(h, w, sums, rec)
    st.camera = motion_ref.camera_record(cam)
    return st, acc, aov, sums, rec, cam, prev


def results(st):
    return st.motion_download(), st.motion_velocity(), st.motion_tiles()


def agree(got, want):
    return all(g.shape == w.shape and same(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("radius,taps,h,w", CASES)
def test_device_velocities_tile_maxima_and_motion_image_equal_the_numpy_restatement_bit_for_bit(radius, taps, h, w):
    st, acc, aov, sums, rec, cam, prev = bound_frame(h, w, seed=1000 * h + w)
    try:
        previous = motion_ref.camera_record(prev)
        for total, shutter in ((1, 0.5), (3, 1.0), (3, 0.0)):
            st.motion_blur("mean", previous, shutter, radius, taps, sample_total=total)
            want = motion_ref.motion(sums, total, rec, cam, prev, shutter, radius, taps)
            assert agree(results(st), want), (total, shutter)
            if shutter == 0.0:
                assert same(want[0][..., :3], (sums[..., :3] / F(total)).astype(F)) and not want[2].any()
        if (h, w) == (40, 56):  # copied tiles beside gathered ones
            near = motion_ref.neighbour_max(motion_ref.motion(sums, 1, rec, cam, prev, 0.5, radius, taps)[2])[..., 2]
            assert (near < 0.5).any() and (near >= 0.5).any()
        st.motion_blur("mean", st.camera, 1.0, radius, taps, sample_total=3)  # the same camera: the source, and not one velocity
        img, uvl, tiles = results(st)
        assert same(img[..., :3], (sums[..., :3] / F(3)).astype(F)) and (img[..., 3] == 1).all() and not uvl.any() and not tiles.any()
        assert same(acc.numpy(), sums) and same(aov.numpy(), rec)  # the kernels read only
    finally:
        st.close()


@pytest.fixture(scope="module")
def rendered():
    """A 160 x 90 house frame with every image the library can hold: (state, {source: (its download, total, its records)}, the camera
    one frame earlier)."""
    w, h = 160, 90
    sc, st = state("house", w, h)
    st.render_upsampled(2 * w, 2 * h, n=4)  # accumulator + AOV (4 spp), the guide, the denoised and the upsampled (320 x 180) image
    accumulate(st, 4)                       # a first temporal frame of the same accumulator and AOV buffer
    st.exposure_meter()
    aov, guide = st.download_aov(), st.download_guide()
    st.depth_of_field("mean", 3.0, 0.05, 6)
    images = {"mean": (st.download(), 4, aov), "denoised": (denoised(st), 1, aov), "temporal": (st.download_temporal(), 1, aov),
              "upsampled": (upsampled(st), 1, guide), "lens": (st.dof_download(), 1, aov)}
    yield st, images, R.state.camera_earlier(st.camera, 0.05, 0.1)
    st.close()


def test_each_source_is_blurred_where_it_lives_and_nothing_else_changes(rendered):
    st, images, previous = rendered
    cam, prev = motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous)
    before = everything(st) + [st.dof_download(), st.dof_coc()]
    assert images["upsampled"][0].shape == (180, 320, 4) and images["mean"][0].shape == (90, 160, 4)
    blurred = {}
    for source, (img, total, rec) in images.items():
        for shutter, radius, taps in ((0.5, 16, 16), (1.0, 5, 6)):
            st.motion_blur(source, previous, shutter, radius, taps)
            got = results(st)
            assert agree(got, motion_ref.motion(img, total, rec, cam, prev, shutter, radius, taps)), (source, shutter)
        blurred[source] = got[0]
        assert (got[1][..., 2] >= 0.5).any() and not same(got[0][..., :3], (img[..., :3] / F(total)).astype(F)), source  # something is blurred
    assert not same(blurred["mean"], blurred["denoised"]) and not same(blurred["mean"], blurred["lens"])
    st.motion_blur("temporal", previous, 1.0, 5, 6, sample_total=0)  # sample_total is ignored for all sources but the mean
    assert same(st.motion_download(), blurred["temporal"])
    # the lens image of the upsampled image is blurred with the guide, the records it was built from
    st.depth_of_field("upsampled", 3.0, 0.05, 6)
    lens_up = st.dof_download()
    st.motion_blur("lens", previous)
    assert agree(results(st), motion_ref.motion(lens_up, 1, images["upsampled"][2], cam, prev))
    st.depth_of_field("mean", 3.0, 0.05, 6)
    for a, b in zip(before, everything(st) + [st.dof_download(), st.dof_coc()]):
        assert same(a, b)
    # the lens goes before the shutter: rsrt_dof refuses the motion image
    raises(INVALID, lambda: st._check(st._L.rsrt_dof(st._ctx, 5, 4, R.state._p(st.camera), C.byref(R.state.DofParams(1.0, 0.01, 8, 0)), None, None), "rsrt_dof"))


def later_passes(st, source, e):
    """What the passes after the shutter make of `source`: the two histograms, the bloom image, the grid and the five displays."""
    st.exposure_meter(source)
    out = [st.exposure_download()[0]]
    st.white_meter(source)
    out.append(st.white_download()[0])
    st.bloom(source, e, levels=3, threshold=0.5)
    out.append(st.bloom_download())
    st.local_exposure(source, 16)
    out.append(st.local_exposure_download()[0])
    out += [st.display_exposed_srgb8(source, e), st.display_bloomed_srgb8(source, e, 0.4), st.display_local_srgb8(source, e, bloom_intensity=0.4),
            st.local_gain(source, e), st.display_colour_srgb8(source, e, white=(1.2, 1.0, 0.8), lut_strength=0.0, shadows=0.5, bloom_intensity=0.4)]
    return out


@pytest.mark.parametrize("source", ["mean", "upsampled", "lens"])
def test_the_motion_image_is_a_source_of_the_later_passes(rendered, source):
    st, images, previous = rendered
    img, total, rec = images[source]
    cam, prev = motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous)
    e = 1.7
    # with `previous` equal to the camera: what those passes give for the motion image's own source
    st.motion_blur(source, st.camera)
    assert same(st.motion_download()[..., :3], (img[..., :3] / F(total)).astype(F))
    for a, b in zip(later_passes(st, "motion", e), later_passes(st, source, e)):
        assert a.shape == b.shape and (np.array_equal(a, b) if a.dtype != F else same(a, b))
    # with a camera that moved: the restatements of those passes on the restated motion image
    st.motion_blur(source, previous, 0.5, 8, 8)
    blurred = st.motion_download()
    assert same(blurred, motion_ref.motion(img, total, rec, cam, prev, 0.5, 8, 8)[0]) and blurred.shape == img.shape
    hist, _, b, grid, shown, bloomed, graded, gain, _ = later_passes(st, "motion", e)
    assert np.array_equal(hist, exposure_ref.histogram(blurred, 1))
    assert shown.shape == blurred.shape and np.array_equal(shown, exposure_ref.display(blurred, 1, e))
    assert same(b, bloom_ref.bloom(blurred, 1, e, 3, 0.5)) and np.array_equal(bloomed, bloom_ref.display(blurred, 1, e, 0.4, b))
    want_grid = local_ref.grid_of(blurred, 1, 16)
    want_gain = local_ref.gains(blurred, 1, e, want_grid, 16)
    assert np.array_equal(grid, want_grid) and same(gain, want_gain)
    assert np.array_equal(graded, local_ref.display(blurred, 1, e, want_gain, 0.4, b))
    st.motion_blur(source, previous, 0.5, 8, 8, sample_total=total)  # the later passes wrote nothing of the pass's
    assert same(st.motion_download(), blurred)
    st.bloom_reset()
    st.local_exposure_reset()


def test_previous_none_is_the_camera_of_the_last_call(rendered):
    st, images, previous = rendered
    img, total, rec = images["mean"]
    cam, prev = motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous)
    now = st.camera.copy()
    try:
        st.motion_reset()
        assert st.motion_camera is None
        st.camera = previous.copy()
        st.motion_blur()  # the first call: the current camera, and the output is the source
        assert same(st.motion_download()[..., :3], (img[..., :3] / F(total)).astype(F)) and not st.motion_velocity().any()
        st.camera = now.copy()
        st.motion_blur()  # after the camera of the call before
        assert agree(results(st), motion_ref.motion(img, total, rec, cam, prev))
        st.motion_blur()  # held still
        assert not st.motion_velocity().any()
        st.motion_reset()
        raises(NOT_READY, st.motion_download)
        assert st.motion_camera is None
    finally:
        st.camera = now


def test_refusals_return_their_status_and_leave_the_motion_image(rendered):
    st, images, previous = rendered
    cam, prev = motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous)
    fresh = R.State()
    try:  # nothing exists yet
        fresh.camera = st.camera.copy()
        for source in ("mean", "denoised", "temporal", "upsampled", "lens"):
            raises(NOT_READY, lambda: fresh.motion_blur(source, sample_total=1))
        for call in (fresh.motion_download, fresh.motion_velocity, fresh.motion_tiles, lambda: fresh.exposure_meter("motion"), lambda: fresh.white_meter("motion"),
                     lambda: fresh.display_exposed_srgb8("motion", 1.0), lambda: fresh.bloom("motion", 1.0), lambda: fresh.local_exposure("motion"),
                     lambda: fresh.display_colour_srgb8("motion", 1.0, lut_strength=0.0)):
            raises(NOT_READY, call)
        fresh.resize(8, 8)  # an accumulator, no records
        raises(NOT_READY, lambda: fresh.motion_blur(sample_total=1))
        assert fresh.motion_camera is None  # a refused call remembers nothing
    finally:
        fresh.close()
    P = R.state.MotionParams
    cam_p, prev_p = R.state._p(st.camera), R.state._p(previous)
    raw = lambda source, total, camera, prev_, params, out=None, stream=None: st._check(  # noqa: E731
        st._L.rsrt_motion_blur(st._ctx, source, total, camera, prev_, params, out, stream), "rsrt_motion_blur")
    st.motion_blur("mean", previous, 0.5, 4, 8)
    m0 = results(st)
    assert agree(m0, motion_ref.motion(images["mean"][0], 4, images["mean"][2], cam, prev, 0.5, 4, 8))
    good = P(0.5, 4, 8, 0)
    for radius in (0, 17):
        raises(INVALID, lambda: st.motion_blur(previous=previous, max_radius=radius))
    for s in (-0.5, 1.5, float("nan"), float("inf")):
        raises(INVALID, lambda: st.motion_blur(previous=previous, shutter=s))
    for t in (0, 1, 7, 34):
        raises(INVALID, lambda: st.motion_blur(previous=previous, taps=t))
    raises(INVALID, lambda: raw(0, 4, cam_p, prev_p, C.byref(P(0.5, 4, 8, 1))))  # flags
    raises(INVALID, lambda: raw(0, 4, None, prev_p, C.byref(good)))              # NULL camera
    raises(INVALID, lambda: raw(0, 4, cam_p, None, C.byref(good)))               # NULL previous
    raises(INVALID, lambda: raw(0, 4, cam_p, prev_p, None))                      # NULL params
    raises(INVALID, lambda: raw(5, 4, cam_p, prev_p, C.byref(good)))             # the motion image as its own source
    raises(INVALID, lambda: raw(7, 4, cam_p, prev_p, C.byref(good)))             # unknown source
    raises(INVALID, lambda: st.motion_blur(previous=previous, sample_total=0))   # sample_total 0 under the mean
    spare = DeviceArray(np.zeros((91, 160, 4), F))
    raises(INVALID, lambda: st.motion_blur(previous=previous, out_ptr=spare.data_ptr() + 4))  # a misaligned output pointer
    short = np.zeros(8, F)
    raises(INVALID, lambda: st._check(st._L.rsrt_motion_download(st._ctx, R.state._p(short), short.size, None, None), "rsrt_motion_download"))
    raises(INVALID, lambda: st._check(st._L.rsrt_motion_velocity_download(st._ctx, R.state._p(short), short.size), "rsrt_motion_velocity_download"))
    raises(INVALID, lambda: st._check(st._L.rsrt_motion_velocity_download(st._ctx, None, 160 * 90 * 3), "rsrt_motion_velocity_download"))
    raises(INVALID, lambda: st._check(st._L.rsrt_motion_tiles_download(st._ctx, R.state._p(short), short.size, None, None), "rsrt_motion_tiles_download"))
    # records of another size than their image
    other = DeviceArray(np.zeros((16, 24, 8), F))
    st.bind_aov(other.data_ptr(), 24, 16)
    raises(INVALID, lambda: st.motion_blur(previous=previous))
    raises(INVALID, lambda: st.motion_blur("lens", previous))  # the lens image was built from the AOV buffer
    st.bind_aov(None, 0, 0)
    raises(NOT_READY, lambda: st.motion_blur("lens", previous))
    aov = DeviceArray(images["mean"][2])
    st.bind_aov(aov.data_ptr(), 160, 90)
    st.bind_guide(other.data_ptr(), 24, 16)
    raises(INVALID, lambda: st.motion_blur("upsampled", previous))
    st.bind_guide(None, 0, 0)
    raises(NOT_READY, lambda: st.motion_blur("upsampled", previous))
    guide = DeviceArray(images["upsampled"][2])
    st.bind_guide(guide.data_ptr(), 320, 180)
    st._bound_records = (aov, guide)  # (they live as long as the state that reads them)
    st.set_partition(0, 2)
    for call in (lambda: st.motion_blur(previous=previous), st.motion_download, st.motion_velocity, st.motion_tiles, st.motion_reset,
                 lambda: st.display_exposed_srgb8("motion", 1.0)):
        raises(INVALID, call)
    st.set_partition(0, 1)
    # after all that: the same motion image, velocities and tile maxima, and passes that still take it
    w, h = C.c_uint32(), C.c_uint32()
    st._check(st._L.rsrt_motion_download(st._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_motion_download")
    assert (w.value, h.value) == (160, 90)
    st._check(st._L.rsrt_motion_download(st._ctx, None, 0, None, C.byref(h)), "rsrt_motion_download")  # either size pointer may be NULL
    st._check(st._L.rsrt_motion_tiles_download(st._ctx, None, 0, C.byref(w), None), "rsrt_motion_tiles_download")
    assert w.value == 10
    assert agree(results(st), m0)
    assert np.array_equal(st.display_exposed_srgb8("motion", 1.5), exposure_ref.display(m0[0], 1, 1.5))
    # a reset drops it; the images stay
    st.motion_reset()
    for call in (st.motion_download, st.motion_velocity, st.motion_tiles, lambda: st.exposure_meter("motion"), lambda: st.display_exposed_srgb8("motion", 1.5)):
        raises(NOT_READY, call)
    assert same(st.download(), images["mean"][0]) and same(st.dof_download(), images["lens"][0])
    st.motion_blur("mean", previous, 0.5, 4, 8)
    assert agree(results(st), m0)
    st.motion_blur("upsampled", previous, 0.5, 4, 8)  # the bound guide holds the records the library's did
    assert agree(results(st), motion_ref.motion(images["upsampled"][0], 1, images["upsampled"][2], cam, prev, 0.5, 4, 8))


def test_a_change_of_the_accumulators_size_drops_the_motion_image():
    h, w = 20, 36
    st, acc, aov, sums, rec, cam, prev = bound_frame(h, w, seed=3)
    other, _ = bloom_ref.synthetic(h, w, seed=4)
    previous = motion_ref.camera_record(prev)
    try:
        b = DeviceArray(other)
        st.motion_blur("mean", previous, 1.0, 5, 8, sample_total=1)
        m0 = results(st)
        assert agree(m0, motion_ref.motion(sums, 1, rec, cam, prev, 1.0, 5, 8))
        st.bind_accumulator(b.data_ptr(), w, h)  # the same size: the motion image stays (it is the caller's to rebuild)
        assert agree(results(st), m0)
        st._check(st._L.rsrt_accumulator_bind(st._ctx, None, 0, 0), "rsrt_accumulator_bind")  # no accumulator any more
        for call in (st.motion_download, st.motion_velocity, st.motion_tiles):
            raises(NOT_READY, call)
        st.bind_accumulator(acc.data_ptr(), w, h)
        raises(NOT_READY, st.motion_download)
        raises(NOT_READY, lambda: st.display_exposed_srgb8("motion", 1.0))
        st.motion_blur("mean", previous, 1.0, 5, 8, sample_total=1)
        assert agree(results(st), m0)
        st.bind_accumulator(acc.data_ptr(), h, w)  # another size
        raises(NOT_READY, st.motion_download)
    finally:
        st.close()
    sc, st = state("default", 32, 16)
    try:
        st.render_samples(2, aov=True)
        previous = R.state.camera_earlier(st.camera, 0.1, 0.2)
        st.motion_blur(previous=previous)
        assert st.motion_download().shape == (16, 32, 4) and st.motion_tiles().shape == (1, 2, 3)
        st.resize(48, 24)
        raises(NOT_READY, st.motion_download)
        raises(NOT_READY, lambda: st.exposure_meter("motion"))
        st.render_samples(2, aov=True)
        st.motion_blur(previous=previous)
        want = motion_ref.motion(st.download(), 2, st.download_aov(), motion_ref.Camera.from_record(st.camera), motion_ref.Camera.from_record(previous))
        assert agree(results(st), want) and want[2].shape == (2, 3, 3)
    finally:
        st.close()


def test_a_callers_stream_a_callers_output_and_stale_scratch():
    h, w = 40, 56
    st, acc, aov, sums, rec, cam, prev = bound_frame(h, w, seed=9)
    previous = motion_ref.camera_record(prev)
    hip = C.CDLL(hip_runtime_path())  # a caller stream from the HIP runtime the library itself uses
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        st.motion_blur("mean", previous, 0.5, 16, 16, sample_total=3)
        own = st.motion_download()
        assert same(own, motion_ref.motion(sums, 3, rec, cam, prev, 0.5, 16, 16)[0])
        st.motion_reset()
        out = DeviceArray(np.full((h, w, 4), 7, F))
        st.motion_blur("mean", previous, 0.5, 16, 16, sample_total=3, stream=stream.value, out_ptr=out.data_ptr())
        st.synchronize()
        assert same(out.numpy(), own) and same(st.motion_download(), own)
        assert np.array_equal(st.display_exposed_srgb8("motion", 0.5), exposure_ref.display(own, 1, 0.5))  # read from the caller's memory
        # two calls in a row with different radii: the second call's bits, whichever is wider
        for first, second in ((16, 2), (1, 8), (8, 1)):
            st.motion_blur("mean", previous, 0.5, first, 16, sample_total=3)
            st.motion_blur("mean", previous, 0.5, second, 16, sample_total=3, stream=stream.value)
            assert agree(results(st), motion_ref.motion(sums, 3, rec, cam, prev, 0.5, second, 16)), (first, second)
        # garbage left in the library's buffers, then a smaller frame
        junk = DeviceArray(np.full((h, w, 4), np.nan, F))
        st.bind_accumulator(junk.data_ptr(), w, h)
        st.motion_blur("mean", previous, 0.5, 16, 16, sample_total=1)
        assert np.isnan(st.motion_download()[..., :3]).all()
        sh, sw = 19, 21
        s2, r2, _, _, _ = motion_ref.synthetic(sh, sw, 10)
        a2, v2 = DeviceArray(s2), DeviceArray(r2)
        st.bind_accumulator(a2.data_ptr(), sw, sh)
        st.bind_aov(v2.data_ptr(), sw, sh)
        st.motion_blur("mean", previous, 0.5, 4, 16, sample_total=3)
        assert agree(results(st), motion_ref.motion(s2, 3, r2, cam, prev, 0.5, 4, 16))
    finally:
        st.close()
        hip.hipStreamDestroy(stream)


def test_cpp_state_blurs_like_the_python_state(tmp_path):
    import test_motion
    exe = test_motion.build_cpp_demo(tmp_path)
    w, h, radius, step = 64, 36, 6, 0.05
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "4", str(radius), str(step)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    word = lambda v: "%08x" % int(np.asarray(v, F).view(np.uint32))  # noqa: E731
    sc, st = state("spheres_only", w, h)
    try:
        st.render_samples(4, aov=True)
        st.motion_blur(max_radius=radius)
        still = st.motion_download()
        assert same(still[..., :3], (st.download()[..., :3] / F(4)).astype(F))
        assert ["still", "%016x" % fnv1a(still.tobytes())] in lines
        first = motion_ref.Camera.from_record(st.camera)
        desc = sc.camera_desc.copy()
        desc["yaw"] = F(desc["yaw"][0]) + F(step)
        st.camera = R.camera_uniform(desc)
        st.render_samples(4, aov=True)
        st.motion_blur(max_radius=radius)
        img, uvl, tiles = results(st)
        want = motion_ref.motion(st.download(), 4, st.download_aov(), motion_ref.Camera.from_record(st.camera), first, 0.5, radius, 16)
        assert agree((img, uvl, tiles), want) and (uvl[..., 2] >= 0.5).any()
        assert next(f for f in lines if f[0] == "motion")[1:] == [str(w), str(h), "%016x" % fnv1a(img.tobytes())]
        assert next(f for f in lines if f[0] == "velocity")[1:] == [str(w * h * 3), "%016x" % fnv1a(uvl.tobytes())]
        assert next(f for f in lines if f[0] == "tiles")[1:] == [str(tiles.shape[1]), str(tiles.shape[0]), "%016x" % fnv1a(tiles.tobytes())]
        e = st.auto_exposure("motion")["exposure"]
        assert ["exposure", word(e)] in lines
        st.bloom("motion")
        shown = st.display_bloomed_srgb8("motion")
        assert next(f for f in lines if f[0] == "display")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        assert ["reset", "yes"] in lines
    finally:
        st.close()


def test_render_png_writes_the_motion_blurred_picture(tmp_path):
    """tools/render_png.py on house at 160 x 90, 8 samples, with motion=4,0: a picture that differs from the sharp one and equals the
    one the same State calls make."""
    import math
    w, h, spp = 160, 90, 8
    tool = [sys.executable, os.path.join(util.ROOT, "tools", "render_png.py"), "house", str(w), str(h), str(spp), "8"]
    pictures = {}
    for which, extra in (("sharp", []), ("motion", ["motion=4,0"])):
        out = str(tmp_path / (which + ".png"))
        r = subprocess.run(tool + [out, "exposure=1.5"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        assert ("blur half-length" in r.stdout) == (which == "motion"), r.stdout
        with open(out, "rb") as f:
            pictures[which] = f.read()
    assert pictures["sharp"] != pictures["motion"]
    sc = R.Scene.load_toml(util.scene_path("house"))
    st = R.State.new(sc, R.Environment.synthetic(2048, 1024), w, h)
    try:
        st.max_bounces = 8
        st.render_samples(spp, aov=True)
        st.motion_blur("mean", R.state.camera_earlier(st.camera, math.radians(4.0), 0.0))
        want = str(tmp_path / "want.png")
        R.host.write_png(want, st.display_exposed_srgb8("motion", 1.5))
        with open(want, "rb") as f:
            assert f.read() == pictures["motion"]
    finally:
        st.close()
