"""Local exposure on the GPU (rsrt_local_exposure, rsrt_local_exposure_download, rsrt_local_gain_download, rsrt_display_local_srgb8):
the blurred grid, the gains and the graded display against the numpy restatement (tests/local_ref.py), bit for bit, on frames around
the splat workgroup's pixel block and the display tile, at three cells, with and without bloom and with special pixels; a grid that
does not depend on what its memory held; every source where it lives, with no effect on any other image; the documented refusals and
what they leave; the drop rule; a caller's stream; the Python and the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bloom_ref
import exposure_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, hip_runtime_path, state
from test_bloom_gpu import denoised, everything, fnv1a, raises, rendered, upsampled  # noqa: F401 (rendered is a fixture)
from test_local import CASES as CPU_CASES, same, seed_of, tile_constants

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32
PW, PH, TW, TH = tile_constants()
# the CPU test's frames; one pixel under and over the splat workgroup's pixel block and the display tile, in each dimension; frames of
# several blocks and tiles each way that are a multiple of nothing
FRAMES = list(dict.fromkeys([(h, w) for h, w, _ in CPU_CASES] + [(PH - 1, PW - 1), (PH + 1, PW + 1), (PH - 1, PW + 1), (PH + 1, PW - 1),
                                                                (TH - 1, TW - 1), (TH + 1, TW + 1), (TH - 1, TW + 1), (TH + 1, TW - 1),
                                                                (4 * TH + 7, 6 * TW + 5), (2 * PH + 7, 3 * PW + 5)]))
PARAMS = ({}, {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0})


def grid_equal(st, want, cell):
    got, c = st.local_exposure_download()
    return c == cell and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("h,w", FRAMES)
def test_device_grid_gains_and_display_equal_the_numpy_restatement_bit_for_bit(h, w):
    sums, _ = local_ref.synthetic(h, w, seed=seed_of(h, w))
    total = 3
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.bloom("mean", 0.37, 3, sample_total=total)
        b = st.bloom_download()
        assert same(b, bloom_ref.bloom(sums, total, 0.37, 3))
        for cell in (8, 32, 64):
            st.local_exposure("mean", cell, sample_total=total)
            grid = local_ref.grid_of(sums, total, cell)
            assert grid_equal(st, grid, cell), cell
            for exposure in (0.37, 40.0):
                for kw in PARAMS:
                    case = (cell, exposure, kw)
                    want = local_ref.gains(sums, total, exposure, grid, cell, **kw)
                    assert same(st.local_gain("mean", exposure, sample_total=total, **kw), want), case
                    assert np.array_equal(st.display_local_srgb8("mean", exposure, sample_total=total, **kw), local_ref.display(sums, total, exposure, want)), case
                    if exposure == 0.37:  # (what the bloom image was built at)
                        assert np.array_equal(st.display_local_srgb8("mean", exposure, bloom_intensity=0.5, sample_total=total, **kw),
                                              local_ref.display(sums, total, exposure, want, 0.5, b)), case
            # strengths 0: the exposed and the bloomed display
            assert np.array_equal(st.display_local_srgb8("mean", 0.37, 0.0, 0.0, sample_total=total), st.display_exposed_srgb8("mean", 0.37, sample_total=total))
            assert np.array_equal(st.display_local_srgb8("mean", 0.37, 0.0, 0.0, bloom_intensity=0.5, sample_total=total),
                                  st.display_bloomed_srgb8("mean", 0.37, 0.5, sample_total=total))
        assert util.same_bits_or_nan(dev.numpy(), sums)  # the kernels read only
    finally:
        st.close()


def test_the_grid_does_not_depend_on_what_its_memory_held():
    """The splat writes every cell and nothing zeroes the buffer: a grid equals a fresh context's whatever was built there before."""
    h, w = PH + 9, 2 * PW + 5
    a, _ = local_ref.synthetic(h, w, seed=21)
    b, _ = local_ref.synthetic(h, w, seed=22)
    small, _ = local_ref.synthetic(TH + 1, TW + 3, seed=23)

    def fresh(sums, cell):
        st = R.State()
        try:
            dev = DeviceArray(sums)
            st.bind_accumulator(dev.data_ptr(), sums.shape[1], sums.shape[0])
            st.local_exposure("mean", cell, sample_total=1)
            return st.local_exposure_download()[0]
        finally:
            st.close()
    want = {cell: fresh(b, cell) for cell in (8, 32, 64)}
    for cell in want:
        assert np.array_equal(want[cell], local_ref.grid_of(b, 1, cell))
    st = R.State()
    try:
        da, db, ds = DeviceArray(a), DeviceArray(b), DeviceArray(small)
        st.bind_accumulator(da.data_ptr(), w, h)
        st.local_exposure("mean", 32, sample_total=1)
        assert grid_equal(st, local_ref.grid_of(a, 1, 32), 32)
        st.bind_accumulator(db.data_ptr(), w, h)  # another frame of the same size
        st.local_exposure("mean", 32, sample_total=1)
        assert grid_equal(st, want[32], 32)
        for cell in (8, 64, 16, 32, 8):  # a change of cell, both ways
            st.local_exposure("mean", cell, sample_total=1)
            assert grid_equal(st, want[cell] if cell in want else local_ref.grid_of(b, 1, cell), cell), cell
        st.bind_accumulator(ds.data_ptr(), small.shape[1], small.shape[0])  # a smaller frame, then the larger one again
        st.local_exposure("mean", 8, sample_total=1)
        assert grid_equal(st, local_ref.grid_of(small, 1, 8), 8)
        st.bind_accumulator(db.data_ptr(), w, h)
        for cell in (64, 8):
            st.local_exposure("mean", cell, sample_total=1)
            assert grid_equal(st, want[cell], cell), cell
    finally:
        st.close()


def everything_and_bloom(st):
    return everything(st) + [st.bloom_download()]


def test_each_source_is_graded_where_it_lives_and_nothing_else_changes(rendered):  # noqa: F811
    st, images = rendered
    st.bloom("mean", 1.5, levels=3)
    before = everything_and_bloom(st)
    assert images["upsampled"][0].shape == (64, 96, 4) and images["mean"][0].shape == (32, 48, 4)
    grids = {}
    for source, (img, total) in images.items():
        for cell in (8, 32):
            st.local_exposure(source, cell)
            grid = local_ref.grid_of(img, total, cell)
            assert grid_equal(st, grid, cell), (source, cell)
            for exposure, kw in ((1.0, {}), (2.5, {"shadows": 1.0, "highlights": 0.75, "max_stops": 3.0}), (0.2, {"key": 0.5})):
                want = local_ref.gains(img, total, exposure, grid, cell, **kw)
                got = st.local_gain(source, exposure, **kw)
                assert got.shape == img.shape[:2] and same(got, want), (source, cell, exposure)
                shown = st.display_local_srgb8(source, exposure, **kw)
                assert shown.shape == img.shape and np.array_equal(shown, local_ref.display(img, total, exposure, want)), (source, cell, exposure)
                assert grid_equal(st, grid, cell)  # the exposure and the params enter at the slice alone
            assert np.array_equal(st.display_local_srgb8(source, 2.5, 0.0, 0.0), st.display_exposed_srgb8(source, 2.5)), source
        grids[source] = grid
        assert (want != 1).any(), source  # something is graded
    assert grids["upsampled"].shape == (32, 2, 3, 2) and grids["mean"].shape == (32, 1, 2, 2)
    assert not np.array_equal(grids["mean"], grids["denoised"])
    st.local_exposure("temporal", 32, sample_total=0)  # sample_total is ignored for all sources but the mean
    assert grid_equal(st, grids["temporal"], 32)
    # the bloom image of the accumulator's size goes with the sources of that size
    st.local_exposure("mean", 32)
    img, total = images["mean"]
    want = local_ref.gains(img, total, 1.5, grids["mean"], 32)
    assert np.array_equal(st.display_local_srgb8("mean", 1.5, bloom_intensity=0.5), local_ref.display(img, total, 1.5, want, 0.5, before[-1]))
    for a, b in zip(before, everything_and_bloom(st)):
        assert util.same_bits_or_nan(a, b)


def test_refusals_return_their_status_and_leave_the_grid(rendered):  # noqa: F811
    st, images = rendered
    fresh = R.State()
    try:  # nothing exists yet
        for source in ("mean", "denoised", "temporal", "upsampled"):
            raises(NOT_READY, lambda: fresh.local_exposure(source, sample_total=1))
        raises(NOT_READY, lambda: fresh.local_exposure_download())
    finally:
        fresh.close()
    L, P = st._L, R.state.LocalParams
    good = P(0.5, 0.5, 0.18, 4.0, 0, 0)
    gain_buf, byte_buf = np.zeros((32, 48), F), np.zeros((32, 48, 4), np.uint8)
    build = lambda source, total, cell, stream=None: st._check(L.rsrt_local_exposure(st._ctx, source, total, cell, stream), "rsrt_local_exposure")  # noqa: E731
    gain = lambda source, total, e, params, buf=gain_buf, n=None: st._check(  # noqa: E731
        L.rsrt_local_gain_download(st._ctx, source, total, e, params, R.state._p(buf) if buf is not None else None, buf.size if n is None else n), "rsrt_local_gain_download")
    show = lambda source, total, e, params, i, buf=byte_buf, n=None: st._check(  # noqa: E731
        L.rsrt_display_local_srgb8(st._ctx, source, total, e, params, i, R.state._p(buf) if buf is not None else None, buf.size if n is None else n), "rsrt_display_local_srgb8")
    st.bloom_reset()
    st.local_exposure_reset()
    raises(NOT_READY, st.local_exposure_download)  # no grid
    raises(NOT_READY, lambda: st.local_gain("mean", 1.5))
    raises(NOT_READY, lambda: st.display_local_srgb8("mean", 1.5))
    st.local_exposure("mean", 8)
    g0 = st.local_exposure_download()[0]
    assert np.array_equal(g0, local_ref.grid_of(images["mean"][0], 4, 8))
    raises(NOT_READY, lambda: st.display_local_srgb8("mean", 1.5, bloom_intensity=0.5))  # no bloom image; without bloom it is not needed
    show(0, 4, 1.5, C.byref(good), 0.0)
    for cell in (0, 1, 7, 9, 24, 128, 0xffffffff):
        raises(INVALID, lambda: build(0, 4, cell))
    raises(INVALID, lambda: build(7, 4, 32))  # unknown source
    raises(INVALID, lambda: build(0, 0, 32))  # sample_total 0 under the mean
    raises(INVALID, lambda: gain(7, 4, 1.5, C.byref(good)))
    raises(INVALID, lambda: show(7, 4, 1.5, C.byref(good), 0.0))
    raises(INVALID, lambda: gain(0, 0, 1.5, C.byref(good)))
    raises(INVALID, lambda: show(0, 0, 1.5, C.byref(good), 0.0))
    for e in (0.0, -1.0, float("nan"), float("inf")):
        raises(INVALID, lambda: gain(0, 4, e, C.byref(good)))
        raises(INVALID, lambda: show(0, 4, e, C.byref(good), 0.0))
    raises(INVALID, lambda: gain(0, 4, 1.5, None))  # NULL params
    raises(INVALID, lambda: show(0, 4, 1.5, None, 0.0))
    for bad in (P(-0.1, 0.5, 0.18, 4.0, 0, 0), P(0.5, 1.5, 0.18, 4.0, 0, 0), P(0.5, 0.5, 0.0, 4.0, 0, 0), P(0.5, 0.5, float("nan"), 4.0, 0, 0),
                P(0.5, 0.5, 0.18, 16.5, 0, 0), P(0.5, 0.5, 0.18, -1.0, 0, 0), P(0.5, 0.5, 0.18, 4.0, 1, 0), P(float("nan"), 0.5, 0.18, 4.0, 0, 0)):
        raises(INVALID, lambda: gain(0, 4, 1.5, C.byref(bad)))
        raises(INVALID, lambda: show(0, 4, 1.5, C.byref(bad), 0.0))
    for i in (-0.5, float("nan"), float("inf")):
        raises(INVALID, lambda: show(0, 4, 1.5, C.byref(good), i))
    raises(INVALID, lambda: gain(0, 4, 1.5, C.byref(good), n=gain_buf.size - 1))  # a wrong float or byte count, a NULL buffer
    raises(INVALID, lambda: gain(0, 4, 1.5, C.byref(good), n=gain_buf.size * 4))
    raises(INVALID, lambda: show(0, 4, 1.5, C.byref(good), 0.0, n=byte_buf.size // 4))
    raises(INVALID, lambda: st._check(L.rsrt_local_gain_download(st._ctx, 0, 4, 1.5, C.byref(good), None, gain_buf.size), "rsrt_local_gain_download"))
    raises(INVALID, lambda: st._check(L.rsrt_display_local_srgb8(st._ctx, 0, 4, 1.5, C.byref(good), 0.0, None, byte_buf.size), "rsrt_display_local_srgb8"))
    short = np.zeros(8, np.uint32)
    raises(INVALID, lambda: st._check(L.rsrt_local_exposure_download(st._ctx, R.state._p(short), short.size, None), "rsrt_local_exposure_download"))
    raises(INVALID, lambda: st._check(L.rsrt_local_exposure_download(st._ctx, None, g0.size, None), "rsrt_local_exposure_download"))
    raises(INVALID, lambda: st.local_gain("upsampled", 1.5))  # the grid was built for the accumulator's size, not the guide's
    raises(INVALID, lambda: st.display_local_srgb8("upsampled", 1.5))
    st.bloom("upsampled", 1.5, levels=2)  # a bloom image of another size than the source
    raises(INVALID, lambda: st.display_local_srgb8("mean", 1.5, bloom_intensity=0.5))
    st.display_local_srgb8("mean", 1.5)
    st.set_partition(0, 2)
    raises(INVALID, st.local_exposure)
    raises(INVALID, st.local_exposure_download)
    raises(INVALID, st.local_exposure_reset)
    raises(INVALID, lambda: st.local_gain("mean", 1.5))
    raises(INVALID, lambda: st.display_local_srgb8("mean", 1.5))
    st.set_partition(0, 1)
    # after all that: the same grid of the same shape, and a display that still works
    dims = (C.c_uint32 * 4)()
    st._check(L.rsrt_local_exposure_download(st._ctx, None, 0, dims), "rsrt_local_exposure_download")
    assert list(dims) == [6, 4, 32, 8]
    got, cell = st.local_exposure_download()
    assert cell == 8 and np.array_equal(got, g0)
    img, total = images["mean"]
    want = local_ref.gains(img, total, 1.5, g0, 8)
    assert same(st.local_gain("mean", 1.5), want) and np.array_equal(st.display_local_srgb8("mean", 1.5), local_ref.display(img, total, 1.5, want))
    # a reset drops it; the images stay
    st.local_exposure_reset()
    raises(NOT_READY, st.local_exposure_download)
    raises(NOT_READY, lambda: st.display_local_srgb8("mean", 1.5))
    assert same(st.download(), img)
    st.local_exposure("mean", 8)
    assert grid_equal(st, g0, 8)


def test_a_change_of_the_accumulators_size_drops_the_grid():
    h, w = 20, 36
    sums, _ = local_ref.synthetic(h, w, seed=3)
    other, _ = local_ref.synthetic(h, w, seed=4)
    st = R.State()
    try:
        a, b = DeviceArray(sums), DeviceArray(other)
        st.bind_accumulator(a.data_ptr(), w, h)
        st.local_exposure("mean", 16, sample_total=1)
        g0 = local_ref.grid_of(sums, 1, 16)
        assert grid_equal(st, g0, 16)
        st.bind_accumulator(b.data_ptr(), w, h)  # the same size: the grid stays (it is the caller's to rebuild)
        assert grid_equal(st, g0, 16)
        assert same(st.local_gain("mean", 1.0, sample_total=1), local_ref.gains(other, 1, 1.0, g0, 16))
        st._check(st._L.rsrt_accumulator_bind(st._ctx, None, 0, 0), "rsrt_accumulator_bind")  # no accumulator any more
        raises(NOT_READY, st.local_exposure_download)
        st.bind_accumulator(a.data_ptr(), w, h)
        raises(NOT_READY, st.local_exposure_download)
        raises(NOT_READY, lambda: st.display_local_srgb8("mean", 1.0, sample_total=1))
        st.local_exposure("mean", 16, sample_total=1)
        assert grid_equal(st, g0, 16)
        st.bind_accumulator(a.data_ptr(), h, w)  # another size
        raises(NOT_READY, st.local_exposure_download)
    finally:
        st.close()
    sc, st = state("default", 32, 16)
    try:
        st.render_samples(2)
        st.local_exposure()
        assert st.local_exposure_download()[0].shape == (32, 1, 1, 2)
        st.resize(48, 24)
        raises(NOT_READY, st.local_exposure_download)
        raises(NOT_READY, st.display_local_srgb8)
        st.render_samples(2)
        st.local_exposure()
        assert grid_equal(st, local_ref.grid_of(st.download(), 2, 32), 32)
    finally:
        st.close()


def test_a_callers_stream_and_calls_in_a_row():
    h, w = 4 * TH + 7, 6 * TW + 5
    sums, _ = local_ref.synthetic(h, w, seed=9)
    R.state.lib()
    hip = C.CDLL(hip_runtime_path())  # a caller stream from the HIP runtime the library itself uses
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    st = R.State()
    try:
        dev = DeviceArray(sums)
        st.bind_accumulator(dev.data_ptr(), w, h)
        st.local_exposure("mean", 32, sample_total=3)
        own = st.local_exposure_download()[0]
        st.local_exposure_reset()
        st.local_exposure("mean", 32, sample_total=3, stream=stream.value)
        st.synchronize()
        assert grid_equal(st, own, 32) and np.array_equal(own, local_ref.grid_of(sums, 3, 32))
        # two calls in a row on different streams: the second call's grid, and a display on the context's stream right behind it
        for first, second in ((8, 64), (64, 8), (32, 16)):
            st.local_exposure("mean", first, sample_total=3)
            st.local_exposure("mean", second, sample_total=3, stream=stream.value)
            grid = local_ref.grid_of(sums, 3, second)
            want = local_ref.gains(sums, 3, 0.5, grid, second)
            assert np.array_equal(st.display_local_srgb8("mean", 0.5, sample_total=3), local_ref.display(sums, 3, 0.5, want)), (first, second)
            assert grid_equal(st, grid, second), (first, second)
    finally:
        st.close()
        hip.hipStreamDestroy(stream)


def test_the_python_state_round_trip_on_house():
    w, h = 64, 36
    sc, st = state("house", w, h)
    try:
        st.render_samples(4)
        r = st.auto_exposure()
        e = F(r["exposure"])
        st.local_exposure()
        acc = st.download()
        grid = local_ref.grid_of(acc, 4, local_ref.DEFAULTS["cell"])
        assert grid_equal(st, grid, 32)
        want = local_ref.gains(acc, 4, e, grid, 32)
        assert same(st.local_gain(), want) and (want > 1).any() and (want < 1).any()  # the room is lifted, the sky lowered
        shown = st.display_local_srgb8()
        assert np.array_equal(shown, local_ref.display(acc, 4, e, want))
        assert not np.array_equal(shown, st.display_exposed_srgb8())
        assert np.array_equal(st.display_local_srgb8(shadows=0.0, highlights=0.0), st.display_exposed_srgb8())
        st.bloom()
        b = st.bloom_download()
        assert np.array_equal(st.display_local_srgb8(bloom_intensity=0.1), local_ref.display(acc, 4, e, want, 0.1, b))
        assert np.array_equal(st.display_local_srgb8(shadows=0.0, highlights=0.0, bloom_intensity=0.1), st.display_bloomed_srgb8())
        st.exposure_reset()  # no remembered exposure: 1
        assert same(st.local_gain(shadows=1.0, key=0.3), local_ref.gains(acc, 4, 1.0, grid, 32, shadows=1.0, key=0.3))
    finally:
        st.close()


def test_cpp_state_grades_like_the_python_state(tmp_path):
    import test_local
    exe = test_local.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "4", "16"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    sc, st = state("spheres_only", w, h)
    try:
        st.render_samples(4)
        e = st.auto_exposure()["exposure"]
        assert ["exposure", "%08x" % int(np.asarray(e, F).view(np.uint32))] in lines
        st.local_exposure(cell=16)
        grid, cell = st.local_exposure_download()
        assert np.array_equal(grid, local_ref.grid_of(st.download(), 4, 16))
        assert next(f for f in lines if f[0] == "grid")[1:] == ["4", "3", "32", "16", "%016x" % fnv1a(grid.tobytes())]
        gain = st.local_gain()
        assert next(f for f in lines if f[0] == "gain")[1:] == [str(gain.size), "%016x" % fnv1a(gain.tobytes())]
        shown = st.display_local_srgb8()
        assert next(f for f in lines if f[0] == "display")[1:] == [str(shown.size), "%016x" % fnv1a(shown.tobytes())]
        assert ["strength0", "yes"] in lines and ["reset", "yes"] in lines
    finally:
        st.close()
