"""The image-space passes on the GPU at the edges of their number formats: the denoiser and the variance guidance against their numpy
restatements, bit for bit, on every case of tests/edge_images.py at shapes around the levels' workgroup; a scene scaled so far that its
first hits lie beyond binary16, through the AOV pass, the filters and the temporal pass; the temporal pass at thin image shapes; and the
display and binary16-mean kernels on overflowing, negative and subnormal means."""
import numpy as np
import pytest

import denoise_ref as D
import edge_images as E
import temporal_ref as T
import test_denoise_gpu as TDG
import test_display
import test_temporal_gpu as TG
import util
import variance_ref as V
import rsoderh_raytracing_amd as R
from test_variance import VARIANTS

pytestmark = pytest.mark.gpu

SHAPES = E.SHAPES + [E.NARROW]
ITERS = (0, 1, 5, 8)
SIGMAS = (0.5, 0.3)  # sigma_normal, sigma_depth (the defaults)


def check(got, want, what):
    assert np.array_equal(util.bits(got[..., :3]), util.bits(want)), what
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all(), what


@pytest.mark.parametrize("h,w", SHAPES)
def test_filter_on_edge_inputs_equals_the_restatements(h, w):
    for c in E.cases(h, w):
        st, acc, aov_t = TDG.bound(h, w, c.sums, c.aov)
        try:
            for iters in ITERS:
                for demod in (True, False):
                    got = st.denoise(iters, 2.0, *SIGMAS, demod, sample_total=c.S, aov_sample_total=c.T)
                    check(got, D.denoise(c.sums, c.aov, c.S, c.T, iters, 2.0, *SIGMAS, demod), (c.name, iters, demod))
                for demod, variance, clamp in VARIANTS:
                    sc = V.SIGMA_L if variance else 2.0
                    got = st.denoise(iters, sc, *SIGMAS, demod, sample_total=c.S, aov_sample_total=c.T, variance=variance, clamp=clamp)
                    want = V.denoise(c.sums, c.aov, c.S, c.T, iters, sc, *SIGMAS, demod, variance, clamp)
                    check(got, want, (c.name, iters, demod, variance, clamp))
            assert np.array_equal(util.bits(acc.numpy()), util.bits(c.sums)), c.name
            assert np.array_equal(util.bits(aov_t.numpy()), util.bits(c.aov)), c.name
        finally:
            st.close()


# -------------------------------------------------------------------------------------------------- a far scene, end to end
def scaled_state(tmp_path, w, h):
    sc = R.Scene.load_toml(E.scaled_default_scene(str(tmp_path)))
    st = R.State.new(sc, R.Environment.synthetic(256, 128), w, h)
    st.max_bounces = 8
    return sc, st


def test_scaled_scene_aov_and_filters(tmp_path):
    w, h, n = 96, 64, 4
    sc, st = scaled_state(tmp_path, w, h)
    try:
        st.render_samples(n, aov=True)
        sums, aov = st.download(), st.download_aov()
        want = D.aov_records(sc, util.oracle_scene(sc), st.camera[0], w, h, 0, n)
        assert np.array_equal(util.bits(aov), util.bits(want))
        z = aov[..., 7] / np.float32(n)
        assert (z >= 65520).any() and ((z < 65504) & (aov[..., 3] > 0)).any()
        check(st.denoise(), D.denoise(sums, aov, n, n), "fixed")
        check(st.denoise(variance=True), V.denoise(sums, aov, n, n, 5, V.SIGMA_L, *SIGMAS, True, True, False), "variance")
        check(st.denoise(clamp=True), V.denoise(sums, aov, n, n, 5, 2.0, *SIGMAS, True, False, True), "clamp")
        check(st.denoise(variance=True, clamp=True), V.denoise(sums, aov, n, n, 5, V.SIGMA_L, *SIGMAS, True, True, True), "both")
    finally:
        st.close()


@pytest.mark.parametrize("moments", [False, True])
def test_scaled_scene_temporal_pass(tmp_path, moments):
    """test_temporal_gpu.PATH with its steps scaled as the scene is: reprojection arithmetic at 1e5 units, bit for bit; then the
    filters of the last frame's temporal colour."""
    w, h = 96, 64
    sc, st = scaled_state(tmp_path, w, h)
    try:
        desc = TG.desc_of(sc)
        ref = V.MomentSequence() if moments else T.Sequence()
        seen = np.zeros(len(T.CODE_NAMES), np.int64)
        for i, (dy, dp, dpos, n) in enumerate(TG.PATH):
            TG.aim(st, desc, dy, dp, tuple(x * E.SCENE_SCALE for x in dpos))
            st.render_temporal(n, moments=moments)
            sums, aov, got = st.download(), st.download_aov(), st.download_temporal()
            cam = T.Camera.from_record(st.camera)
            if moments:
                want, wmom, code = ref.frame(sums, aov, n, n, cam)
                mom = st.download_temporal_moments()
                assert np.array_equal(util.bits(mom), util.bits(wmom)), i
            else:
                want, code = ref.frame(sums, aov, n, n, cam)
            assert np.array_equal(util.bits(got), util.bits(want)), i
            assert np.isfinite(got).all(), i
            seen += np.bincount(code.reshape(-1), minlength=len(seen))
        assert seen[T.IDENTITY] and seen[T.REPROJECTED], seen
        assert (aov[..., 7] / np.float32(n) >= 65520).any()
        check(st.denoise(temporal=True), D.denoise(got, aov, 1, n), "temporal fixed")
        if moments:
            for clamp in (False, True):
                want = V.denoise(got, aov, 1, n, 5, V.SIGMA_L, *SIGMAS, True, True, clamp, mom)
                check(st.denoise(temporal=True, variance=True, clamp=clamp), want, ("temporal variance", clamp))
    finally:
        st.close()


@pytest.mark.parametrize("w,h", [(65, 5), (1, 97)])
def test_temporal_pass_at_thin_shapes(w, h):
    """The bit-exact temporal check of test_temporal_gpu (and its moments) on real renders one pixel past a wave's row, and one pixel
    wide."""
    sc, st = TG.state("default", w, h)
    try:
        desc = TG.desc_of(sc)
        ref = V.MomentSequence()
        for i, (dy, dp, dpos, n) in enumerate(TG.PATH):
            TG.aim(st, desc, dy, dp, dpos)
            st.render_temporal(n, moments=True)
            sums, aov = st.download(), st.download_aov()
            want, wmom, _ = ref.frame(sums, aov, n, n, T.Camera.from_record(st.camera))
            assert np.array_equal(util.bits(st.download_temporal()), util.bits(want)), i
            assert np.array_equal(util.bits(st.download_temporal_moments()), util.bits(wmom)), i
    finally:
        st.close()


# -------------------------------------------------------------------------------------------------- display and the binary16 mean
def test_display_and_mean_on_edge_values():
    sums, S = E.display_edges(), E.DISPLAY_S
    h, w = sums.shape[:2]
    acc = TDG.DeviceArray(sums)
    st = R.State()
    try:
        st.bind_accumulator(acc.data_ptr(), w, h)
        dev = st.display_srgb8(S)
        assert np.array_equal(dev, R.host.display_srgb8(sums, S))
        assert np.array_equal(dev, test_display.display_numpy(sums, S))
        m = st.download_mean_f16(S)
        want = (sums[..., :3] / np.float32(S)).astype(np.float16)
        assert np.isinf(want).any() and ((want != 0) & (np.abs(want) < np.float16(2.0 ** -14))).any()
        assert np.array_equal(m[..., :3].view(np.uint16), want.view(np.uint16))
        assert (m[..., 3] == 1.0).all()
    finally:
        st.close()
