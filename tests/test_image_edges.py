"""The image-space passes at the edges of their number formats, without a GPU: the denoiser's and the variance guidance's headers
compiled for the CPU against their numpy restatements, bit for bit, on every case of tests/edge_images.py (far and tiny depths, zero
and near-epsilon albedo, misses, huge and subnormal radiance) at shapes around the levels' workgroup; every output finite where the
inputs are; the binary16 depth feature's saturation; and a scene scaled so far that its first hits lie beyond binary16, end to end
through the checker."""
import numpy as np
import pytest

import denoise_ref as D
import edge_images as E
import oracle
import util
import variance_ref as V
import rsoderh_raytracing_amd as R
from test_denoise import host_filter  # noqa: F401  (fixture)
from test_variance import VARIANTS, host  # noqa: F401  (fixture)
import test_variance

SHAPES = E.SHAPES + [E.NARROW]
ITERS = (0, 1, 5, 8)
SIGMAS = (0.5, 0.3)  # sigma_normal, sigma_depth (the defaults)


def sigma_color(variance):
    return V.SIGMA_L if variance else 2.0


@pytest.mark.parametrize("h,w", SHAPES)
def test_fixed_filter_on_edge_inputs_matches_numpy_and_stays_finite(host_filter, h, w):
    for c in E.cases(h, w):
        for iters in ITERS:
            for demod in (True, False):
                got = host_filter(c.sums, c.aov, c.S, c.T, iters, 2.0, *SIGMAS, demod)
                want = D.denoise(c.sums, c.aov, c.S, c.T, iters, 2.0, *SIGMAS, demod)
                assert np.isfinite(want).all(), (c.name, iters, demod)
                assert np.array_equal(util.bits(got), util.bits(want)), (c.name, iters, demod)


@pytest.mark.parametrize("h,w", SHAPES)
def test_variance_filter_on_edge_inputs_matches_numpy_and_stays_finite(host, h, w):
    """Every VARIANTS combination from the input's own moments, and the variance-guided filter over temporal moment records with frames
    below, at and above RSRT_SV_MIN_FRAMES, with and without the clamp."""
    mom = E.moment_records(h, w, seed=h + w)
    assert (mom[..., 2] < V.MIN_FRAMES).any() and (mom[..., 2] == V.MIN_FRAMES).any()
    for c in E.cases(h, w):
        for iters in ITERS:
            runs = [(demod, variance, clamp, None) for demod, variance, clamp in VARIANTS]
            runs += [(True, True, clamp, mom) for clamp in (False, True)]
            for demod, variance, clamp, m in runs:
                sc = sigma_color(variance)
                got, _ = test_variance.host_filter(host, c.sums, c.aov, c.S, c.T, iters, sc, *SIGMAS, demod, variance, clamp, m)
                want = V.denoise(c.sums, c.aov, c.S, c.T, iters, sc, *SIGMAS, demod, variance, clamp, m)
                what = (c.name, iters, demod, variance, clamp, m is not None)
                assert np.isfinite(want).all(), what
                assert np.array_equal(util.bits(got), util.bits(want)), what


def test_depth_feature_saturates_at_the_largest_binary16():
    """Means below 65520 pack to the bits they always did; from 65520 on (which binary16 rounds to inf) they pack to 65504."""
    z = np.array([0.0, 3.0, 65488.0, 65503.0, 65504.0, 65519.99, np.nextafter(np.float32(65520), np.float32(0)), 65520.0, 1e5, 1e7,
                  3e38], np.float32)
    aov = np.zeros((1, len(z), 8), np.float32)
    aov[0, :, 4] = 1.0
    aov[0, :, 7] = z * np.float32(4)
    f = D.features(aov, 4)
    plain = (aov[..., 4:8] / np.float32(4)).astype(np.float16).astype(np.float32)
    below = z < 65520
    assert np.array_equal(util.bits(f[0, below]), util.bits(plain[0, below]))
    assert (f[0, ~below, 3] == np.float32(65504)).all() and np.isinf(plain[0, ~below, 3]).all()
    assert D.DEPTH_MAX == np.float32(np.finfo(np.float16).max)
    assert "#define RSRT_DN_DEPTH_MAX 65504.0f" in open(util.ROOT + "/include/rsrt_denoise.h").read()


def test_one_far_pixel_no_longer_poisons_the_frame(host_filter, host):
    """One pixel at mean depth 70,000 in an ordinary frame: the fixed filter (8 x 8, five levels) and the variance-guided filter with and
    without the clamp (16 x 16) stay finite everywhere."""
    sums, aov = E.base(8, 8, seed=3)
    aov[4, 4, 7] = np.float32(70000 * E.T_TOTAL)
    got = host_filter(sums, aov, E.S_TOTAL, E.T_TOTAL, 5, 2.0, *SIGMAS, True)
    assert np.isfinite(got).all()
    assert np.array_equal(util.bits(got), util.bits(D.denoise(sums, aov, E.S_TOTAL, E.T_TOTAL, 5, 2.0, *SIGMAS)))
    sums, aov = E.base(16, 16, seed=4)
    aov[7, 9, 7] = np.float32(70000 * E.T_TOTAL)
    for clamp in (False, True):
        got, v = test_variance.host_filter(host, sums, aov, E.S_TOTAL, E.T_TOTAL, 5, V.SIGMA_L, *SIGMAS, True, True, clamp)
        assert np.isfinite(got).all() and np.isfinite(v).all(), clamp
        want = V.denoise(sums, aov, E.S_TOTAL, E.T_TOTAL, 5, V.SIGMA_L, *SIGMAS, True, True, clamp)
        assert np.array_equal(util.bits(got), util.bits(want)), clamp


def test_existing_inputs_pack_as_before():
    """The saturation changes nothing below 65520: the features of the suites' synthetic frames are plain binary16 roundings."""
    import test_denoise
    import test_temporal
    frames = [test_denoise.synthetic(91, 173, 4, 3, seed=1)[1]]
    rng = np.random.default_rng(2)
    frames.append(test_temporal.synthetic_frame(test_temporal.look(*test_temporal.P0), 64, 48, 1, 2, rng)[1])
    for aov in frames:
        T = 3 if aov is frames[0] else 2
        plain = (aov[..., 4:8] / np.float32(T)).astype(np.float16).astype(np.float32)
        assert np.array_equal(util.bits(D.features(aov, T)), util.bits(plain))


# -------------------------------------------------------------------------------------------------- a far scene, end to end
def scaled_frame(tmp_path, w, h, n):
    """default.toml scaled by 2^15: the checker's sums and the restated AOV records of samples [0, n)."""
    sc = R.Scene.load_toml(E.scaled_default_scene(str(tmp_path)))
    osc = util.oracle_scene(sc)
    cam = sc.camera_uniform()
    aov = D.aov_records(sc, osc, np.asarray(cam).reshape(-1)[0], w, h, 0, n)
    sums, _ = oracle.render(osc, util.oracle_env(R.Environment.synthetic(256, 128)), cam.view(oracle.CAMERA), w, h, 0, n, 8)
    return sc, sums, aov


def far_and_near(aov, n):
    """Pixels whose mean depth packs to inf without the saturation, and hit pixels nearer than 65504."""
    z = aov[..., 7] / np.float32(n)
    return int((z >= 65520).sum()), int(((z < 65504) & (aov[..., 3] > 0)).sum())


def test_scaled_scene_filters_to_finite_values(tmp_path, host_filter, host):
    w, h, n = 96, 64, 4
    sc, sums, aov = scaled_frame(tmp_path, w, h, n)
    assert sc.spheres["radius"].max() == np.float32(1.3 * E.SCENE_SCALE)
    far, near = far_and_near(aov, n)
    assert far > 0 and near > 0, (far, near)
    assert np.isfinite(sums).all() and np.isfinite(aov).all()
    want = D.denoise(sums, aov, n, n)
    assert np.isfinite(want).all()
    assert np.array_equal(util.bits(host_filter(sums, aov, n, n, 5, 2.0, *SIGMAS, True)), util.bits(want))
    for variance, clamp in ((True, False), (True, True), (False, True)):
        sc_ = sigma_color(variance)
        want = V.denoise(sums, aov, n, n, 5, sc_, *SIGMAS, True, variance, clamp)
        assert np.isfinite(want).all(), (variance, clamp)
        got, _ = test_variance.host_filter(host, sums, aov, n, n, 5, sc_, *SIGMAS, True, variance, clamp)
        assert np.array_equal(util.bits(got), util.bits(want)), (variance, clamp)


def test_host_display_on_edge_values():
    """The host display pass against test_display's restatement on overflowing, negative and subnormal means (the GPU test holds the
    kernel to both)."""
    import test_display
    sums, S = E.display_edges(), E.DISPLAY_S
    mean = (sums[..., :3] / np.float32(S)).astype(np.float16)
    assert np.isinf(mean).any() and ((mean != 0) & (np.abs(mean) < np.float16(2.0 ** -14))).any() and (mean < 0).any()
    assert np.array_equal(R.host.display_srgb8(sums, S), test_display.display_numpy(sums, S))
