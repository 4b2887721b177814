"""Guided upsampling on the GPU (rsrt_guide_render, rsrt_upsample): the guide records against the checker's closest hits, the kernel
against its numpy restatement, bit for bit, for every source and output; no effect on any input; an edge kept by the guide; a picture
closer to the reference than bilinear upsampling and than the same number of paths traced at full size; the documented errors; the
Python and the C++ State."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import upsample_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, display_rmse, state

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def test_guide_records_equal_the_checker_hits_bit_for_bit():
    w, h, W, H = 80, 45, 160, 90
    sc, st = state("house", w, h)
    try:
        st.render_samples(2, aov=True)
        acc, aov = st.download(), st.download_aov()
        st.render_guide(W, H, 3, 4)
        got = st.download_guide()
        want = denoise_ref.aov_records(sc, util.oracle_scene(sc), st.camera[0], W, H, 3, 4)
        assert got.shape == (H, W, 8) and want[..., 3].max() == 4 and want[..., 3].sum() > 0
        assert same(got, want)
        assert st.guide_sample_count == 4 and (st.guide_width, st.guide_height) == (W, H)
        st.clear_guide()
        assert not st.download_guide().any() and st.guide_sample_count == 0
        st.render_guide(W, H, 3, 2)
        st.render_guide(W, H, 5, 2)
        assert same(st.download_guide(), got)  # [3,5) + [5,7) = [3,7)
        st.render_guide(W + 1, H, 3, 1)  # another size: a fresh, zeroed buffer
        assert st.download_guide().shape == (H, W + 1, 8) and st.download_guide()[..., 3].max() == 1
        assert same(st.download(), acc) and same(st.download_aov(), aov)  # the guide calls touched neither
        assert (st.width, st.height, st.sample_count, st.aov_sample_count) == (w, h, 2, 2)
    finally:
        st.close()


def test_guide_needs_no_accumulator():
    sc = R.Scene.load_toml(util.scene_path("default"))
    st = R.State()
    try:
        st.upload_scene(sc)
        st.camera = np.array(sc.camera_uniform()).view(R.types.CAMERA).reshape(1).copy()
        st.render_guide(40, 24, 0, 1)
        assert st.download_guide()[..., 3].max() == 1
        with pytest.raises(R.RsrtError) as e:
            st.upsample(sample_total=1, aov_sample_total=1)
        assert e.value.status == NOT_READY and "no accumulator" in str(e.value)  # still none
    finally:
        st.close()


def bound(lo, hi, seed):
    import test_upsample
    sums, aov, guide = test_upsample.inputs(lo, hi, seed)
    dev = [DeviceArray(a) for a in (sums, aov, guide)]
    st = R.State()
    st.bind_accumulator(dev[0].data_ptr(), lo[1], lo[0])
    st.bind_aov(dev[1].data_ptr(), lo[1], lo[0])
    st.bind_guide(dev[2].data_ptr(), hi[1], hi[0])
    return st, (sums, aov, guide), dev


def unchanged(host, dev):
    return all(same(d.numpy(), a) for a, d in zip(host, dev))


def shapes():
    import test_upsample
    return test_upsample.SHAPES


@pytest.mark.parametrize("lo,hi", shapes())
def test_kernel_equals_the_numpy_restatement_bit_for_bit(lo, hi):
    import test_upsample
    st, (sums, aov, guide), dev = bound(lo, hi, seed=11 * lo[0] + lo[1])
    try:
        for sn, sz in test_upsample.SIGMAS:
            for demod in (True, False):
                got = st.upsample("mean", sn, sz, demod, sample_total=4, aov_sample_total=3, guide_sample_total=5)
                want = upsample_ref.upsample(sums, aov, guide, 4, 3, 5, sn, sz, demod)
                assert got.shape == (hi[0], hi[1], 4) and (got[..., 3] == 1.0).all()
                assert same(got[..., :3], want), (sn, sz, demod)
        disp = st.upsampled_display_srgb8()
        assert same(disp, R.host.display_srgb8(got, 1))
        out = DeviceArray(np.zeros((hi[0], hi[1], 4), np.float32))  # into a caller's buffer
        st.upsample("mean", sample_total=4, aov_sample_total=3, guide_sample_total=5, out_ptr=out.data_ptr(), download=False)
        st.synchronize()
        assert same(out.numpy()[..., :3], upsample_ref.upsample(sums, aov, guide, 4, 3, 5))
        assert unchanged((sums, aov, guide), dev)
    finally:
        st.close()


def test_inf_features_fall_back_on_the_gpu_too():
    lo, hi = (45, 87), (91, 173)
    import test_upsample
    sums, aov, guide = test_upsample.inputs(lo, hi, seed=5)
    aov[10:20, 30:50, 4:7] = 1e9
    guide[40:70, 20:60, 4:7] = 1e9
    dev = [DeviceArray(a) for a in (sums, aov, guide)]
    st = R.State()
    try:
        st.bind_accumulator(dev[0].data_ptr(), lo[1], lo[0])
        st.bind_aov(dev[1].data_ptr(), lo[1], lo[0])
        st.bind_guide(dev[2].data_ptr(), hi[1], hi[0])
        got = st.upsample("mean", sample_total=4, aov_sample_total=3, guide_sample_total=5)
        want, fallback = upsample_ref.upsample(sums, aov, guide, 4, 3, 5, return_fallback=True)
        assert np.isfinite(got).all() and fallback[40:70, 20:60].all()
        assert same(got[..., :3], want)
    finally:
        st.close()


def test_denoised_and_temporal_sources_equal_the_restatement():
    lo, hi = (45, 87), (91, 173)
    st, (sums, aov, guide), dev = bound(lo, hi, seed=3)
    try:
        den = st.denoise(3, sample_total=4, aov_sample_total=3)
        for demod in (True, False):
            got = st.upsample("denoised", 0.3, 0.2, demod, sample_total=0, aov_sample_total=3, guide_sample_total=5)  # sample_total is ignored
            assert same(got[..., :3], upsample_ref.upsample(den, aov, guide, 1, 3, 5, 0.3, 0.2, demod)), demod
        assert same(st.denoise(3, sample_total=4, aov_sample_total=3), den)  # ... and the denoiser's scratch was left alone
        sc = R.Scene.load_toml(util.scene_path("default"))
        st.camera = np.array(sc.camera_uniform()).view(R.types.CAMERA).reshape(1).copy()
        p = R.state.TemporalParams(32, 0.05, 0.9)
        st._check(st._L.rsrt_temporal_accumulate(st._ctx, R.state._p(st.camera), 4, 3, C.byref(p), None), "rsrt_temporal_accumulate")
        hist = st.download_temporal()
        for demod in (True, False):
            got = st.upsample("temporal", demodulate=demod, sample_total=0, aov_sample_total=3, guide_sample_total=5)
            assert same(got[..., :3], upsample_ref.upsample(hist, aov, guide, 1, 3, 5, demodulate=demod)), demod
        assert same(st.download_temporal(), hist) and same(st.denoise(3, sample_total=4, aov_sample_total=3), den)
        assert unchanged((sums, aov, guide), dev)
    finally:
        st.close()


def test_normal_step_in_the_guide_keeps_its_two_colours():
    (h, w), (H, W) = (48, 32), (96, 64)
    left_lo, left_hi = np.arange(w) < w // 2, np.arange(W) < W // 2
    colours = np.float32([[0.9, 0.2, 0.1], [0.1, 0.3, 0.9]])
    sums = np.ones((h, w, 4), np.float32)
    sums[..., :3] = np.where(left_lo[None, :, None], colours[0], colours[1]) * 4

    def records(hh, ww, left):  # one albedo: only the normals tell the halves apart
        a = np.zeros((hh, ww, 8), np.float32)
        a[..., :3], a[..., 3] = 4 * 0.5, 4
        a[..., 4:7] = np.where(left[None, :, None], np.float32([1, 0, 0]), np.float32([0, 0, 1])) * 4
        a[..., 7] = 4 * 2.0
        return a
    aov, guide = records(h, w, left_lo), records(H, W, left_hi)
    dev = [DeviceArray(a) for a in (sums, aov, guide)]
    st = R.State()
    try:
        st.bind_accumulator(dev[0].data_ptr(), w, h)
        st.bind_aov(dev[1].data_ptr(), w, h)
        st.bind_guide(dev[2].data_ptr(), W, H)
        want = np.broadcast_to(np.where(left_hi[None, :, None], colours[0], colours[1]), (H, W, 3))
        out = st.upsample("mean", sigma_normal=0.01, sample_total=4, aov_sample_total=4, guide_sample_total=4)
        assert np.allclose(out[..., :3], want, rtol=0.01, atol=0)
        blur = st.upsample("mean", sigma_normal=1e3, sample_total=4, aov_sample_total=4, guide_sample_total=4)  # without the normal weight it bleeds
        assert not np.allclose(blur[:, W // 2 - 1, :3], want[:, W // 2 - 1], rtol=0.01, atol=0)
    finally:
        st.close()


@pytest.mark.parametrize("name,W,H", [("house", 192, 108), ("suzanne", 160, 96)])
def test_upsampled_image_is_closer_to_the_reference(name, W, H):
    """4 spp traced at half size (samples 0-3, the guide over the same samples) against 512 spp of disjoint samples (1000-1511) at full
    size, as the user sees them: RMSE of the display pass's sRGB bytes.  Measured on the CPU restatement before the kernel existed
    (guided / bilinear): house mean 22.999 / 36.952, denoised 17.592 / 20.236, full-size 1 spp denoised 40.724; suzanne mean 18.211 /
    20.631, denoised 23.455 / 23.904, full-size 1 spp denoised 29.506."""
    w, h = (W + 1) // 2, (H + 1) // 2
    sc, full = state(name, W, H)
    _, st = state(name, w, h)
    try:
        full.render_range(1000, 512)
        ref = R.host.display_srgb8(full.download(), 512)
        full.clear()
        full.render_samples(1, aov=True)  # the same number of paths, traced at full size
        full.denoise(download=False)
        full_1spp = display_rmse(full.denoised_display_srgb8(), ref)

        def bilinear(img):
            up = np.ones((H, W, 4), np.float32)
            up[..., :3] = upsample_ref.bilinear(img[..., :3], H, W)
            return display_rmse(R.host.display_srgb8(up, 1), ref)
        st.render_samples(4, aov=True)
        st.render_guide(W, H, 0, 4)
        st.upsample("mean", download=False)
        mean_guided = display_rmse(st.upsampled_display_srgb8(), ref)
        mean_bilinear = bilinear(st.download() / np.float32(4))
        den = st.denoise()
        st.upsample("denoised", download=False)
        den_guided = display_rmse(st.upsampled_display_srgb8(), ref)
        den_bilinear = bilinear(den)
        print("%s %dx%d from %dx%d: display RMSE mean guided %.3f bilinear %.3f; denoised guided %.3f bilinear %.3f; full-size 1 spp denoised %.3f"
              % (name, W, H, w, h, mean_guided, mean_bilinear, den_guided, den_bilinear, full_1spp))
        assert mean_guided < mean_bilinear
        if name == "house":
            assert den_guided < den_bilinear
        assert den_guided < full_1spp
    finally:
        st.close()
        full.close()


def raises(status, call):
    with pytest.raises(R.RsrtError) as e:
        call()
    assert e.value.status == status, e.value


def test_errors():
    sc, st = state("default", 32, 16)
    try:
        up = lambda **kw: st.upsample(**{"sample_total": 1, "aov_sample_total": 1, "guide_sample_total": 1, **kw})  # noqa: E731
        raises(NOT_READY, st.clear_guide)
        raises(NOT_READY, up)  # no AOV buffer
        st.render_samples(1, aov=True)
        raises(NOT_READY, up)  # no guide
        raises(NOT_READY, st.upsampled_display_srgb8)
        st.render_guide(64, 32, 0, 1)
        acc, aov, guide = st.download(), st.download_aov(), st.download_guide()
        raises(NOT_READY, lambda: up(source="denoised"))  # no denoised image
        raises(NOT_READY, lambda: up(source="temporal"))  # no temporal frame
        raw = lambda params, out=None: st._check(st._L.rsrt_upsample(st._ctx, 1, 1, 1, params, out, None), "rsrt_upsample")  # noqa: E731
        raises(INVALID, lambda: raw(None))  # NULL params
        P = R.state.UpsampleParams
        raises(INVALID, lambda: raw(C.byref(P(8 | 1, 0.5, 0.3))))  # an unknown flag
        raises(INVALID, lambda: raw(C.byref(P(2 | 4 | 1, 0.5, 0.3))))  # DENOISED | TEMPORAL
        for bad in ({"sigma_normal": 0.0}, {"sigma_depth": 1e7}, {"sigma_normal": float("nan")}, {"sample_total": 0}, {"aov_sample_total": 0},
                    {"guide_sample_total": 0}):
            raises(INVALID, lambda: up(**bad))
        mine = DeviceArray(np.zeros((32, 64 + 1, 4), np.float32))
        raises(INVALID, lambda: raw(C.byref(P(1, 0.5, 0.3)), C.c_void_p(mine.data_ptr() + 4)))  # a misaligned output pointer
        raises(INVALID, lambda: st._check(st._L.rsrt_guide_render(st._ctx, R.state._p(st.camera), 64, 32, 0, 1, 1, None), "rsrt_guide_render"))  # flags
        raises(INVALID, lambda: st.render_guide(16385, 1, 0, 1))
        st.denoise(download=False)
        assert up(source="denoised").shape == (32, 64, 4)  # sample_total would be ignored anyway
        assert same(st.download(), acc) and same(st.download_aov(), aov) and same(st.download_guide(), guide)  # no refused call wrote anything
        other = DeviceArray(np.zeros((8, 8, 8), np.float32))
        st.bind_aov(other.data_ptr(), 8, 8)  # AOV size != accumulator size
        raises(INVALID, up)
        st.bind_aov(None, 0, 0)
        st.render_aov(0, 1)
        for gw, gh in ((31, 32), (64, 15), (16385, 16)):  # a guide smaller than the accumulator in x, in y; above the largest size
            big = DeviceArray(np.zeros(8, np.float32))  # (never read: the call is refused)
            st.bind_guide(big.data_ptr(), gw, gh)
            raises(INVALID, up)
        st.bind_guide(None, 0, 0)
        raises(NOT_READY, up)  # the bound guide is gone, the library's was given up at the bind
        st.render_guide(32, 16, 0, 1)  # the same size is fine
        assert up().shape == (16, 32, 4)
        st.set_partition(0, 2)
        raises(INVALID, up)
        raises(INVALID, lambda: st.render_guide(32, 16, 0, 1))
        st.set_partition(0, 1)
    finally:
        st.close()


def test_render_upsampled_equals_the_manual_sequence():
    w, h, W, H = 48, 27, 96, 54
    sc, st = state("house", w, h)
    _, man = state("house", w, h)
    try:
        for denoise in (True, False):
            got = st.render_upsampled(W, H, 2, denoise=denoise)
            k = man.sample_count
            man.render_samples(2, aov=True)
            man.render_guide(W, H, k, 2)
            if denoise:
                man.denoise(download=False)
            want = man.upsample("denoised" if denoise else "mean")
            assert got.shape == (H, W, 4) and same(got, want), denoise
        assert st.sample_count == st.aov_sample_count == st.guide_sample_count == 4
        for s in (st, man):  # a new camera restarts the low frame and the guide
            s.camera = s.camera.copy()
            s.camera["pos"][0][0] += 0.25
        got = st.render_upsampled(W, H, 1)
        assert st.sample_count == st.aov_sample_count == st.guide_sample_count == 1
        man.render_samples(1, aov=True)
        assert man.guide_sample_count == 0 and not man.download_guide().any()  # the scene-hash reset cleared the guide too
        man.render_guide(W, H, 0, 1)
        man.denoise(download=False)
        assert same(got, man.upsample("denoised"))
        got = st.render_upsampled(W + 2, H, 1)  # another output size: a fresh guide over this call's samples
        assert got.shape == (H, W + 2, 4) and st.guide_sample_count == 1 and st.sample_count == 2
    finally:
        st.close()
        man.close()


def test_cpp_state_upsamples_like_the_python_state(tmp_path):
    import subprocess
    import test_upsample
    exe = test_upsample.build_cpp_demo(tmp_path)
    w, h, W, H = 40, 24, 80, 48
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), str(W), str(H), "4", "8", "256", "128", str(tmp_path / "o.f32")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(tmp_path / "o.f32", np.float32).reshape(H, W, 4)
    sc, st = state("house", w, h)
    try:
        assert same(got, st.render_upsampled(W, H, 4))
    finally:
        st.close()
