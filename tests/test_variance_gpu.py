"""The variance guidance on the GPU: the moments kernel (RSRT_TEMPORAL_MOMENTS) against the numpy restatement fed with the frames' own
downloads, bit for bit, and a MOMENTS run's history against a plain run's; the variance-guided filter and the clamp against the
restatement; no effect on the other passes; the documented errors and resets; the C++ State; and the error against a converged
reference along a panning and a held camera."""
import ctypes as C

import numpy as np
import pytest

import temporal_ref as T
import test_denoise
import test_denoise_gpu
import test_temporal_gpu as TG
import util
import variance_ref as V
import rsoderh_raytracing_amd as R

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4


def accumulate_ex(st, n, flags, t=None):
    p = R.state.TemporalParams(**R.state.TEMPORAL_DEFAULTS)
    st._check(st._L.rsrt_temporal_accumulate_ex(st._ctx, R.state._p(st.camera), n, n if t is None else t, C.byref(p), flags, None),
              "rsrt_temporal_accumulate_ex")


@pytest.mark.parametrize("name,w,h", [("default", 64, 48), ("house", 160, 90), ("suzanne", 96, 64)])
def test_moments_kernel_equals_the_restatement_bit_for_bit(name, w, h):
    sc, st = TG.state(name, w, h)
    _, plain = TG.state(name, w, h)
    try:
        desc, pdesc = TG.desc_of(sc), TG.desc_of(sc)
        ref = V.MomentSequence()
        seen = np.zeros(len(T.CODE_NAMES), np.int64)
        for i, (dy, dp, dpos, n) in enumerate(TG.PATH):
            TG.aim(st, desc, dy, dp, dpos)
            TG.aim(plain, pdesc, dy, dp, dpos)
            st.render_temporal(n, moments=True)
            plain.render_temporal(n)
            sums, aov, got, mom = st.download(), st.download_aov(), st.download_temporal(), st.download_temporal_moments()
            wcol, wmom, code = ref.frame(sums, aov, n, n, T.Camera.from_record(st.camera))
            assert np.array_equal(util.bits(got), util.bits(wcol)), (name, i)
            assert np.array_equal(util.bits(mom), util.bits(wmom)), (name, i)
            assert np.array_equal(util.bits(got), util.bits(plain.download_temporal())), (name, i)  # the plain run's history
            seen += np.bincount(code.reshape(-1), minlength=len(seen))
        print(name, dict(zip(T.CODE_NAMES, seen.tolist())))
        assert seen[T.IDENTITY] and seen[T.REPROJECTED], seen
    finally:
        st.close()
        plain.close()


@pytest.mark.parametrize("h,w", [(91, 173), (1, 1), (300, 7)])
def test_filter_equals_the_restatement_bit_for_bit(h, w):
    import test_variance
    sums, aov = test_denoise.synthetic(h, w, 4, 3, seed=13 * h + w)
    sums = test_variance.with_fireflies(sums, h * w)
    st, acc, aov_t = test_denoise_gpu.bound(h, w, sums, aov)
    try:
        for iters in (0, 1, 2, 5, 8):
            for demod, variance, clamp in test_variance.VARIANTS:
                sc = 4.0 if variance else 2.0
                got = st.denoise(iters, sc, 0.3, 0.2, demod, sample_total=4, aov_sample_total=3, variance=variance, clamp=clamp)
                want = V.denoise(sums, aov, 4, 3, iters, sc, 0.3, 0.2, demod, variance, clamp)
                assert np.array_equal(util.bits(got[..., :3]), util.bits(want)), (iters, demod, variance, clamp)
                assert (got[..., 3] == 1.0).all()
        assert np.array_equal(util.bits(acc.numpy()), util.bits(sums)) and np.array_equal(util.bits(aov_t.numpy()), util.bits(aov))
    finally:
        st.close()


@pytest.mark.parametrize("name,w,h", [("house", 160, 90), ("suzanne", 96, 64)])
def test_temporal_filter_equals_the_restatement_bit_for_bit(name, w, h):
    """Over the temporal colour and its moments along the camera path: every frame, with and without the clamp, and the default filter
    of the same frame unchanged."""
    sc, st = TG.state(name, w, h)
    try:
        desc = TG.desc_of(sc)
        few = many = 0
        for i, (dy, dp, dpos, n) in enumerate(TG.PATH + [(0.0, 0.0, (0, 0, 0), 1)] * 3):
            TG.aim(st, desc, dy, dp, dpos)
            st.render_temporal(n, moments=True)
            tmp, aov, mom = st.download_temporal(), st.download_aov(), st.download_temporal_moments()
            for clamp in (False, True):
                got = st.denoise(temporal=True, variance=True, clamp=clamp)
                want = V.denoise(tmp, aov, 1, n, 5, V.SIGMA_L, 0.5, 0.3, True, True, clamp, mom)
                assert np.array_equal(util.bits(got[..., :3]), util.bits(want)), (i, clamp)
            fixed = st.denoise(temporal=True)
            import denoise_ref
            assert np.array_equal(util.bits(fixed[..., :3]), util.bits(denoise_ref.denoise(tmp, aov, 1, n))), i
            few, many = few + int((mom[..., 2] < 4).sum()), many + int((mom[..., 2] >= 4).sum())
        assert few > 0 and many > 0  # the spatial and the temporal estimate
    finally:
        st.close()


def test_passes_stay_isolated():
    sc, st = TG.state("house", 96, 54)
    _, ref = TG.state("house", 96, 54)
    try:
        desc, rdesc = TG.desc_of(sc), TG.desc_of(sc)
        for k, dyaw in enumerate((0.0, 0.03, 0.0)):
            TG.aim(st, desc, dyaw)
            TG.aim(ref, rdesc, dyaw)
            st.render_temporal(2, moments=True)
            ref.render_temporal(2)
        sums, aov, tmp = st.download(), st.download_aov(), st.download_temporal()
        assert np.array_equal(util.bits(sums), util.bits(ref.download())) and np.array_equal(util.bits(aov), util.bits(ref.download_aov()))
        assert np.array_equal(util.bits(tmp), util.bits(ref.download_temporal()))
        d0, t0 = ref.denoise(), ref.denoise(temporal=True)
        for kw in ({"variance": True}, {"variance": True, "clamp": True}, {"clamp": True}, {"temporal": True, "variance": True, "clamp": True}):
            st.denoise(**kw)
            assert np.array_equal(util.bits(st.denoise()), util.bits(d0)), kw
            assert np.array_equal(util.bits(st.denoise(temporal=True)), util.bits(t0)), kw
        assert np.array_equal(util.bits(st.download()), util.bits(sums)) and np.array_equal(util.bits(st.download_aov()), util.bits(aov))
        assert np.array_equal(util.bits(st.download_temporal()), util.bits(tmp))
        m0 = st.download_temporal_moments()
        st.denoise(temporal=True, variance=True)
        assert np.array_equal(util.bits(st.download_temporal_moments()), util.bits(m0))
    finally:
        st.close()
        ref.close()


def test_errors_and_resets():
    sc, st = TG.state("house", 64, 40)
    try:
        st.render_samples(1, aov=True)
        with pytest.raises(R.RsrtError) as e:
            accumulate_ex(st, 1, 2)
        assert e.value.status == INVALID  # unknown flags
        with pytest.raises(R.RsrtError) as e:
            st.denoise(variance=True, demodulate=False)
        assert e.value.status == INVALID
        with pytest.raises(R.RsrtError) as e:
            st._check(st._L.rsrt_denoise(st._ctx, 1, 1, C.byref(R.state.DenoiseParams(5, 1 | 16, 2.0, 0.5, 0.3)), None, None), "rsrt_denoise")
        assert e.value.status == INVALID  # unknown denoise flags
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal_moments()
        assert e.value.status == NOT_READY  # no frame yet
        st.render_temporal(1)
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal_moments()
        assert e.value.status == NOT_READY  # the last frame carried no moments
        with pytest.raises(R.RsrtError) as e:
            st.denoise(temporal=True, variance=True)
        assert e.value.status == NOT_READY
        st.denoise(temporal=True, clamp=True)  # the clamp alone needs no moments
        # a MOMENTS toggle drops the history, in the library itself (the camera held: identity otherwise)
        st.clear()
        st.render_range(50, 1)
        st.clear_aov()
        st.render_aov(50, 1)
        accumulate_ex(st, 1, 1)
        assert TG.first_frame(st, 1) and (st.download_temporal_moments()[..., 2] == 1).all()
        accumulate_ex(st, 1, 1)
        assert (st.download_temporal()[..., 3] == 2).all() and (st.download_temporal_moments()[..., 2] == 2).all()
        accumulate_ex(st, 1, 0)
        assert TG.first_frame(st, 1)
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal_moments()
        assert e.value.status == NOT_READY
        accumulate_ex(st, 1, 1)
        assert TG.first_frame(st, 1)
        # ... and the State resets its own key (sample indices from 0)
        st.render_temporal(1, moments=True)
        st.render_temporal(1, moments=True)
        assert st.temporal_sample_count == 2 and (st.download_temporal_moments()[..., 2] == 2).all()
        st.render_temporal(1)
        assert st.temporal_sample_count == 1 and TG.first_frame(st, 1)
        st.render_temporal(1, moments=True)
        assert st.temporal_sample_count == 1 and (st.download_temporal_moments()[..., 2] == 1).all()
        # a reset and a resize
        st.temporal_reset()
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal_moments()
        assert e.value.status == NOT_READY
        st.render_temporal(1, moments=True)
        st.resize(48, 30)
        st.resize(64, 40)
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal_moments()
        assert e.value.status == NOT_READY
        st.set_partition(0, 2)
        for call in (lambda: accumulate_ex(st, 1, 1), lambda: st.denoise(variance=True, clamp=True)):
            with pytest.raises(R.RsrtError) as e:
                call()
            assert e.value.status == INVALID
        st.set_partition(0, 1)
    finally:
        st.close()


def rmse(a, b):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).mean()))


def disp(x):
    return R.host.display_srgb8(np.concatenate([x[..., :3], np.ones(x.shape[:2] + (1,), np.float32)], axis=-1), 1)


def test_panning_camera_errors():
    """House 320x180, 8 panning frames of 1 spp, against 1024 spp at the last camera from disjoint samples.  The clamp lowers the fixed
    filter's linear error and the variance-guided filter lowers the display error.  The variance-guided filter does NOT lower the linear
    error (measured 1.36x the fixed filter's with the clamp): it spreads the demodulated fireflies it cannot clamp over their neighbours,
    and remodulation by a brighter albedo amplifies them."""
    w, h = 320, 180
    sc, st = TG.state("house", w, h)
    try:
        desc = TG.desc_of(sc)
        for i in range(8):
            TG.aim(st, desc, 0.004 if i else 0.0)
            st.render_temporal(1, moments=True)
        tmp = st.download_temporal()
        out = {"temporal": tmp, "fixed": st.denoise(temporal=True), "fixed+clamp": st.denoise(temporal=True, clamp=True),
               "variance": st.denoise(temporal=True, variance=True), "variance+clamp": st.denoise(temporal=True, variance=True, clamp=True)}
        st.clear()
        st.render_range(100000, 1024)
        ref = st.download()[..., :3] / np.float32(1024)
        ref_disp = disp(ref)
        lin = {k: rmse(v, ref) for k, v in out.items()}
        dsp = {k: rmse(disp(v), ref_disp) for k, v in out.items()}
        print("house %dx%d, 8 panning 1-spp frames; RMSE / the fixed filter's, linear and display:" % (w, h))
        for k in out:
            print("  %-15s linear %.4f (%.3fx)  display %.3f (%.3fx)" % (k, lin[k], lin[k] / lin["fixed"], dsp[k], dsp[k] / dsp["fixed"]))
        assert lin["fixed+clamp"] < lin["fixed"]
        assert dsp["variance+clamp"] < dsp["fixed"] and dsp["variance"] < dsp["fixed"]
    finally:
        st.close()


def test_held_camera_errors():
    """House 96x54, 256 frames of 1 spp at one camera (max_history 256), against 4096 spp from disjoint samples.  The moments count the
    frames and the display error of the variance-guided filter stays below the unfiltered history's.  Its linear error does NOT stay
    at the unfiltered history's (measured 1.66x): the fireflies that remain at 256 spp keep the variance high where they are, and the
    filter spreads them."""
    w, h = 96, 54
    sc, st = TG.state("house", w, h)
    try:
        for _ in range(256):
            st.render_temporal(1, max_history=256, moments=True)
        tmp = st.download_temporal()
        mom = st.download_temporal_moments()
        assert (tmp[..., 3] == 256).all() and (mom[..., 2] == 256).all()
        var = st.denoise(temporal=True, variance=True)
        fixed = st.denoise(temporal=True)
        st.clear()
        st.render_range(1000000, 4096)
        ref = st.download()[..., :3] / np.float32(4096)
        e_t, e_v, e_f = rmse(tmp, ref), rmse(var, ref), rmse(fixed, ref)
        d_t, d_v, d_f = rmse(disp(tmp), disp(ref)), rmse(disp(var), disp(ref)), rmse(disp(fixed), disp(ref))
        print("house %dx%d, 256 held 1-spp frames, linear RMSE: temporal %.5f, variance-guided %.5f (%.3fx), fixed filter %.5f (%.3fx)"
              % (w, h, e_t, e_v, e_v / e_t, e_f, e_f / e_t))
        print("  display RMSE: temporal %.3f, variance-guided %.3f (%.3fx), fixed filter %.3f (%.3fx)" % (d_t, d_v, d_v / d_t, d_f, d_f / d_t))
        assert d_v < d_t
    finally:
        st.close()


def test_cpp_state_matches_the_python_state(tmp_path):
    import subprocess
    import test_variance
    exe = test_variance.build_cpp_demo(tmp_path)
    w, h = 80, 48
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", str(tmp_path / "o.f32")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(tmp_path / "o.f32", np.float32).reshape(5, h, w, 4)
    sc, st = TG.state("house", w, h)
    try:
        desc = TG.desc_of(sc)
        for f, n in enumerate((1, 1, 2, 1)):
            TG.aim(st, desc, 0.03 if f == 1 else 0.0, 0.02 if f == 3 else 0.0, (0.1, 0, 0) if f == 3 else (0, 0, 0))
            st.render_temporal(n, moments=True)
            assert np.array_equal(util.bits(got[f]), util.bits(st.download_temporal_moments())), f
        assert np.array_equal(util.bits(got[4]), util.bits(st.denoise(temporal=True, variance=True, clamp=True)))
    finally:
        st.close()
