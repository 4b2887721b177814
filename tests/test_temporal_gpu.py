"""The temporal pass on the GPU (rsrt_temporal_accumulate, State.render_temporal): the kernel against the numpy restatement fed with
the frames' own accumulator and AOV downloads, bit for bit; an unchanged camera converging like the accumulator; less error than the
single frame along a moving camera; no effect on the other passes; the documented errors and resets; the C++ State."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import temporal_ref as T
import util
import rsoderh_raytracing_amd as R

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4


def state(name, w, h, bounces=8):
    sc = R.Scene.load_toml(util.scene_path(name))
    st = R.State.new(sc, R.Environment.synthetic(256, 128), w, h)
    st.max_bounces = bounces
    return sc, st


def desc_of(sc):
    return np.array(sc.camera_desc).view(R.types.CAMERA_DESC).reshape(1).copy()


def aim(st, desc, dyaw=0.0, dpitch=0.0, dpos=(0.0, 0.0, 0.0)):
    """Moves desc (in f32, as the C++ State's arithmetic does) and points the State's camera at it."""
    desc["yaw"] += np.float32(dyaw)
    desc["pitch"] += np.float32(dpitch)
    desc["pos"][0] += np.asarray(dpos, np.float32)
    st.camera = np.array(R.camera_uniform(desc)).view(R.types.CAMERA).reshape(1).copy()


def accumulate(st, n, t=None, max_history=32, depth_tolerance=0.05, normal_tolerance=0.9, camera=True, params=True):
    """rsrt_temporal_accumulate itself (no State logic around it)."""
    p = R.state.TemporalParams(max_history, depth_tolerance, normal_tolerance)
    st._check(st._L.rsrt_temporal_accumulate(st._ctx, R.state._p(st.camera) if camera else None, n, n if t is None else t,
                                             C.byref(p) if params else None, None), "rsrt_temporal_accumulate")


# path: (yaw, pitch, pos step, spp) relative to the previous frame: a turn, a held frame, a jump that disoccludes, a tilt
PATH = [(0.0, 0.0, (0, 0, 0), 1), (0.02, 0.0, (0, 0, 0), 2), (0.0, 0.0, (0, 0, 0), 1), (-0.05, 0.0, (0.6, 0.1, -0.4), 1),
        (0.0, 0.03, (0, 0, 0), 2)]


@pytest.mark.parametrize("name,w,h", [("default", 64, 48), ("house", 160, 90), ("suzanne", 96, 64)])
def test_kernel_equals_the_restatement_bit_for_bit(name, w, h):
    sc, st = state(name, w, h)
    try:
        desc = desc_of(sc)
        ref = T.Sequence()
        seen = np.zeros(len(T.CODE_NAMES), np.int64)
        for i, (dy, dp, dpos, n) in enumerate(PATH):
            aim(st, desc, dy, dp, dpos)
            st.render_temporal(n)
            sums, aov, got = st.download(), st.download_aov(), st.download_temporal()
            want, code = ref.frame(sums, aov, n, n, T.Camera.from_record(st.camera))
            assert np.array_equal(util.bits(got), util.bits(want)), (name, i)
            seen += np.bincount(code.reshape(-1), minlength=len(seen))
        print(name, dict(zip(T.CODE_NAMES, seen.tolist())))
        assert seen[T.IDENTITY] and seen[T.REPROJECTED], seen
        assert seen[T.PLANE_REJECTED] + seen[T.NORMAL_REJECTED] + seen[T.LOW_WEIGHT] + seen[T.OUT_OF_VIEW] > 0, seen
    finally:
        st.close()


def test_unchanged_camera_converges_like_the_accumulator():
    sc, st = state("house", 160, 90)
    try:
        for _ in range(8):
            st.render_temporal(1, max_history=8)
        got = st.download_temporal()
        assert (got[..., 3] == 8).all()
        st.clear()
        st.render_range(0, 8)
        want = st.download()[..., :3] / np.float32(8)
        rel = np.abs(got[..., :3] - want) / np.maximum(np.abs(want), np.float32(1e-30))
        print("max relative difference to the 8-spp mean: %.3g" % rel.max())
        assert np.allclose(got[..., :3], want, rtol=1e-6, atol=0)
    finally:
        st.close()


def rmse(a, b):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).mean()))


def test_temporal_output_is_closer_to_the_reference():
    """House 320x180, 8 frames of 1 spp while the camera pans; the reference is 1024 spp at the last camera from disjoint samples."""
    w, h = 320, 180
    sc, st = state("house", w, h)
    try:
        desc = desc_of(sc)
        for i in range(8):
            aim(st, desc, 0.004 if i else 0.0)
            st.render_temporal(1)
        one = st.download()  # the last frame's own sample
        tmp = st.download_temporal()
        noisy_disp = st.display_srgb8()
        st.denoise()
        den_one = st.denoised_display_srgb8()
        st.denoise(temporal=True)
        den_tmp = st.denoised_display_srgb8()
        st.clear()
        st.render_range(100000, 1024)
        ref = st.download()[..., :3] / np.float32(1024)
        ref_disp = R.host.display_srgb8(st.download(), 1024)
        tmp_disp = R.host.display_srgb8(np.concatenate([tmp[..., :3], np.ones((h, w, 1), np.float32)], axis=-1), 1)
        lin = rmse(tmp, ref) / rmse(one, ref)
        disp = rmse(tmp_disp, ref_disp) / rmse(noisy_disp, ref_disp)
        filt = rmse(den_tmp, ref_disp) / rmse(den_one, ref_disp)
        print("house %dx%d, 8 frames of 1 spp panning: linear RMSE ratio temporal / 1 spp %.3f; display RMSE ratio %.3f; "
              "filtered temporal / filtered 1 spp %.3f" % (w, h, lin, disp, filt))
        assert lin < 1.0 and disp < 1.0 and filt < 1.0
    finally:
        st.close()


def test_passes_stay_isolated():
    sc, st = state("house", 96, 54)
    _, ref = state("house", 96, 54)
    try:
        desc = desc_of(sc)
        st.render_temporal(2)
        aim(st, desc, 0.03)
        st.render_temporal(3)  # samples [2, 5)
        ref.camera = st.camera.copy()
        ref.render_range(2, 3)
        ref.render_aov(2, 3)
        sums, aov = st.download(), st.download_aov()
        assert np.array_equal(util.bits(sums), util.bits(ref.download())) and np.array_equal(util.bits(aov), util.bits(ref.download_aov()))
        assert st.sample_count == 3 and st.aov_sample_count == 3 and st.temporal_sample_count == 5
        d0 = st.denoise()
        accumulate(st, 3)  # one more temporal frame over the same inputs: the filter of the accumulator does not see it
        assert np.array_equal(util.bits(st.denoise()), util.bits(d0))
        assert np.array_equal(util.bits(d0[..., :3]), util.bits(denoise_ref.denoise(sums, aov, 3, 3)))
        tmp = st.download_temporal()
        got = st.denoise(temporal=True, sample_total=7)  # (ignored)
        assert np.array_equal(util.bits(got[..., :3]), util.bits(denoise_ref.denoise(tmp, aov, 1, 3)))
        got0 = st.denoise(0, temporal=True)
        assert np.array_equal(util.bits(got0[..., :3]), util.bits(tmp[..., :3]))
        assert np.array_equal(util.bits(st.download()), util.bits(sums))
    finally:
        st.close()
        ref.close()


def first_frame(st, n):
    sums, got = st.download(), st.download_temporal()
    return np.array_equal(util.bits(got[..., :3]), util.bits(sums[..., :3] / np.float32(n))) and (got[..., 3] == n).all()


def test_errors():
    sc, st = state("default", 32, 16)
    bare = R.State()
    try:
        bare.camera = st.camera.copy()
        with pytest.raises(R.RsrtError) as e:
            accumulate(bare, 1)
        assert e.value.status == NOT_READY  # no accumulator
        with pytest.raises(R.RsrtError) as e:
            accumulate(st, 1)
        assert e.value.status == NOT_READY  # no AOV buffer
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal()
        assert e.value.status == NOT_READY  # no frame yet
        st.render_samples(1, aov=True)
        with pytest.raises(R.RsrtError) as e:
            st.denoise(temporal=True)
        assert e.value.status == NOT_READY
        bad = [{"max_history": 0}, {"max_history": (1 << 24) + 1}, {"depth_tolerance": 0.0}, {"depth_tolerance": 2e6},
               {"depth_tolerance": float("nan")}, {"normal_tolerance": 1.5}, {"normal_tolerance": -1.5}, {"normal_tolerance": float("nan")},
               {"t": 0}, {"camera": False}, {"params": False}]
        for kw in bad:
            with pytest.raises(R.RsrtError) as e:
                accumulate(st, 1, **kw)
            assert e.value.status == INVALID, kw
        with pytest.raises(R.RsrtError) as e:
            accumulate(st, 0)
        assert e.value.status == INVALID
        accumulate(st, 1, max_history=1 << 24, depth_tolerance=1e-6, normal_tolerance=-1.0)  # the ends of the ranges are valid
        import test_denoise_gpu
        other = test_denoise_gpu.DeviceArray(np.zeros((8, 8, 8), np.float32))
        st.bind_aov(other.data_ptr(), 8, 8)
        with pytest.raises(R.RsrtError) as e:
            accumulate(st, 1)
        assert e.value.status == INVALID  # AOV of another size
        st.bind_aov(None, 0, 0)
        st.set_partition(0, 2)
        with pytest.raises(R.RsrtError) as e:
            accumulate(st, 1)
        assert e.value.status == INVALID
        st.set_partition(0, 1)
    finally:
        st.close()
        bare.close()


def test_history_is_dropped():
    sc, st = state("house", 64, 40)
    try:
        st.render_temporal(1)
        st.render_temporal(1)
        assert (st.download_temporal()[..., 3] == 2).all()  # held camera: identity
        st.temporal_reset()
        st.render_temporal(1)
        assert first_frame(st, 1) and st.temporal_sample_count == 1
        st.render_temporal(2)
        assert (st.download_temporal()[..., 3] == 3).all()
        # the library drops it by itself: a new environment (same camera, so identity otherwise)
        st.upload_environment(0, R.Environment.synthetic(128, 64))
        st.clear()
        st.render_range(10, 1)
        st.clear_aov()
        st.render_aov(10, 1)
        accumulate(st, 1)
        assert first_frame(st, 1)
        accumulate(st, 1)
        assert (st.download_temporal()[..., 3] == 2).all()
        # ... a resize, back to the same size
        st.resize(64, 40)
        st.resize(48, 30)
        st.resize(64, 40)
        st.render_range(11, 1)
        st.render_aov(11, 1)
        with pytest.raises(R.RsrtError) as e:
            st.download_temporal()
        assert e.value.status == NOT_READY
        accumulate(st, 1)
        assert first_frame(st, 1)
        # ... and the State on a change of the render settings
        st.render_temporal(1)
        st.max_bounces = 3
        st.render_temporal(2)
        assert first_frame(st, 2) and st.temporal_sample_count == 2
    finally:
        st.close()


def test_cpp_state_matches_the_python_state(tmp_path):
    import subprocess
    import test_temporal
    exe = test_temporal.build_cpp_demo(tmp_path)
    w, h = 80, 48
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "8", "256", "128", str(tmp_path / "o.f32")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(tmp_path / "o.f32", np.float32).reshape(5, h, w, 4)
    sc, st = state("house", w, h)
    try:
        desc = desc_of(sc)
        for f, n in enumerate((1, 1, 2, 1)):
            aim(st, desc, 0.03 if f == 1 else 0.0, 0.02 if f == 3 else 0.0, (0.1, 0, 0) if f == 3 else (0, 0, 0))
            st.render_temporal(n)
            assert np.array_equal(util.bits(got[f]), util.bits(st.download_temporal())), f
        assert np.array_equal(util.bits(got[4]), util.bits(st.denoise(temporal=True)))
    finally:
        st.close()
