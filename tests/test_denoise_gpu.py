"""The denoiser on the GPU (rsrt_aov_render, rsrt_denoise): the AOV records against the checker's closest hits of the restated camera
rays, the filter against its numpy restatement, bit for bit; no effect on the accumulator; a real reduction of the noise; the
documented errors."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import util
import rsoderh_raytracing_amd as R

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4


def state(name, w, h, bounces=8):
    sc = R.Scene.load_toml(util.scene_path(name))
    st = R.State.new(sc, R.Environment.synthetic(256, 128), w, h)
    st.max_bounces = bounces
    return sc, st


@pytest.mark.parametrize("name,w,h", [("default", 64, 48), ("house", 160, 90), ("suzanne", 96, 64)])
def test_aov_records_equal_the_checker_hits_bit_for_bit(name, w, h):
    sc, st = state(name, w, h)
    try:
        st.render_aov(3, 4)
        got = st.download_aov()
        want = denoise_ref.aov_records(sc, util.oracle_scene(sc), st.camera[0], w, h, 3, 4)
        assert want[..., 3].max() == 4 and want[..., 3].sum() > 0
        assert np.array_equal(util.bits(got), util.bits(want))
        st.clear_aov()
        assert not st.download_aov().any()
        st.render_aov(3, 2)
        st.render_aov(5, 2)
        assert np.array_equal(util.bits(st.download_aov()), util.bits(got))  # [3,5) + [5,7) = [3,7)
    finally:
        st.close()


def hip_runtime_path():
    """The HIP runtime librsrt.so is bound to: the one from the ROCm install, or torch's copy when torch was loaded first (then the
    loader gave librsrt that one, same soname)."""
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln}, key=lambda q: "torch" in q)
    return paths[0]


class DeviceArray:
    """Caller-owned device memory for the bind calls, from the HIP runtime librsrt.so itself is linked against (torch brings a HIP runtime
    of its own; buffers are not passed between the two)."""

    def __init__(self, host):
        R.state.lib()
        self.L = C.CDLL(hip_runtime_path())
        self.host = np.ascontiguousarray(host, np.float32)
        self.ptr = C.c_void_p()
        assert self.L.hipMalloc(C.byref(self.ptr), C.c_size_t(max(self.host.nbytes, 16))) == 0
        assert self.L.hipMemcpy(self.ptr, self.host.ctypes.data_as(C.c_void_p), C.c_size_t(self.host.nbytes), 1) == 0  # host to device

    def data_ptr(self):
        return self.ptr.value

    def numpy(self):
        out = np.empty_like(self.host)
        assert self.L.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0  # device to host
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            self.L.hipFree(self.ptr)


def bound(h, w, sums, aov):
    acc, aov_t = DeviceArray(sums), DeviceArray(aov)
    st = R.State()
    st.bind_accumulator(acc.data_ptr(), w, h)
    st.bind_aov(aov_t.data_ptr(), w, h)
    return st, acc, aov_t


@pytest.mark.parametrize("h,w", [(91, 173), (1, 1), (300, 7)])
def test_filter_equals_the_numpy_restatement_bit_for_bit(h, w):
    import test_denoise
    sums, aov = test_denoise.synthetic(h, w, 4, 3, seed=11 * h + w)
    st, acc, aov_t = bound(h, w, sums, aov)
    try:
        for iters in range(7):
            for demod in (True, False):
                got = st.denoise(iters, 2.0, 0.3, 0.2, demod, sample_total=4, aov_sample_total=3)
                want = denoise_ref.denoise(sums, aov, 4, 3, iters, 2.0, 0.3, 0.2, demod)
                assert np.array_equal(util.bits(got[..., :3]), util.bits(want)), (iters, demod)
                assert (got[..., 3] == 1.0).all()
                if iters == 0:
                    assert np.array_equal(got[..., :3], sums[..., :3] / np.float32(4))
        out = DeviceArray(np.zeros((h, w, 4), np.float32))  # into a caller's buffer
        st.denoise(4, sample_total=4, aov_sample_total=3, out_ptr=out.data_ptr(), download=False)
        st.synchronize()
        want = denoise_ref.denoise(sums, aov, 4, 3, 4)
        assert np.array_equal(util.bits(out.numpy()[..., :3]), util.bits(want))
        assert np.array_equal(util.bits(acc.numpy()), util.bits(sums)) and np.array_equal(util.bits(aov_t.numpy()), util.bits(aov))
    finally:
        st.close()


def test_passes_leave_the_accumulator_alone():
    sc, st = state("house", 96, 54)
    _, ref = state("house", 96, 54)
    try:
        st.render_samples(3, aov=True)
        ref.render_samples(3)
        a = st.download()
        assert np.array_equal(util.bits(a), util.bits(ref.download()))
        assert st.aov_sample_count == 3 and st.download_aov()[..., 3].max() == 3
        st.render_aov(10, 2)
        st.denoise()
        disp = st.denoised_display_srgb8()
        assert disp.shape == (54, 96, 4) and (disp[..., 3] == 255).all()
        assert np.array_equal(util.bits(st.download()), util.bits(a))
        st.camera = st.camera.copy()
        st.camera["pos"][0][0] += 0.25  # a new camera: the scene-hash reset clears the AOV buffer too
        st.render_samples(1)
        assert not st.download_aov().any() and st.aov_sample_count == 0
    finally:
        st.close()
        ref.close()


def display_rmse(a, b):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).mean()))


@pytest.mark.parametrize("name,w,h,limit", [("house", 320, 180, 0.6), ("suzanne", 256, 144, 0.9)])
def test_denoised_image_is_closer_to_the_reference(name, w, h, limit):
    """4 spp (samples 0-3) against 1024 spp from disjoint samples (1000-2023), as the user sees them: the display pass's sRGB bytes
    (the linear error of a 4-spp image is fireflies, which an edge-stopping filter keeps by design)."""
    sc, st = state(name, w, h)
    try:
        st.render_range(1000, 1024)
        ref = R.host.display_srgb8(st.download(), 1024)
        st.clear()
        st.render_samples(4, aov=True)
        noisy = st.display_srgb8()
        st.denoise()
        den = st.denoised_display_srgb8()
        ratio = display_rmse(den, ref) / display_rmse(noisy, ref)
        print("%s %dx%d: display RMSE noisy %.2f, denoised %.2f, ratio %.3f" % (name, w, h, display_rmse(noisy, ref), display_rmse(den, ref), ratio))
        assert ratio <= limit
    finally:
        st.close()


def test_normal_step_keeps_its_two_colours():
    h, w = 64, 96
    sums = np.zeros((h, w, 4), np.float32)
    aov = np.zeros((h, w, 8), np.float32)
    left = np.arange(w) < w // 2
    sums[..., :3] = np.where(left[None, :, None], np.float32([0.9, 0.2, 0.1]), np.float32([0.1, 0.3, 0.9])) * 4
    aov[..., :3], aov[..., 3] = 4 * 0.5, 4  # one albedo: only the normals tell the halves apart
    aov[..., 4:7] = np.where(left[None, :, None], np.float32([1, 0, 0]), np.float32([0, 0, 1])) * 4
    aov[..., 7] = 4 * 2.0
    st, acc, aov_t = bound(h, w, sums, aov)
    try:
        out = st.denoise(5, sigma_color=1e3, sigma_normal=0.01, sample_total=4, aov_sample_total=4)
        want = sums[..., :3] / 4
        assert np.allclose(out[..., :3], want, rtol=0.01, atol=0)
        blur = st.denoise(5, sigma_color=1e3, sigma_normal=1e3, sample_total=4, aov_sample_total=4)  # without the normal weight it bleeds
        assert not np.allclose(blur[:, w // 2 - 1, :3], want[:, w // 2 - 1], rtol=0.01, atol=0)
    finally:
        st.close()


def test_errors():
    sc, st = state("default", 32, 16)
    try:
        with pytest.raises(R.RsrtError) as e:
            st.denoise(sample_total=1, aov_sample_total=1)
        assert e.value.status == NOT_READY  # no AOV buffer
        st.render_samples(1, aov=True)
        with pytest.raises(R.RsrtError) as e:
            st.denoise(9)
        assert e.value.status == INVALID
        for bad in ({"sigma_color": 0.0}, {"sample_total": 0}):
            with pytest.raises(R.RsrtError) as e:
                st.denoise(**bad)
            assert e.value.status == INVALID
        other = DeviceArray(np.zeros((8, 8, 8), np.float32))
        st.bind_aov(other.data_ptr(), 8, 8)  # size mismatch
        with pytest.raises(R.RsrtError) as e:
            st.denoise()
        assert e.value.status == INVALID
        st.bind_aov(None, 0, 0)
        st.set_partition(0, 2)
        for call in (lambda: st.render_aov(0, 1), lambda: st.denoise()):
            with pytest.raises(R.RsrtError) as e:
                call()
            assert e.value.status == INVALID
        st.set_partition(0, 1)
        with pytest.raises(R.RsrtError) as e:
            st._check(st._L.rsrt_aov_render(st._ctx, R.state._p(st.camera), 32, 16, 0, 1, 1, None), "rsrt_aov_render")  # flags must be 0
        assert e.value.status == INVALID
    finally:
        st.close()


def test_cpp_state_denoises_like_the_python_state(tmp_path):
    import subprocess
    import test_denoise
    exe = test_denoise.build_cpp_demo(tmp_path)
    w, h = 80, 48
    r = subprocess.run([exe, util.scene_path("house"), str(w), str(h), "4", "8", "256", "128", str(tmp_path / "o.f32")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(tmp_path / "o.f32", np.float32).reshape(h, w, 4)
    sc, st = state("house", w, h)
    try:
        st.render_samples(4, aov=True)
        assert np.array_equal(util.bits(got), util.bits(st.denoise()))
    finally:
        st.close()
