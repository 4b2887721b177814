"""The noise estimate on the GPU (rsrt_noise_snapshot, rsrt_noise_estimate, rsrt_noise_download): the kernel against its numpy
restatement, bit for bit, special pixels and partial tiles included; on a real render, with no effect on the accumulator; the documented
errors and what drops the snapshot; render_to_noise through the Python and the C++ State."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import noise_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray, state
from test_noise import COUNTS, FRAMES, TILES

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def same_summary(got, want):
    return all(got[k] == want[k] for k in ("tiles_x", "tiles_y", "tiles_above")) and same(got["max_error"], want["max_error"]) \
        and same(got["mean_error"], want["mean_error"])


def raises(status, call):
    with pytest.raises(R.RsrtError) as e:
        call()
    assert e.value.status == status, e.value


@pytest.mark.parametrize("h,w", FRAMES)
def test_kernel_equals_the_numpy_restatement_bit_for_bit(h, w):
    st = R.State()
    try:
        for n1, n2 in COUNTS:
            s1, s2, special = noise_ref.synthetic(h, w, n1, n2, seed=1000 * h + w)
            d1, d2 = DeviceArray(s1), DeviceArray(s2)
            st.bind_accumulator(d1.data_ptr(), w, h)
            st.noise_snapshot(sample_total=n1)
            st.bind_accumulator(d2.data_ptr(), w, h)  # the same size: the snapshot stays
            for tile in TILES:
                for threshold in (0.25, float("inf")):
                    got, gs = st.noise_estimate(tile, threshold, sample_total=n2)
                    want, ws = noise_ref.estimate(s1, n1, s2, n2, tile, threshold)
                    assert got.shape == want.shape and not np.isnan(got).any()
                    assert same(got, want), (n1, n2, tile)
                    assert same_summary(gs, ws), (n1, n2, tile, threshold, gs, ws)
                    if special:
                        assert np.isinf(got).any() and gs["tiles_above"] >= int(np.isinf(got).sum()) > 0
            assert util.same_bits_or_nan(d1.numpy(), s1) and util.same_bits_or_nan(d2.numpy(), s2)  # read only
    finally:
        st.close()


def test_estimate_of_a_real_render_reads_and_never_writes():
    w, h = 70, 37
    sc, st = state("default", w, h)
    _, plain = state("default", w, h)
    try:
        st.render_samples(4)
        a4 = st.download()
        st.noise_snapshot()
        assert same(st.download(), a4)
        st.render_samples(4)
        a8 = st.download()
        tiles, s = st.noise_estimate()
        want, ws = noise_ref.estimate(a4, 4, a8, 8)
        assert tiles.shape == (3, 5) and np.isfinite(tiles).all() and (tiles > 0).any()
        assert same(tiles, want) and same_summary(s, ws)
        t2, s2 = st.noise_download()
        assert same(t2, tiles) and s2 == s
        assert same(st.download(), a8)
        plain.render_samples(8)
        assert same(plain.download(), a8)
        assert st.sample_count == 8
    finally:
        st.close()
        plain.close()


def test_errors_and_what_drops_the_snapshot():
    sc, st = state("default", 32, 16)
    try:
        est = lambda **kw: st.noise_estimate(**{"sample_total": 8, **kw})  # noqa: E731
        raw = lambda n, params: st._check(st._L.rsrt_noise_estimate(st._ctx, n, params, None), "rsrt_noise_estimate")  # noqa: E731
        P = R.state.NoiseParams
        raises(NOT_READY, est)               # before a snapshot
        raises(NOT_READY, st.noise_download)  # before any estimate
        st.render_samples(4)
        raises(NOT_READY, est)
        st.noise_snapshot()
        st.render_samples(4)
        acc = st.download()
        tiles, s = est()
        # refused calls: nothing is launched, the last estimate and the accumulator stay what they were
        raises(INVALID, lambda: est(sample_total=4))   # n2 == n1
        raises(INVALID, lambda: est(sample_total=3))   # n2 < n1
        raises(INVALID, lambda: est(tile=(8, 6)))      # 48 pixels
        raises(INVALID, lambda: est(tile=(128, 64)))   # 8192 pixels
        raises(INVALID, lambda: est(tile=(0, 64)))
        raises(INVALID, lambda: est(threshold=float("nan")))
        raises(INVALID, lambda: est(threshold=-1.0))
        raises(INVALID, lambda: raw(8, C.byref(P(16, 16, 0.0, 1))))  # flags
        raises(INVALID, lambda: raw(8, None))                          # NULL params
        raises(INVALID, lambda: st.noise_snapshot(sample_total=0))
        bad = np.zeros(3, np.float32)
        raises(INVALID, lambda: st._check(st._L.rsrt_noise_download(st._ctx, R.state._p(bad), bad.size, None), "rsrt_noise_download"))
        st.set_partition(0, 2)
        raises(INVALID, est)
        raises(INVALID, st.noise_snapshot)
        raises(INVALID, st.noise_download)
        st.set_partition(0, 1)
        t2, s2 = st.noise_download()
        assert same(t2, tiles) and s2 == s and same(st.download(), acc)
        only = np.zeros(tiles.shape, np.float32)  # the tiles alone, the summary alone
        st._check(st._L.rsrt_noise_download(st._ctx, R.state._p(only), only.size, None), "rsrt_noise_download")
        assert same(only, tiles)
        assert est(threshold=float("inf"))[1]["tiles_above"] == 0  # +inf is a threshold
        # a reset, a clear, a resize and a bind of another size drop both; a later snapshot starts anew
        st.noise_reset()
        raises(NOT_READY, est)
        raises(NOT_READY, st.noise_download)
        assert same(st.download(), acc)
        st.noise_snapshot(sample_total=4)
        assert est()[0].shape == tiles.shape  # (the accumulator against itself at other counts)
        st.clear()
        raises(NOT_READY, est)
        raises(NOT_READY, st.noise_download)
        st.render_samples(2)
        st.noise_snapshot()
        st.render_samples(2)
        assert st.noise_estimate()[0].shape == (1, 2)
        st.resize(48, 16)
        raises(NOT_READY, lambda: st.noise_estimate(sample_total=8))
        raises(NOT_READY, st.noise_download)
        st.render_samples(2)
        st.noise_snapshot()
        st.render_samples(2)
        assert st.noise_estimate()[0].shape == (1, 3)
        mine = DeviceArray(np.ones((8, 16, 4), np.float32))
        st.bind_accumulator(mine.data_ptr(), 16, 8)  # another size
        raises(NOT_READY, lambda: st.noise_estimate(sample_total=8))
        raises(NOT_READY, st.noise_download)
        st.noise_snapshot(sample_total=1)
        got, _ = st.noise_estimate(tile=(8, 8), sample_total=2)  # a = 1, m = 1 / 2: |m - a| summed = 1.5, over sqrt(1.5 + 1e-3)
        assert got.shape == (1, 2) and same(got, noise_ref.estimate(mine.host, 1, mine.host, 2, (8, 8))[0])
    finally:
        st.close()


def test_no_accumulator_is_not_ready():
    st = R.State()
    try:
        raises(NOT_READY, lambda: st.noise_snapshot(sample_total=1))
        raises(NOT_READY, lambda: st.noise_estimate(sample_total=2))
    finally:
        st.close()


@pytest.mark.parametrize("threshold,total,pairs", [(float("inf"), 16, [(8, 16)]), (0.0, 64, [(8, 16), (16, 32), (32, 64)])])
def test_render_to_noise(threshold, total, pairs):
    w, h = 64, 36
    sc, st = state("spheres_only", w, h)
    _, man = state("spheres_only", w, h)
    try:
        st.render_samples(3)  # whatever was there before: it starts from a clear
        got_total, rounds = st.render_to_noise(threshold, min_samples=8, max_samples=64)
        assert got_total == total == st.sample_count and [(r[0], r[1]) for r in rounds] == pairs
        man.render_samples(pairs[0][0])
        for (n1, n2), r in zip(pairs, rounds):
            a1 = man.download()
            man.render_samples(n2 - n1)
            a2 = man.download()
            _, ws = noise_ref.estimate(a1, n1, a2, n2, (16, 16), threshold)
            assert same(r[2], ws["max_error"]) and same(r[3], ws["mean_error"]) and r[4] == ws["tiles_above"], (n1, n2, r, ws)
        assert same(st.download(), man.download())  # man: render_samples from a clear, in other steps — equal to one call too:
        man.clear()
        man.render_samples(total)
        assert same(st.download(), man.download())
        assert same(st.noise_download()[0], noise_ref.estimate(a1, n1, a2, n2)[0])
    finally:
        st.close()
        man.close()


def test_cpp_state_renders_to_noise_like_the_python_state(tmp_path):
    import test_noise
    exe = test_noise.build_cpp_demo(tmp_path)
    w, h = 64, 36
    r = subprocess.run([exe, util.scene_path("spheres_only"), str(w), str(h), "8", "256", "128", "0", "8", "64", str(tmp_path / "t.f32")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines()]
    cpp_rounds = [(int(f[1]), int(f[2]), float.fromhex(f[3]), float.fromhex(f[4]), int(f[5])) for f in lines if f and f[0] == "round"]
    tail = next(f for f in lines if f and f[0] == "total")
    sc, st = state("spheres_only", w, h)
    try:
        total, rounds = st.render_to_noise(0.0, min_samples=8, max_samples=64)
        tiles, _ = st.noise_download()
        assert (int(tail[1]), int(tail[3]), int(tail[4])) == (total, tiles.shape[1], tiles.shape[0])
        assert cpp_rounds == rounds and len(rounds) == 3
        assert same(np.fromfile(tmp_path / "t.f32", np.float32).reshape(tiles.shape), tiles)
    finally:
        st.close()
