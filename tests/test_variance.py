"""The variance guidance without a GPU: the temporal moments (include/rsrt_temporal.h) and the variance-guided filter with the firefly
clamp (include/rsrt_variance.h), compiled for the CPU, against the numpy restatement the GPU tests hold the kernels to
(tests/variance_ref.py), bit for bit, on synthetic inputs that reach every branch; the ABI, the defaults and the kernels' resources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import temporal_ref as T
import test_denoise
import test_temporal
import util
import variance_ref as V
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sv") / "libsv.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "variance_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.sv_moments_frame.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 5 + [C.c_uint32, C.c_float, C.c_float] + \
        [C.c_void_p] * 4
    L.sv_filter.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3
    return L


class HostMoments:
    """The header's MOMENTS pass over frames, through tests/cpp/variance_host.cpp."""

    def __init__(self, L, max_history=32, depth_tolerance=0.05, normal_tolerance=0.9):
        self.L, self.p = L, (max_history, depth_tolerance, normal_tolerance)
        self.cam = self.col = self.feat = self.mom = None

    def frame(self, sums, aov, S, Tn, cam):
        h, w = sums.shape[:2]
        sums, aov = np.ascontiguousarray(sums, np.float32), np.ascontiguousarray(aov, np.float32)
        col, feat, mom = (np.zeros((h, w, 4), np.float32) for _ in range(3))
        code = np.zeros((h, w), np.int32)
        ca = test_temporal.cam_array(cam)
        pa = test_temporal.cam_array(self.cam) if self.cam is not None else None
        z = np.zeros((h, w, 4), np.float32)
        pc, pf, pm = (x if x is not None else z for x in (self.col, self.feat, self.mom))
        self.L.sv_moments_frame(sums.ctypes.data, aov.ctypes.data, w, h, S, Tn, ca.ctypes.data, pa.ctypes.data if pa is not None else None,
                                pc.ctypes.data, pf.ctypes.data, pm.ctypes.data, *self.p, col.ctypes.data, feat.ctypes.data, mom.ctypes.data,
                                code.ctypes.data)
        self.cam, self.col, self.feat, self.mom = cam, col, feat, mom
        return col, mom, code


def host_filter(L, sums, aov, S, Tn, iters, sc, sn, sz, demod, variance, clamp, mom=None):
    h, w = sums.shape[:2]
    sums, aov = np.ascontiguousarray(sums, np.float32), np.ascontiguousarray(aov, np.float32)
    out, v = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    m = np.ascontiguousarray(mom, np.float32) if mom is not None else None
    L.sv_filter(sums.ctypes.data, aov.ctypes.data, w, h, S, Tn, iters, sc, sn, sz, int(demod), int(variance), int(clamp),
                m.ctypes.data if m is not None else None, out.ctypes.data, v.ctypes.data)
    return out, v


# -------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("w,h", [(64, 48), (61, 37)])
@pytest.mark.parametrize("path", sorted(test_temporal.PATHS))
def test_moments_match_numpy_bit_for_bit(host, w, h, path):
    rng = np.random.default_rng(w * 100 + h + len(path) + 7)
    ref, dev, plain = V.MomentSequence(), HostMoments(host), T.Sequence()
    for i, (pos, yaw, pitch, fov) in enumerate(test_temporal.PATHS[path]):
        cam = test_temporal.look(pos, yaw, pitch, fov)
        S, Tn = 1 + i % 2, 1 + (i + 1) % 2
        sums, aov = test_temporal.synthetic_frame(cam, w, h, S, Tn, rng)
        gcol, gmom, gcode = dev.frame(sums, aov, S, Tn, cam)
        wcol, wmom, wcode = ref.frame(sums, aov, S, Tn, cam)
        pcol, pcode = plain.frame(sums, aov, S, Tn, cam)
        assert np.array_equal(gcode, wcode) and np.array_equal(gcode, pcode), (path, i)
        assert np.array_equal(util.bits(gcol), util.bits(pcol)) and np.array_equal(util.bits(wcol), util.bits(pcol)), (path, i)  # = a plain frame
        assert np.array_equal(util.bits(gmom), util.bits(wmom)), (path, i)


def test_moments_every_branch_and_a_still_camera(host):
    """A sequence through every camera change, then a held camera: first frames, identity, reprojection, rejection; frames < 4 and >= 4;
    scale falls as S / (samples so far) while the camera holds."""
    w, h = 96, 64
    rng = np.random.default_rng(15)
    ref, dev = V.MomentSequence(), HostMoments(host)
    P = test_temporal.PATHS
    path = P["translate"] + P["yaw_pitch"][1:] + [((0.0, 1.2, 2.0), 0.7, -0.15, 0.9)] + P["backward"] + [P["backward"][-1]] * 5
    seen = np.zeros(len(T.CODE_NAMES), np.int64)
    few = many = 0
    for i, (pos, yaw, pitch, fov) in enumerate(path):
        cam = test_temporal.look(pos, yaw, pitch, fov)
        sums, aov = test_temporal.synthetic_frame(cam, w, h, 1, 2, rng)
        _, gmom, gcode = dev.frame(sums, aov, 1, 2, cam)
        _, wmom, wcode = ref.frame(sums, aov, 1, 2, cam)
        assert np.array_equal(gcode, wcode) and np.array_equal(util.bits(gmom), util.bits(wmom)), i
        seen += np.bincount(wcode.reshape(-1), minlength=len(seen))
        few, many = few + int((gmom[..., 2] < 4).sum()), many + int((gmom[..., 2] >= 4).sum())
    print(dict(zip(T.CODE_NAMES, seen.tolist())), "frames < 4: %d, >= 4: %d" % (few, many))
    assert (seen > 0).all() and few > 0 and many > 0
    # the last 6 frames held the camera: identity everywhere, 6 more frames, scale = 1 / (nh + 1) with the weight from the history
    assert (gcode == T.IDENTITY).all()
    assert np.array_equal(util.bits(gmom[..., 3]), util.bits(np.float32(1) / dev.col[..., 3]))


def test_moments_toggle_and_first_frame(host):
    """Numpy's MomentSequence drops the history on a toggle, as the library does; a first frame's record is (l, l^2, 1, 1)."""
    w, h = 40, 30
    rng = np.random.default_rng(3)
    cam = test_temporal.look(*test_temporal.P0)
    seq = V.MomentSequence()
    sums, aov = test_temporal.synthetic_frame(cam, w, h, 1, 1, rng)
    _, m, code = seq.frame(sums, aov, 1, 1, cam)
    l = V.lum(V.prepare(sums, aov, 1, 1))
    assert (code == T.FIRST).all() and np.array_equal(util.bits(m), util.bits(np.stack([l, l * l, np.ones_like(l), np.ones_like(l)], -1)))
    seq.frame(sums, aov, 1, 1, cam, moments=False)
    _, m, code = seq.frame(sums, aov, 1, 1, cam)
    assert (code == T.FIRST).all() and (m[..., 2] == 1).all()
    _, m, code = seq.frame(sums, aov, 1, 1, cam)
    assert (code == T.IDENTITY).all() and (m[..., 2] == 2).all() and (m[..., 3] == np.float32(0.5)).all()


# -------------------------------------------------------------------------------------------------- filter
def synthetic_moments(h, w, seed):
    """Moment records with frames on both sides of 4, some with mu2 < mu1^2 (v = 0) and scale in (0, 1]."""
    rng = np.random.default_rng(seed)
    mu1 = rng.uniform(0, 2, (h, w))
    m = np.stack([mu1, mu1 * mu1 + rng.normal(0.05, 0.1, (h, w)), rng.integers(1, 9, (h, w)), rng.uniform(0.05, 1, (h, w))], -1)
    return m.astype(np.float32)


def with_fireflies(sums, seed, frac=0.02):
    rng = np.random.default_rng(seed)
    s = sums.copy()
    hot = rng.random(s.shape[:2]) < frac
    s[hot, :3] *= np.float32(40.0)
    return s


VARIANTS = [(True, True, True), (True, True, False), (True, False, True), (False, False, True)]  # demodulate, variance, clamp


@pytest.mark.parametrize("h,w", [(91, 173), (1, 1), (300, 7), (2, 3)])
@pytest.mark.parametrize("iters", [0, 1, 2, 5, 8])
@pytest.mark.parametrize("temporal", [False, True])
def test_filter_matches_numpy_bit_for_bit(host, h, w, iters, temporal):
    sums, aov = test_denoise.synthetic(h, w, 4, 3, seed=h * 1000 + w + iters)
    sums = with_fireflies(sums, h + w)
    mom = synthetic_moments(h, w, h * w + iters) if temporal else None
    for demod, variance, clamp in VARIANTS:
        if variance is False and temporal:
            continue
        sc = 4.0 if variance else 2.0
        got, _ = host_filter(host, sums, aov, 4, 3, iters, sc, 0.3, 0.2, demod, variance, clamp, mom)
        want = V.denoise(sums, aov, 4, 3, iters, sc, 0.3, 0.2, demod, variance, clamp, mom)
        assert np.array_equal(util.bits(got), util.bits(want)), (demod, variance, clamp)
        if iters == 0:
            assert np.array_equal(got, sums[..., :3] / np.float32(4))


def test_filter_branches_occur(host):
    """Clamp hits and misses (borders included), v = 0, the temporal and the spatial estimate: each occurs, and the host's variance
    before the first level equals the restatement's."""
    h, w = 61, 89
    sums, aov = test_denoise.synthetic(h, w, 4, 3, seed=5)
    sums = with_fireflies(sums, 5)
    r = V.prepare(sums, aov, 4, 3)
    clamped, hit = V.clamp(r)
    border = np.zeros((h, w), bool)
    border[[0, -1], :] = border[:, [0, -1]] = True
    assert hit.any() and (~hit).any() and (hit & border).any() and (~hit & border).any()
    assert np.array_equal(util.bits(clamped[~hit]), util.bits(r[~hit]))
    f = denoise_ref.features(aov, 3)
    m = synthetic_moments(h, w, 9)
    v, temporal = V.variance(m, f, 0.3, 0.2)
    assert temporal.any() and (~temporal).any() and (v == 0).any() and (v > 0).any()
    _, gv = host_filter(host, sums, aov, 4, 3, 1, 4.0, 0.3, 0.2, True, True, True, m)
    assert np.array_equal(util.bits(gv), util.bits(v))
    l = V.lum(r)
    v0, _ = V.variance(np.stack([l, l * l, np.ones_like(l), np.ones_like(l)], -1), f, 0.3, 0.2)
    _, gv0 = host_filter(host, sums, aov, 4, 3, 1, 4.0, 0.3, 0.2, True, True, False)
    assert np.array_equal(util.bits(gv0), util.bits(v0)) and (v0 > 0).all()


def test_clamp_removes_an_isolated_firefly_only():
    r = np.full((5, 6, 3), 0.5, np.float32)
    r[2, 3] = [40.0, 30.0, 20.0]  # a firefly
    r[0, 0] = [0.6, 0.6, 0.6]     # a local maximum at the border
    r[4, 1] = r[4, 2] = [3.0, 3.0, 3.0]  # two equal bright neighbours: neither is a strict maximum
    out, hit = V.clamp(r)
    assert hit[2, 3] and hit[0, 0] and not hit[4, 1] and not hit[4, 2] and hit.sum() == 2
    assert abs(V.lum(out[2, 3]) - V.lum(r[2, 2])) < 1e-6 and np.allclose(out[2, 3] / r[2, 3], out[2, 3, 0] / r[2, 3, 0])
    one, hit1 = V.clamp(np.full((1, 1, 3), 9.0, np.float32))
    assert not hit1.any() and (one == 9.0).all()


def test_variance_defaults_match_the_header(host):
    from rsoderh_raytracing_amd import state
    mf, eps, sl, rad = C.c_float(), C.c_float(), C.c_float(), C.c_int()
    host.sv_defaults(C.byref(mf), C.byref(eps), C.byref(sl), C.byref(rad))
    assert (mf.value, rad.value) == (4.0, 3) and sl.value == 4.0 and eps.value == np.float32(1e-6)
    assert V.MIN_FRAMES == mf.value and V.EPS == np.float32(eps.value) and V.SIGMA_L == sl.value and V.RADIUS == rad.value
    assert state.VARIANCE_SIGMA_L == 4.0 and (state.TEMPORAL_MOMENTS, state.DENOISE_VARIANCE, state.DENOISE_CLAMP) == (1, 4, 8)
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_TEMPORAL_MOMENTS = 1u" in hdr and "RSRT_DENOISE_VARIANCE = 4u, RSRT_DENOISE_CLAMP = 8u" in hdr
    assert "default RSRT_SV_SIGMA_L 4.0" in hdr
    assert C.sizeof(state.TemporalParams) == 12 and C.sizeof(state.DenoiseParams) == 20


def test_library_exports_the_variance_guidance():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_temporal_accumulate_ex", "rsrt_temporal_moments_download"):
        assert hasattr(lib, n), n
    assert hasattr(R.State, "download_temporal_moments")
    import inspect
    assert "moments" in inspect.signature(R.State.render_temporal).parameters
    assert {"variance", "clamp"} <= set(inspect.signature(R.State.denoise).parameters)


def test_variance_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = [n for n in md if "rt_sv_" in n or "rt_temporal_moments_kernel" in n]
    assert len(names) == 5, names
    for n in names:
        assert md[n]["private_segment_fixed_size"] == 0 and md[n]["vgpr_spill_count"] == 0, (n, md[n])


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "variance_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "variance_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_variance_compiles(tmp_path):
    build_cpp_demo(tmp_path)
