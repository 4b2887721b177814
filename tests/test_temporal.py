"""The temporal pass without a GPU: its published per-pixel arithmetic (include/rsrt_temporal.h), compiled for the CPU, against the
numpy restatement the GPU tests hold the kernel to (tests/temporal_ref.py), bit for bit, on synthetic frame sequences; the camera
mapping's round trip; the ABI and the parameter defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as T
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tp") / "libtp.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "temporal_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.tp_frame.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 4 + [C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 3
    L.tp_roundtrip.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    return L


def cam_array(cam):
    return np.concatenate([cam.pos, cam.rot.reshape(9), [cam.fov_y]]).astype(np.float32)


class HostSequence:
    """The header's pass over frames, through tests/cpp/temporal_host.cpp."""

    def __init__(self, L, max_history=32, depth_tolerance=0.05, normal_tolerance=0.9):
        self.L, self.p = L, (max_history, depth_tolerance, normal_tolerance)
        self.cam = self.col = self.feat = None

    def frame(self, sums, aov, S, Tn, cam):
        h, w = sums.shape[:2]
        sums, aov = np.ascontiguousarray(sums, np.float32), np.ascontiguousarray(aov, np.float32)
        col, feat, code = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32)
        ca = cam_array(cam)
        pa = cam_array(self.cam) if self.cam is not None else None
        pc = self.col if self.col is not None else np.zeros((h, w, 4), np.float32)
        pf = self.feat if self.feat is not None else np.zeros((h, w, 4), np.float32)
        self.L.tp_frame(sums.ctypes.data, aov.ctypes.data, w, h, S, Tn, ca.ctypes.data, pa.ctypes.data if pa is not None else None,
                        pc.ctypes.data, pf.ctypes.data, *self.p, col.ctypes.data, feat.ctypes.data, code.ctypes.data)
        self.cam, self.col, self.feat = cam, col, feat
        return col, code


# -------------------------------------------------------------------------------------------------- synthetic frames
def look(pos, yaw, pitch, fov):
    """A camera at pos turned by yaw (about y) and pitch (about x); it looks down its -z axis."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = ry @ rx  # columns: the camera's right, up and back axes in the world
    return T.Camera(pos, m.T, fov)  # rot[j] = column j


def scene_hits(cam, w, h):
    """First hits of the centre rays in a small analytic scene: a floor (y = 0), a raised block top (y = 0.6 over x in [-0.5, 0.8],
    z in [-4, -2.5]: a depth step), a back wall (z = -7, y < 3) with a rough patch, sky above.  -> z, normal, rough mask (z = inf: sky)."""
    ys, xs = np.mgrid[0:h, 0:w]
    d = T.center_ray(cam, w, h, xs, ys).astype(np.float64)
    o = cam.pos.astype(np.float64)
    z = np.full((h, w), np.inf)
    n = np.zeros((h, w, 3))
    rough = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        t = -o[1] / d[..., 1]  # floor
        hit = t > 0
        z, n = np.where(hit, t, z), np.where(hit[..., None], [0.0, 1.0, 0.0], n)
        t = (0.6 - o[1]) / d[..., 1]  # block top
        p = o + t[..., None] * d
        hit = (t > 0) & (t < z) & (p[..., 0] >= -0.5) & (p[..., 0] <= 0.8) & (p[..., 2] >= -4) & (p[..., 2] <= -2.5)
        z, n = np.where(hit, t, z), np.where(hit[..., None], [0.0, 1.0, 0.0], n)
        t = (-7 - o[2]) / d[..., 2]  # back wall
        p = o + t[..., None] * d
        hit = (t > 0) & (t < z) & (p[..., 1] >= 0) & (p[..., 1] < 3)
        z, n = np.where(hit, t, z), np.where(hit[..., None], [0.0, 0.0, 1.0], n)
        rough = hit & (p[..., 0] > 0.5) & (p[..., 0] < 3) & (p[..., 1] > 1)
    return z, n, rough


def synthetic_frame(cam, w, h, S, Tn, rng):
    """Noisy sums of S samples and AOV records of Tn samples of the analytic scene seen from cam: partial hits at random pixels,
    jittered normals and depths, and on the rough patch a fresh random normal every frame."""
    z, n, rough = scene_hits(cam, w, h)
    surf = np.isfinite(z)
    hits = np.where(surf, Tn, 0).astype(np.float32)
    flip = rng.random((h, w)) < 0.05
    hits[flip] = rng.integers(0, Tn + 1, flip.sum())
    tilt = np.where(rough[..., None], rng.normal(0, 0.8, (h, w, 3)), rng.normal(0, 0.01, (h, w, 3)))
    nn = n + tilt
    nn /= np.linalg.norm(nn, axis=-1, keepdims=True)
    zz = np.where(surf, z, 0.0) * (1 + rng.normal(0, 0.002, (h, w)))
    aov = np.zeros((h, w, 8), np.float32)
    aov[..., :3] = 0.7 * hits[..., None]
    aov[..., 3] = hits
    aov[..., 4:7] = nn * hits[..., None]
    aov[..., 7] = zz * hits
    base = np.where(surf[..., None], 0.3 + 0.2 * n, [0.6, 0.7, 0.9])
    sums = np.zeros((h, w, 4), np.float32)
    sums[..., :3] = np.maximum(base * S + rng.normal(0, 0.3, (h, w, 3)) * np.sqrt(S), 0)
    sums[..., 3] = 1.0
    return sums, aov


P0 = ((0.0, 1.2, 2.0), 0.0, -0.15, 0.9)
PATHS = {
    "translate": [P0, ((0.15, 1.2, 2.0), 0.0, -0.15, 0.9), ((0.3, 1.25, 1.9), 0.0, -0.15, 0.9)],
    "yaw_pitch": [P0, ((0.0, 1.2, 2.0), 0.06, -0.15, 0.9), ((0.0, 1.2, 2.0), 0.06, -0.1, 0.9)],
    "fov": [P0, ((0.0, 1.2, 2.0), 0.0, -0.15, 0.8), ((0.0, 1.2, 2.0), 0.0, -0.15, 0.8)],  # the last: unchanged
    "backward": [P0, ((0.0, 1.2, 4.5), 0.0, -0.15, 0.9), ((0.1, 1.2, 4.5), 0.02, -0.15, 0.9)],
    "still": [P0, P0, P0],
}


@pytest.mark.parametrize("w,h", [(64, 48), (61, 37)])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_header_arithmetic_matches_numpy_bit_for_bit(host, w, h, path):
    rng = np.random.default_rng(w * 100 + h + len(path))
    ref, dev = T.Sequence(), HostSequence(host)
    for i, (pos, yaw, pitch, fov) in enumerate(PATHS[path]):
        cam = look(pos, yaw, pitch, fov)
        S, Tn = 1 + i % 2, 1 + (i + 1) % 2
        sums, aov = synthetic_frame(cam, w, h, S, Tn, rng)
        got, gcode = dev.frame(sums, aov, S, Tn, cam)
        want, wcode = ref.frame(sums, aov, S, Tn, cam)
        assert np.array_equal(gcode, wcode), (path, i)
        assert np.array_equal(util.bits(got), util.bits(want)), (path, i)
        assert np.array_equal(util.bits(dev.feat), util.bits(ref.feat)), (path, i)


def test_every_branch_occurs_bit_for_bit(host):
    """One longer sequence through every camera change, with the tolerances at their defaults: each of the pass's outcomes occurs."""
    w, h = 96, 64
    rng = np.random.default_rng(5)
    ref, dev = T.Sequence(), HostSequence(host)
    seen = np.zeros(len(T.CODE_NAMES), np.int64)
    path = PATHS["translate"] + PATHS["yaw_pitch"][1:] + [((0.0, 1.2, 2.0), 0.7, -0.15, 0.9)] + PATHS["backward"] + PATHS["fov"][1:]
    for i, (pos, yaw, pitch, fov) in enumerate(path):
        cam = look(pos, yaw, pitch, fov)
        sums, aov = synthetic_frame(cam, w, h, 1, 2, rng)
        got, gcode = dev.frame(sums, aov, 1, 2, cam)
        want, wcode = ref.frame(sums, aov, 1, 2, cam)
        assert np.array_equal(gcode, wcode) and np.array_equal(util.bits(got), util.bits(want)), i
        seen += np.bincount(wcode.reshape(-1), minlength=len(seen))
    print(dict(zip(T.CODE_NAMES, seen.tolist())))
    assert (seen > 0).all(), dict(zip(T.CODE_NAMES, seen.tolist()))


def test_unchanged_camera_converges_like_the_accumulator(host):
    """Identity frames: the weight counts the samples exactly and the colour stays within 1e-6 of the plain mean."""
    w, h = 40, 30
    rng = np.random.default_rng(9)
    cam = look(*P0)
    dev = HostSequence(host, max_history=8)
    total = np.zeros((h, w, 4), np.float32)
    for i in range(8):
        sums, aov = synthetic_frame(cam, w, h, 1, 1, rng)
        total[..., :3] += sums[..., :3]
        got, code = dev.frame(sums, aov, 1, 1, cam)
        assert (code == (T.FIRST if i == 0 else T.IDENTITY)).all()
    assert (got[..., 3] == 8).all()
    assert np.allclose(got[..., :3], total[..., :3] / np.float32(8), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("w,h", [(160, 90), (64, 48), (7, 5), (1920, 1080)])
@pytest.mark.parametrize("z", [0.01, 1.0, 37.5, 1e4])
def test_centre_ray_projects_back_to_its_pixel(host, w, h, z):
    """The projection inverts start_path's mapping: pixel x aims at fx = x (not x + 0.5), and sy points up."""
    cam = look((0.3, -1.0, 2.0), 0.4, -0.3, 0.7)
    fx, fy = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32)
    ca = cam_array(cam)
    host.tp_roundtrip(ca.ctypes.data, w, h, z, fx.ctypes.data, fy.ctypes.data)
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.abs(fx - xs.reshape(-1)).max() < 1e-3 and np.abs(fy - ys.reshape(-1)).max() < 1e-3
    # the restatement agrees
    d = T.center_ray(cam, w, h, xs, ys)
    rx, ry, front = T.project(cam, w, h, np.float32(z) * d)
    assert front.all() and np.array_equal(util.bits(rx.reshape(-1)), util.bits(fx)) and np.array_equal(util.bits(ry.reshape(-1)), util.bits(fy))


def test_temporal_defaults_match_the_header():
    from rsoderh_raytracing_amd import state
    hdr = open(os.path.join(util.ROOT, "include", "rsrt_temporal.h")).read()
    assert "#define RSRT_TP_MAX_HISTORY 32u" in hdr and "#define RSRT_TP_DEPTH_TOLERANCE 0.05f" in hdr
    assert "#define RSRT_TP_NORMAL_TOLERANCE 0.9f" in hdr and "#define RSRT_TP_MIN_WEIGHT 0.01f" in hdr
    assert "max_history 32 samples (in [1, 2^24]), depth_tolerance tau_z 0.05 (in [1e-6, 1e6]), normal_tolerance tau_n 0.9 (in [-1, 1])" in hdr
    assert state.TEMPORAL_DEFAULTS == T.DEFAULTS == {"max_history": 32, "depth_tolerance": 0.05, "normal_tolerance": 0.9}
    assert C.sizeof(state.TemporalParams) == 12
    assert state.DENOISE_TEMPORAL == 2


def test_library_exports_the_temporal_pass():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_temporal_accumulate", "rsrt_temporal_reset", "rsrt_temporal_download"):
        assert hasattr(lib, n), n
    for n in ("render_temporal", "temporal_reset", "download_temporal"):
        assert hasattr(R.State, n), n


def test_temporal_kernel_uses_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = [n for n in md if "rt_temporal_kernel" in n]
    assert len(names) == 1, names
    assert md[names[0]]["private_segment_fixed_size"] == 0 and md[names[0]]["vgpr_spill_count"] == 0, md[names[0]]


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "temporal_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "temporal_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_temporal_compiles(tmp_path):
    build_cpp_demo(tmp_path)
