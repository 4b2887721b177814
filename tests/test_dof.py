"""Depth of field without a GPU: its published arithmetic (include/rsrt_dof.h), compiled for the CPU, against the numpy restatement the
GPU tests hold the kernels to (tests/dof_ref.py), bit for bit, special pixels included; the distance table; identity at aperture 0 and
on the focus plane; the occlusion rule both ways; energy and support of one bright pixel; the tap order; the parameter check; the ABI
and the kernels' code objects."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dof_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (3, 5), (17, 33), (40, 56)]  # (h, w)
RADII = [1, 4, 16]
F = np.float32
same = util.same_bits_or_nan


def cam_floats(cam):
    """pos, rot (column-major: rot[3 j + k] = column j's k), fov_y: the 13 floats the header's frame is made from."""
    return np.concatenate([cam.pos, cam.rot.reshape(-1), [cam.fov_y]]).astype(F)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dof") / "libdof.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "dof_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.dof_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dof_gather.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.dof_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.dof_table.argtypes = [C.c_void_p]
    L.dof_params_ok.argtypes = [C.c_void_p]
    L.dof_defaults.argtypes = [C.c_void_p]
    L.dof_layout.argtypes = [C.c_void_p]

    class Host:
        @staticmethod
        def prepare(sums, total, rec, cam, focus_distance, aperture, max_radius):
            sums, rec, c = np.ascontiguousarray(sums, F), np.ascontiguousarray(rec, F), cam_floats(cam)
            h, w = sums.shape[:2]
            p = state.DofParams(focus_distance, aperture, max_radius, 0)
            out = np.full((h, w, 4), 7, F)
            L.dof_prepare(sums.ctypes.data, rec.ctypes.data, h, w, total, c.ctypes.data, C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def gather(prep, max_radius):
            prep = np.ascontiguousarray(prep, F)
            h, w = prep.shape[:2]
            out = np.full((h, w, 4), 7, F)
            L.dof_gather(prep.ctypes.data, h, w, max_radius, out.ctypes.data)
            return out

        @staticmethod
        def dof(sums, total, rec, cam, focus_distance, aperture, max_radius):
            p = Host.prepare(sums, total, rec, cam, focus_distance, aperture, max_radius)
            return Host.gather(p, max_radius), p[..., 3]

        @staticmethod
        def depth(rec, cam):
            rec, c = np.ascontiguousarray(rec, F), cam_floats(cam)
            out = np.full(rec.shape[:2], 7, F)
            L.dof_depth(rec.ctypes.data, rec.shape[0], rec.shape[1], c.ctypes.data, out.ctypes.data)
            return out

        @staticmethod
        def ok(focus_distance=1.0, aperture=0.01, max_radius=8, flags=0):
            p = state.DofParams(focus_distance, aperture, max_radius, flags)
            return bool(L.dof_params_ok(C.byref(p)))
    Host.L = L
    return Host


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("radius", RADII)
def test_header_arithmetic_matches_numpy_bit_for_bit(host, h, w, radius):
    focus = 2.0
    sums, rec, cam, special = dof_ref.synthetic(h, w, seed=1000 * h + w, focus_distance=focus)
    assert bool(special) == (h * w >= 16)
    assert same(host.depth(rec, cam), dof_ref.depth(rec, cam))
    for total, aperture in ((1, 0.05), (3, 0.4), (3, 0.0)):
        case = (total, aperture)
        prep = host.prepare(sums, total, rec, cam, focus, aperture, radius)
        want_prep = dof_ref.prepare(sums, total, rec, cam, focus, aperture, radius)
        assert same(prep, want_prep), case
        r = prep[..., 3]
        assert np.isfinite(r).all() and (np.abs(r) <= radius).all(), case
        got = host.gather(prep, radius)
        assert same(got, dof_ref.gather(want_prep, radius)) and (got[..., 3] == 1).all(), case
        if aperture == 0.0:  # (a) the source's colour bits, special pixels included
            assert same(got[..., :3], want_prep[..., :3]) and not r.any()
    if h * w >= 16:  # the layout has both fields and the clamp (the pixel of depth 0)
        r = dof_ref.coc(rec, cam, focus, 0.4, radius)
        assert (r < 0).any() and (r > 0).any() and (r == -radius).any()


def test_the_distance_table_is_the_rounded_square_root(host):
    got = np.zeros((33, 33), F)
    host.L.dof_table(got.ctypes.data)
    d = np.arange(-16, 17)
    want = np.sqrt((d[:, None] ** 2 + d[None, :] ** 2).astype(F))
    assert want.dtype == F and same(got, want) and same(got, dof_ref.dist_table())
    # correctly rounded: the nearest f32 to the float64 root (which is within half a float64 ulp of the true one)
    assert np.array_equal(got, np.sqrt((d[:, None] ** 2 + d[None, :] ** 2).astype(np.float64)).astype(F))
    assert got[16, 16] == 0 and got[16, 19] == 3 and got[12, 19] == 5 and got[0, 0] == F(np.sqrt(512.0))
    # the committed header is what the generator prints
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "tools", "gen_dof_table.py")], stdout=subprocess.PIPE, text=True, check=True)
    assert r.stdout == open(os.path.join(util.ROOT, "include", "rsrt_dof_table.h")).read()


def flat_frame(h, w, seed, z, cam=None, hits=1):
    """Random positive colours (total 1) over records at depth z [h, w]."""
    rng = np.random.default_rng(seed)
    cam = cam or dof_ref.default_camera()
    sums = np.ones((h, w, 4), F)
    sums[..., :3] = np.exp(rng.normal(-1.0, 1.0, (h, w, 3))).astype(F)
    return sums, dof_ref.records_at_depth(np.broadcast_to(F(z), (h, w)) if np.isscalar(z) else z, cam, hits), cam


def test_everything_on_the_focus_plane_is_the_identity(host):
    """(b) records at the focus depth along the AXIS: the corners of the frame are farther from the eye than the centre, and still sharp."""
    h, w, focus = 24, 40, 3.0
    sums, _, cam, _ = dof_ref.synthetic(h, w, seed=11)
    rec = dof_ref.records_at_depth(np.full((h, w), focus, F), cam, hits=3)
    dist = rec[..., 7] / rec[..., 3]
    assert dist[0, 0] > 1.05 * dist[h // 2, w // 2]  # a plane, not a sphere
    for radius in RADII:
        got, r = host.dof(sums, 3, rec, cam, focus, 0.5, radius)
        assert np.abs(r).max() < 1e-4  # (the cosine does not divide exactly everywhere)
        assert same(got[..., :3], (sums[..., :3] / F(3)).astype(F))
        want, _ = dof_ref.dof(sums, 3, rec, cam, focus, 0.5, radius)
        assert same(got, want)
    # the same records read as distances from the eye (a sphere) would blur the corner: the cosine is what keeps it sharp
    assert 0.5 * h * (1 - focus / dist[0, 0]) > 0.5


def test_an_in_focus_foreground_keeps_its_pixels_over_a_far_background(host):
    """(c)"""
    h, w, focus, radius = 32, 40, 2.0, 8
    z = np.full((h, w), 50.0, F)
    z[10:22, 12:28] = focus
    sums, rec, cam = flat_frame(h, w, 5, z)
    got, r = host.dof(sums, 1, rec, cam, focus, 0.3, radius)
    fg = np.zeros((h, w), bool)
    fg[10:22, 12:28] = True
    assert (r[~fg] == radius).all() and np.abs(r[fg]).max() < 1e-4
    assert same(got[fg][:, :3], sums[fg][:, :3])
    changed = (util.bits(got[..., :3]) != util.bits(sums[..., :3])).any(axis=-1)
    assert changed[~fg].all() and not changed[fg].any()
    assert same(got, dof_ref.dof(sums, 1, rec, cam, focus, 0.3, radius)[0])


def test_a_near_field_block_spreads_over_an_in_focus_background(host):
    """(d) background pixels within R of the block change, pixels farther than R + 1 from it do not."""
    h, w, focus, radius = 40, 48, 4.0, 6
    z = np.full((h, w), focus, F)
    z[16:24, 20:28] = 0.04
    sums, rec, cam = flat_frame(h, w, 6, z)
    sums[..., :3] = 1.0
    sums[16:24, 20:28, :3] = (5.0, 3.0, 2.0)
    got, r = host.dof(sums, 1, rec, cam, focus, 0.3, radius)
    near = np.zeros((h, w), bool)
    near[16:24, 20:28] = True
    assert (r[near] == -radius).all() and np.abs(r[~near]).max() < 1e-4
    yy, xx = np.mgrid[0:h, 0:w]
    ny, nx = np.nonzero(near)
    dist = np.sqrt(((yy[..., None] - ny) ** 2 + (xx[..., None] - nx) ** 2).min(axis=-1))
    changed = (util.bits(got[..., :3]) != util.bits(sums[..., :3])).any(axis=-1)
    assert changed[~near & (dist <= radius)].all()
    assert not changed[dist > radius + 1].any() and (dist > radius + 1).sum() > 100
    assert same(got, dof_ref.dof(sums, 1, rec, cam, focus, 0.3, radius)[0])


def test_one_bright_pixel_keeps_its_energy_and_its_support(host):
    """(e) uniform r = 6 (sky everywhere: r = aperture * h = 0.1875 * 32), one bright pixel more than R from every border.  Every interior
    pixel has the same acc.w, so the outputs sum to the pixel's value up to the rounding of at most 1089 sequential f32 adds a pixel:
    n * eps = 1089 * 2^-24 = 6.5e-5 < 1e-4 relative.  Beyond r + 0.5 the weight is exactly 0."""
    h, w, radius = 32, 44, 8
    cam = dof_ref.default_camera()
    rec = dof_ref.records_at_depth(np.full((h, w), np.inf, F), cam)
    sums = np.zeros((h, w, 4), F)
    sums[..., 3] = 1
    value = np.array([700.0, 3.25, 0.001], F)
    sums[15, 21, :3] = value
    got, r = host.dof(sums, 1, rec, cam, 1.0, 0.1875, radius)
    assert (r == 6).all()
    assert same(got, dof_ref.dof(sums, 1, rec, cam, 1.0, 0.1875, radius)[0])
    total = got[..., :3].astype(np.float64).sum(axis=(0, 1))
    print("energy: relative errors", np.abs(total / value.astype(np.float64) - 1))
    assert (np.abs(total / value.astype(np.float64) - 1) <= 1e-4).all()
    yy, xx = np.mgrid[0:h, 0:w]
    dist = np.sqrt((yy - 15.0) ** 2 + (xx - 21.0) ** 2)
    assert not got[dist > 6.5][:, :3].any() and (got[dist < 6.0][:, 0] > 0).all()


def test_the_taps_are_summed_in_the_published_order(host):
    """(f) colours spanning many binades under a uniform blur: summing the same taps in the reverse order (the frame flipped both ways
    and the result flipped back: the geometry and the distance table are symmetric) rounds differently.  The header takes the published
    order; one value's bits are pinned."""
    h, w, radius = 21, 21, 4
    rng = np.random.default_rng(2024)
    cam = dof_ref.default_camera()
    rec = dof_ref.records_at_depth(np.full((h, w), np.inf, F), cam)
    sums = np.ones((h, w, 4), F)
    sums[..., :3] = (rng.integers(1, 1 << 20, (h, w, 3)).astype(F) * F(2.0) ** rng.integers(-24, 4, (h, w, 3)).astype(F)).astype(F)  # (exact)
    prep = dof_ref.prepare(sums, 1, rec, cam, 1.0, 4.0 / h, radius)
    assert (prep[..., 3] == prep[0, 0, 3]).all() and 3.9 < prep[0, 0, 3] <= 4.0
    want = dof_ref.gather(prep, radius)
    reverse = dof_ref.gather(prep[::-1, ::-1], radius)[::-1, ::-1]
    assert not same(want, reverse) and np.allclose(want, reverse, rtol=1e-5)
    y, x = [(int(a), int(b)) for a, b in zip(*np.nonzero((util.bits(want) != util.bits(reverse)).any(axis=-1))) if 4 <= a < h - 4 and 4 <= b < w - 4][0]
    got = host.gather(prep, radius)
    assert same(got, want)
    assert util.bits(got[y, x]).tolist() == util.bits(want[y, x]).tolist() != util.bits(reverse[y, x]).tolist()
    assert (y, x, util.bits(got[y, x]).tolist()) == PINNED, (y, x, [hex(v) for v in util.bits(got[y, x])])


PINNED = (4, 4, [0x489bb4e5, 0x481d97f9, 0x48c2caf9, 0x3f800000])  # (y, x, the four words of the lens image there, from dof_ref)


def test_params_ok_accepts_and_rejects(host):
    good = [{}, {"max_radius": 1}, {"max_radius": 16}, {"aperture": 0.0}, {"aperture": -0.0}, {"aperture": 10.0}, {"focus_distance": 1e-30}, {"focus_distance": 3e38}]
    bad = [{"max_radius": 0}, {"max_radius": 17}, {"max_radius": 0xffffffff}, {"flags": 1}, {"flags": 0x80000000}]
    bad += [{"focus_distance": v} for v in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf"))]
    bad += [{"aperture": v} for v in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf"))]
    for kw in good:
        assert host.ok(**kw) and dof_ref.params_ok(**dict(dof_ref.DEFAULTS, **kw)), kw
    for kw in bad:
        assert not host.ok(**kw) and not dof_ref.params_ok(**dict(dof_ref.DEFAULTS, **kw)), kw


def test_struct_layout_and_defaults(host):
    lay = np.zeros(7, np.uint32)
    host.L.dof_layout(lay.ctypes.data)
    P = state.DofParams
    assert list(lay) == [C.sizeof(P), P.aperture.offset, P.max_radius.offset, P.flags.offset, state.DOF_MAX_RADIUS, state.IMAGE_SOURCES["lens"], 33]
    assert C.sizeof(P) == 16 and [f[0] for f in P._fields_] == ["focus_distance", "aperture", "max_radius", "flags"]
    d = P()
    host.L.dof_defaults(C.byref(d))
    got = {"focus_distance": d.focus_distance, "aperture": d.aperture, "max_radius": d.max_radius, "flags": d.flags}
    want = {k: (v if isinstance(v, int) else float(F(v))) for k, v in dof_ref.DEFAULTS.items()}
    assert got == want and {k: (v if isinstance(v, int) else float(F(v))) for k, v in state.DOF_DEFAULTS.items()} == want
    assert dof_ref.MAX_RADIUS == state.DOF_MAX_RADIUS == 16
    assert state.IMAGE_SOURCES == dict(state.EXPOSURE_SOURCES, lens=4) and "lens" not in state.EXPOSURE_SOURCES
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_EXPOSURE_LENS = 4" in hdr
    import inspect
    sig = inspect.signature(R.State.depth_of_field).parameters
    assert [sig[k].default for k in ("source", "focus_distance", "aperture", "max_radius", "sample_total", "stream")] == ["mean", None, None, None, None, None]
    assert inspect.signature(R.State.focus_at).parameters["source"].default == "mean"


def test_library_exports_depth_of_field():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_dof", "rsrt_dof_download", "rsrt_dof_coc_download", "rsrt_dof_depth_at", "rsrt_dof_reset"):
        assert hasattr(lib, n), n
    for m in ("depth_of_field", "dof_download", "dof_coc", "focus_at", "dof_reset"):
        assert hasattr(R.State, m), m


KERNELS = ("rt_dof_prepare_kernel", "rt_dof_gather_kernel")


def test_dof_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def tile_constants():
    """RT_DOF_TW, RT_DOF_TH of the gather kernel, from the source's #defines."""
    import re
    src = open(os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip", "rt_dof.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)\b" % n, src).group(1)) for n in ("RT_DOF_TW", "RT_DOF_TH"))


def test_tile_constants_are_readable():
    tw, th = tile_constants()
    assert tw >= 1 and th >= 1 and tw * th == 256
    assert (tw + 32) * (th + 32) * 20 + 4 <= 64 * 1024  # the LDS a workgroup asks for at radius 16


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "dof_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "dof_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_depth_of_field_compiles(tmp_path):
    build_cpp_demo(tmp_path)
