"""Camera motion blur without a GPU: its published arithmetic (include/rsrt_motion.h), compiled for the CPU, against the numpy restatement
the GPU tests hold the kernels to (tests/motion_ref.py), bit for bit, special pixels included; the identities; how the sky and near and
far surfaces move; the occlusion rule; the ties of both maxima; the tap order; the parameter check; the ABI and the kernels' code
objects."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

FRAMES = [(1, 1), (3, 5), (17, 33), (40, 56)]  # (h, w): one pixel, less than a tile, 2 x 3 clipped tiles, 3 x 4 tiles
RADII = [1, 4, 16]
TAPS = [2, 16]
F = np.float32
same = util.same_bits_or_nan


def cam_floats(cam):
    """pos, rot (column-major: rot[3 j + k] = column j's k), fov_y: the 13 floats the header's frame is made from."""
    return np.concatenate([cam.pos, cam.rot.reshape(-1), [cam.fov_y]]).astype(F)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("motion") / "libmotion.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "motion_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.motion_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.motion_tile_max.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.motion_neighbour_max.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.motion_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.motion_params_ok.argtypes = [C.c_void_p]
    L.motion_defaults.argtypes = [C.c_void_p]
    L.motion_layout.argtypes = [C.c_void_p]

    class Host:
        @staticmethod
        def prepare(sums, total, rec, cam, prev, shutter, max_radius):
            sums, rec, c, q = np.ascontiguousarray(sums, F), np.ascontiguousarray(rec, F), cam_floats(cam), cam_floats(prev)
            h, w = sums.shape[:2]
            p = state.MotionParams(shutter, max_radius, 16, 0)
            out = np.full((h, w, 7), 7, F)
            L.motion_prepare(sums.ctypes.data, rec.ctypes.data, h, w, total, c.ctypes.data, q.ctypes.data, C.byref(p), out.ctypes.data)
            return out

        @staticmethod
        def tile_max(prep):
            prep = np.ascontiguousarray(prep, F)
            h, w = prep.shape[:2]
            out = np.full((motion_ref.tiles_of(h), motion_ref.tiles_of(w), 3), 7, F)
            L.motion_tile_max(prep.ctypes.data, h, w, out.ctypes.data)
            return out

        @staticmethod
        def neighbour_max(tiles):
            tiles = np.ascontiguousarray(tiles, F)
            out = np.full(tiles.shape, 7, F)
            L.motion_neighbour_max(tiles.ctypes.data, tiles.shape[0], tiles.shape[1], out.ctypes.data)
            return out

        @staticmethod
        def gather(prep, tiles, taps):
            prep, tiles = np.ascontiguousarray(prep, F), np.ascontiguousarray(tiles, F)
            h, w = prep.shape[:2]
            out = np.full((h, w, 4), 7, F)
            L.motion_gather(prep.ctypes.data, tiles.ctypes.data, h, w, taps, out.ctypes.data)
            return out

        @staticmethod
        def motion(sums, total, rec, cam, prev, shutter, max_radius, taps):
            p = Host.prepare(sums, total, rec, cam, prev, shutter, max_radius)
            t = Host.tile_max(p)
            return Host.gather(p, t, taps), np.concatenate([p[..., 5:7], p[..., 3:4]], axis=-1), t

        @staticmethod
        def ok(shutter=0.5, max_radius=16, taps=16, flags=0):
            p = state.MotionParams(shutter, max_radius, taps, flags)
            return bool(L.motion_params_ok(C.byref(p)))
    Host.L = L
    return Host


@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("taps", TAPS)
def test_header_arithmetic_matches_numpy_bit_for_bit(host, h, w, radius, taps):
    sums, rec, cam, prev, placed = motion_ref.synthetic(h, w, seed=1000 * h + w)
    assert bool(placed) == (h * w >= 16)
    for total, shutter in ((1, 0.5), (3, 1.0), (3, 0.0)):
        case = (total, shutter)
        prep = host.prepare(sums, total, rec, cam, prev, shutter, radius)
        want_prep = motion_ref.prepare(sums, total, rec, cam, prev, shutter, radius)
        assert same(prep, want_prep), case
        l = prep[..., 3]
        assert np.isfinite(l).all() and (l >= 0).all() and (l <= radius).all() and not np.isnan(prep[..., 4]).any(), case
        tiles = host.tile_max(prep)
        want_tiles = motion_ref.tile_max(want_prep)
        assert same(tiles, want_tiles), case
        near = host.neighbour_max(tiles)
        want_near = motion_ref.neighbour_max(want_tiles)
        assert same(near, want_near), case
        got = host.gather(prep, tiles, taps)
        assert same(got, motion_ref.gather(want_prep, taps, want_near)) and (got[..., 3] == 1).all(), case
        copied = np.repeat(np.repeat(want_near[..., 2] < 0.5, 16, axis=0), 16, axis=1)[:h, :w]
        assert same(got[copied][:, :3], want_prep[copied][:, :3])  # a tile under half a pixel: the source's colour bits
        if shutter == 0.0:
            assert same(got[..., :3], want_prep[..., :3]) and not l.any() and not tiles.any()
        elif placed:  # the frame really holds every listed case
            has = motion_ref.contains(sums, rec, cam, prev, placed, shutter, radius)
            assert all(has.values()), has
        if (h, w) == (40, 56) and shutter == 0.5:  # both paths of the gather
            assert (want_near[..., 2] < 0.5).any() and (want_near[..., 2] >= 0.5).any()
            assert (util.bits(got[~copied][:, :3]) != util.bits(want_prep[~copied][:, :3])).any()


def flat_frame(h, w, seed, dist, hits=1):
    """Random positive colours (total 1) over records at ray distance dist."""
    rng = np.random.default_rng(seed)
    sums = np.ones((h, w, 4), F)
    sums[..., :3] = np.exp(rng.normal(-1.0, 1.0, (h, w, 3))).astype(F)
    return sums, motion_ref.records_at_distance(np.broadcast_to(F(dist), (h, w)) if np.isscalar(dist) else dist, hits)


def test_the_same_camera_or_a_closed_shutter_is_the_identity(host):
    h, w = 24, 40
    sums, rec, cam, prev, placed = motion_ref.synthetic(h, w, seed=11)
    colour = (sums[..., :3] / F(3)).astype(F)
    assert np.isinf(colour).any() and np.isnan(colour).any()
    twin = motion_ref.Camera(cam.pos.copy(), cam.rot.copy(), cam.fov_y)
    for other, shutter in ((twin, 1.0), (prev, 0.0), (twin, 0.0)):
        for radius in RADII:
            got, uvl, tiles = host.motion(sums, 3, rec, cam, other, shutter, radius, 16)
            assert same(got[..., :3], colour) and (got[..., 3] == 1).all()
            assert not uvl.any() and not tiles.any()
            want, want_uvl, want_tiles = motion_ref.motion(sums, 3, rec, cam, other, shutter, radius, 16)
            assert same(got, want) and same(uvl, want_uvl) and same(tiles, want_tiles)
    # a camera that differs in one bit is another camera: the velocity is not exactly 0 everywhere
    moved = motion_ref.Camera(cam.pos.copy(), cam.rot.copy(), cam.fov_y)
    moved.pos[0] = np.nextafter(moved.pos[0], F(10))
    assert not cam.same(moved) and cam.same(twin)


def test_the_sky_follows_the_rotation_only(host):
    """Under a pure translation the sky does not move; under a pure yaw by a small angle theta the centre pixel moves by
    hs W tan(theta) / (2 m aspect) pixels, m = sin(fov / 2) (the projection's own scale), away from where it was."""
    h, w = 36, 64
    cam = motion_ref.Camera([0.5, 1.0, -2.0], np.eye(3, dtype=F), 0.9)
    sums, rec = flat_frame(h, w, 3, np.inf)
    _, uvl, _ = host.motion(sums, 1, rec, cam, motion_ref.earlier(cam, 0.0, 0.7, -0.4), 1.0, 16, 16)
    print("sky under a translation: max |u| %.3g px" % np.abs(uvl[..., :2]).max())
    assert np.abs(uvl[..., :2]).max() < 0.01
    theta, shutter = 0.01, 1.0
    prev = motion_ref.earlier(cam, theta)
    _, uvl, _ = host.motion(sums, 1, rec, cam, prev, shutter, 16, 16)
    want_uvl = motion_ref.motion(sums, 1, rec, cam, prev, shutter, 16, 16)[1]
    assert same(uvl, want_uvl)
    y, x = h // 2, w // 2
    expect = 0.5 * shutter * w * np.tan(theta) / (2.0 * float(cam.m) * (w / h))
    fx, _, _ = motion_ref.temporal_ref.project(prev, w, h, motion_ref.temporal_ref.center_ray(cam, w, h, np.array(x), np.array(y)))
    ux = float(uvl[y, x, 0])
    print("yaw %.3g: ux %.6g, expected %.6g" % (theta, abs(ux), expect))
    assert abs(abs(ux) / expect - 1.0) < 0.01 and np.sign(ux) == np.sign(x - float(fx)) and abs(float(uvl[y, x, 1])) < 0.01 * expect


def test_near_surfaces_move_faster_than_far_ones(host):
    h, w = 32, 48
    cam = motion_ref.Camera([0.0, 0.0, 0.0], np.eye(3, dtype=F), 0.9)
    dist = np.full((h, w), 20.0, F)
    dist[:, w // 2:] = 2.0
    sums, rec = flat_frame(h, w, 4, dist)
    _, uvl, _ = host.motion(sums, 1, rec, cam, motion_ref.earlier(cam, 0.0, 0.0, 0.1), 0.5, 16, 16)
    far, near = uvl[:, :w // 2, 2], uvl[:, w // 2:, 2]
    assert far.max() < near.min() and far.min() > 0 and near.max() < 16
    assert 8 < near.mean() / far.mean() < 12  # the parallax goes as 1 / depth: ten times


def test_a_static_foreground_keeps_its_colour_over_a_fast_background(host):
    """A near pixel that does not move (l = 0) among far pixels that move at the clamp: every tap is behind it (f = 0), so a tap counts
    only through the pixel's own half-pixel cone, which no tap of a long line lies in.  The yardstick is the restated value; with these
    inputs that is the pixel's colour to within the rounding of acc / N + (1 - 0) c: here exactly."""
    h, w, radius, taps = 33, 49, 8, 16
    rng = np.random.default_rng(8)
    prep = np.zeros((h, w, 7), F)
    prep[..., :3] = np.exp(rng.normal(-1.0, 1.0, (h, w, 3))).astype(F)
    prep[..., 3], prep[..., 4], prep[..., 5] = radius, 50.0, radius  # the background: far, moving along x at the clamp
    fy, fx = 16, 24
    prep[fy, fx, 3:] = (0.0, 1.0, 0.0, 0.0)                          # the foreground pixel: near and still
    tiles = host.tile_max(prep)
    assert (tiles[..., 2] == radius).all()
    got = host.gather(prep, tiles, taps)
    want = motion_ref.gather(prep, taps)
    assert same(got, want)
    assert same(got[fy, fx, :3], prep[fy, fx, :3])
    assert (util.bits(got[fy, fx + 3, :3]) != util.bits(prep[fy, fx + 3, :3])).any()  # the background beside it is blurred ...
    # ... and the foreground pixel spreads over the background no farther than its own half pixel: it weighs nothing in its neighbours
    without = prep.copy()
    without[fy, fx, :3] = 1e6
    assert same(motion_ref.gather(without, taps)[fy, fx + 3], want[fy, fx + 3])


def test_ties_in_both_maxima_go_to_the_first_in_row_major_order(host):
    h, w = 40, 56
    prep = np.zeros((h, w, 7), F)
    prep[..., 4] = 5.0
    # tile (0, 0): three texels of the same greatest length, in different directions; the first in row-major order is (2, 9)
    for (y, x), (ux, uy) in {(5, 3): (0.0, 3.0), (2, 9): (3.0, 0.0), (2, 12): (-3.0, 0.0)}.items():
        prep[y, x, 3], prep[y, x, 5], prep[y, x, 6] = 3.0, ux, uy
    prep[3, 3, 3], prep[3, 3, 5] = 2.0, 2.0
    # tiles (0, 3) and (2, 2): the same length again
    prep[1, 50, 3], prep[1, 50, 6] = 3.0, -3.0
    prep[35, 40, 3], prep[35, 40, 5], prep[35, 40, 6] = 3.0, F(3.0 * 0.6), F(3.0 * 0.8)
    tiles = host.tile_max(prep)
    assert same(tiles, motion_ref.tile_max(prep))
    assert tiles[0, 0].tolist() == [3.0, 0.0, 3.0] and tiles[0, 3].tolist() == [0.0, -3.0, 3.0] and not tiles[1].any() and not tiles[0, 1].any()
    near = host.neighbour_max(tiles)
    assert same(near, motion_ref.neighbour_max(tiles))
    assert near[1, 1].tolist() == [3.0, 0.0, 3.0]            # (0, 0) comes before (2, 2)
    assert near[1, 2].tolist() == [0.0, -3.0, 3.0]           # (0, 3) comes before (2, 2)
    assert near[2, 1].tolist() == tiles[2, 2].tolist() and near[1, 3].tolist() == [0.0, -3.0, 3.0] and near[0, 1].tolist() == [3.0, 0.0, 3.0]
    # all nine equal: the first tile's record, whatever the others' directions
    tiles9 = np.zeros((3, 3, 3), F)
    tiles9[..., 2] = 2.0
    tiles9[..., 0] = np.arange(9, dtype=F).reshape(3, 3)
    assert host.neighbour_max(tiles9)[1, 1].tolist() == [0.0, 0.0, 2.0] and host.neighbour_max(tiles9)[2, 2].tolist() == [4.0, 0.0, 2.0]


def test_the_taps_are_summed_in_the_published_order(host):
    """Colours spanning many binades under a uniform velocity: summing the same taps in the reverse order rounds differently.  The
    header takes the published order; one value's bits are pinned."""
    h, w, radius, taps = 21, 37, 6, 16
    rng = np.random.default_rng(2024)
    prep = np.zeros((h, w, 7), F)
    prep[..., :3] = (rng.integers(1, 1 << 20, (h, w, 3)).astype(F) * F(2.0) ** rng.integers(-24, 4, (h, w, 3)).astype(F)).astype(F)  # (exact)
    prep[..., 3], prep[..., 4], prep[..., 5] = radius, 7.0, radius
    want = motion_ref.gather(prep, taps)
    reverse = motion_ref.gather(prep, taps, order=range(taps - 1, -1, -1))
    assert not same(want, reverse) and np.allclose(want, reverse, rtol=1e-5)
    y, x = [(int(a), int(b)) for a, b in zip(*np.nonzero((util.bits(want) != util.bits(reverse)).any(axis=-1))) if radius <= b < w - radius][0]
    got = host.gather(prep, host.tile_max(prep), taps)
    assert same(got, want)
    assert util.bits(got[y, x]).tolist() == util.bits(want[y, x]).tolist() != util.bits(reverse[y, x]).tolist()
    assert (y, x, util.bits(got[y, x]).tolist()) == PINNED, (y, x, [hex(v) for v in util.bits(got[y, x])])


PINNED = (0, 6, [0x48d56cde, 0x473945ff, 0x478e094c, 0x3f800000])  # (y, x, the four words of the motion image there, from motion_ref)


def test_params_ok_accepts_and_rejects(host):
    good = [{}, {"max_radius": 1}, {"max_radius": 16}, {"shutter": 0.0}, {"shutter": -0.0}, {"shutter": 1.0}, {"shutter": 1e-30}, {"taps": 2}, {"taps": 32}]
    bad = [{"max_radius": 0}, {"max_radius": 17}, {"max_radius": 0xffffffff}, {"flags": 1}, {"flags": 0x80000000}]
    bad += [{"shutter": v} for v in (-1e-30, -1.0, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf"))]
    bad += [{"taps": v} for v in (0, 1, 3, 15, 33, 34, 0xfffffffe)]
    for kw in good:
        assert host.ok(**kw) and motion_ref.params_ok(**dict(motion_ref.DEFAULTS, **kw)), kw
    for kw in bad:
        assert not host.ok(**kw) and not motion_ref.params_ok(**dict(motion_ref.DEFAULTS, **kw)), kw


def test_struct_layout_and_defaults(host):
    lay = np.zeros(8, np.uint32)
    host.L.motion_layout(lay.ctypes.data)
    P = state.MotionParams
    assert list(lay) == [C.sizeof(P), P.max_radius.offset, P.taps.offset, P.flags.offset, state.MOTION_MAX_RADIUS, state.MOTION_TILE,
                         state.DISPLAY_SOURCES["motion"], motion_ref.MAX_TAPS]
    assert C.sizeof(P) == 16 and [f[0] for f in P._fields_] == ["shutter", "max_radius", "taps", "flags"]
    d = P()
    host.L.motion_defaults(C.byref(d))
    got = {"shutter": d.shutter, "max_radius": d.max_radius, "taps": d.taps, "flags": d.flags}
    want = {k: (v if isinstance(v, int) else float(F(v))) for k, v in motion_ref.DEFAULTS.items()}
    assert got == want and {k: (v if isinstance(v, int) else float(F(v))) for k, v in state.MOTION_DEFAULTS.items()} == want
    assert motion_ref.MAX_RADIUS == motion_ref.TILE == state.MOTION_MAX_RADIUS == state.MOTION_TILE == 16
    assert state.DISPLAY_SOURCES == dict(state.IMAGE_SOURCES, motion=5)
    assert state.IMAGE_SOURCES == dict(state.EXPOSURE_SOURCES, lens=4) and "motion" not in state.IMAGE_SOURCES
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    assert "RSRT_EXPOSURE_MOTION = 5" in hdr
    import inspect
    sig = inspect.signature(R.State.motion_blur).parameters
    names = ("source", "previous", "shutter", "max_radius", "taps", "sample_total", "out_ptr", "stream")
    assert [k for k in sig if k != "self"] == list(names) and [sig[k].default for k in names] == ["mean"] + [None] * 7


def test_library_exports_camera_motion_blur():
    lib = C.CDLL(_build.build_hip())
    for n in ("rsrt_motion_blur", "rsrt_motion_download", "rsrt_motion_velocity_download", "rsrt_motion_tiles_download", "rsrt_motion_reset"):
        assert hasattr(lib, n), n
    for m in ("motion_blur", "motion_download", "motion_velocity", "motion_tiles", "motion_reset"):
        assert hasattr(R.State, m), m


KERNELS = ("rt_motion_prepare_kernel", "rt_motion_gather_kernel")


def test_motion_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (kernel, k)


def tile_constants():
    """RT_MOTION_TILE, RT_MOTION_MAX_HALO of the gather kernel, from the source's #defines."""
    src = open(os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip", "rt_motion.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)\b" % n, src).group(1)) for n in ("RT_MOTION_TILE", "RT_MOTION_MAX_HALO"))


def test_the_gathers_lds_at_radius_16_fits():
    tile, halo = tile_constants()
    assert tile == motion_ref.TILE and halo == motion_ref.MAX_RADIUS == 16
    assert (tile + 2 * halo) ** 2 * 20 <= 64 * 1024  # the LDS a workgroup asks for at radius 16: a float4 and a float a staged texel


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "motion_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "motion_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_motion_blur_compiles(tmp_path):
    build_cpp_demo(tmp_path)
