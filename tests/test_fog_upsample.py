"""The fog rebuild without a GPU: its published arithmetic (include/rsrt_fog_upsample.h), compiled for the CPU, against the numpy
restatement the GPU tests hold the kernels to (tests/fog_upsample_ref.py), bit for bit, edge inputs included; a derivable accuracy
check across a depth edge, which the plain tent upsample of the records misses; a clear medium; the ABI; the kernels' code objects."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import fog_ref
import fog_upsample_ref as ref
import upsample_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

F = np.float32
same = util.same_bits_or_nan
LIGHT = fog_ref.unit((0.4, 0.6, -0.7))
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "fog_upsample_host.cpp")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def equal(a, b):
    return a.shape == b.shape and np.array_equal(util.bits(a), util.bits(b))


def compile_host(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", out] + list(flags)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fogup") / "libfogup.so")
    compile_host(so, "-fPIC", "-shared")
    L = C.CDLL(so)
    V, Z, U, Fl = C.c_void_p, C.c_size_t, C.c_uint32, C.c_float
    L.fogup_source.argtypes = [V, Fl, Z, V]
    L.fogup_tau.argtypes = [V, V, Fl, Z, V]
    L.fogup_axis.argtypes = [U, U, V, V, V]
    L.fogup_taps.argtypes = [V, V, Z, V]
    L.fogup_finish.argtypes = [V, V, V, Z, V]
    L.fogup_rebuild.argtypes = [V, V, Fl, U, U, V, Fl, V, U, U, V]
    L.fogup_source_max_bits.restype = U
    return L


def param_set(**kw):
    return fog_ref.params(**dict({"light_dir": LIGHT}, **kw))


def c_params(p):
    return state.FogParams.of(**p)


def host_source(host, rec, n):
    rec = np.ascontiguousarray(rec, F).reshape(-1, 4)
    out = np.full((len(rec), 3), 7, F)
    host.fogup_source(ptr(rec), float(n), len(rec), ptr(out))
    return out


def host_tau(host, p, g, T):
    g = np.ascontiguousarray(g, F).reshape(-1, 8)
    out = np.full(len(g), 7, F)
    host.fogup_tau(C.byref(c_params(p)), ptr(g), float(T), len(g), ptr(out))
    return out


def host_rebuild(host, p, colour, rec, n, g, T):
    rec, g, colour = np.ascontiguousarray(rec, F), np.ascontiguousarray(g, F), np.ascontiguousarray(colour, F)
    (h, w), (H, W) = rec.shape[:2], g.shape[:2]
    out = np.full((H, W, 4), 7, F)
    host.fogup_rebuild(C.byref(c_params(p)), ptr(rec), float(n), w, h, ptr(g), float(T), ptr(colour), W, H, ptr(out))
    return out


def test_the_standalone_program_runs(tmp_path):
    exe = str(tmp_path / "fogup_main")
    compile_host(exe, "-DFOGUP_HOST_MAIN")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split()[1] == "7b800000", r.stdout  # (2^120)


def test_source_term_matches_numpy_bit_for_bit_at_its_edges(host):
    assert host.fogup_source_max_bits() == int(util.bits(np.array([ref.SOURCE_MAX]))[0]) == 0x7b800000
    rng = np.random.default_rng(5)
    n = 4
    rec = np.empty((2000, 4), F)
    rec[:, 3] = (rng.random(2000) * n).astype(F)
    rec[:, :3] = (rng.random((2000, 3)) * 3).astype(F)
    big = F(3.0e38)
    rec[0] = (1, 2, 3, n)                                   # 1 - Tm == 0: a clear medium, no source term
    rec[1] = (1, 2, 3, F(n) * (F(1) - F(2.0 ** -24)))       # 1 - Tm == 2^-24
    rec[2] = (big, np.inf, 0, F(n) * (F(1) - F(2.0 ** -24)))  # the quotient exceeds the clamp (and is inf)
    rec[3] = (F(1e35), F(1e36), F(1e37), F(n) * F(0.999))   # ... ordinary transmittance, a quotient above 2^120
    rec[4] = (0, 0, 0, 0)                                   # opaque and dark
    rec[5] = (1, 2, 3, np.nextafter(F(n), F(np.inf)))       # (Tm > 1: never written, still no source term)
    rec[6] = (-0.0, 0, 0, 2)
    one = F(1) - rec[:3, 3] / F(n)
    assert one[0] == 0 and one[1] == F(2.0 ** -24)
    got, want = host_source(host, rec, n), ref.source(rec, n)
    assert same(got, want)
    assert not got[0].any() and not got[5].any() and (got[2, :2] == ref.SOURCE_MAX).all() and got[2, 2] == 0 and (got[3] == ref.SOURCE_MAX).all()
    assert same(got[1], (rec[1, :3] / F(n)).astype(F) / F(2.0 ** -24))
    assert np.isfinite(got).all() and (got <= ref.SOURCE_MAX).all()
    for total in (1, 3, 16):
        assert same(host_source(host, rec, total), ref.source(rec, total))
    # nine taps of the clamp stay finite, and times 1 - tau == 0 they are 0
    acc = np.zeros(4, F)
    hs, sq = np.ones(9, F), np.full((9, 3), ref.SOURCE_MAX, F)
    host.fogup_taps(ptr(hs), ptr(sq), 9, ptr(acc))
    assert np.isfinite(acc).all() and acc[3] == 9
    out, colour, one_tau = np.full(3, 7, F), np.array([-0.0, 0.5, 2.0], F), np.ones(1, F)
    host.fogup_finish(ptr(colour), ptr(acc), ptr(one_tau), 1, ptr(out))
    assert equal(out, colour)


@pytest.mark.parametrize("kw", [{"density": 0.15, "max_distance": 20.0}, {"density": 0.0}, {"density": 2.5, "max_distance": 7.0},
                                {"density": 1.0e6, "max_distance": 1.0e30}, {"density": 1.0e-30}])
def test_tau_matches_numpy_bit_for_bit_at_its_edges(host, kw):
    p = param_set(**kw)
    k = fog_ref.prepare(p)
    dist = F(p["max_distance"])
    rng = np.random.default_rng(11)
    for T in (1, 3, 16):
        n = 600
        g = (rng.random((n, 8)) * 5).astype(F)
        hits = rng.integers(0, T + 1, n).astype(F)
        hits[:8] = (0, T, T, T, T, max(T - 1, 0), min(1, T), T)
        d = (rng.random(n) * 1.5 * float(dist)).astype(F)
        d[1:5] = (dist, np.nextafter(dist, F(0)), np.nextafter(dist, F(np.inf)), 0)
        g[:, 3], g[:, 7] = hits, (d * hits).astype(F)
        g[0, 7] = 9  # (a distance sum without hits is not read)
        got, want = host_tau(host, p, g, T), ref.tau(k, g, T)
        assert same(got, want), T
        e_far = fog_ref.transmittance(k, dist)
        assert got[0] == e_far and ((got >= 0) & (got <= 1)).all()
        if T == 1:  # the transmittance rsrt_fog_record adds for the sample the record holds; at and beyond max_distance the far one
            hit = hits > 0
            assert same(got, fog_ref.transmittance(k, fog_ref.segment(k, hit, d)))
            assert got[1] == e_far and got[3] == e_far and (got[2] >= e_far)
        if p["density"] == 0:
            assert (got == 1).all()


@pytest.mark.parametrize("low,out", [(1, 1), (2, 7), (34, 67), (3, 5), (8, 16), (5, 5), (48, 96), (512, 1024)])
def test_axis_coordinates_and_tents(host, low, out):
    u, xn, tent = np.full(out, 7, F), np.full(out, 7, np.int32), np.full((out, 3), 7, F)
    host.fogup_axis(low, out, ptr(u), ptr(xn), ptr(tent))
    wu, wxn = upsample_ref.coords(low, out)
    assert same(u, wu) and np.array_equal(xn, wxn)
    for i, d in enumerate((-1, 0, 1)):
        assert same(tent[:, i], (F(1) - np.abs(((wxn + d).astype(F) - wu).astype(F)) * F(0.5)).astype(F))
    # every tent is 1/4 or more, the nearest pixel lies in 0 .. low and at least one of its taps inside the frame
    assert (tent >= 0.25).all() and (xn >= 0).all() and (xn <= low).all()
    inside = [(xn + d >= 0) & (xn + d < low) for d in (-1, 0, 1)]
    assert (inside[0] | inside[1] | inside[2]).all()
    if low == out:
        assert np.array_equal(xn, np.arange(out)) and (tent == np.array([0.5, 1.0, 0.5], F)).all()


def frame(rng, w, h, W, H, T, n):
    """Random low records of n samples (some clear, some saturated), first-hit records of T samples and a source colour."""
    rec = np.empty((h, w, 4), F)
    rec[..., 3] = (rng.random((h, w)) * n).astype(F)
    rec[..., :3] = (rng.random((h, w, 3)) * 2).astype(F)
    flat = rec.reshape(-1, 4)
    flat[::5] = (0, 0, 0, n)
    flat[::7, 0] = np.inf
    g = (rng.random((H, W, 8)) * 4).astype(F)
    hits = rng.integers(0, T + 1, (H, W)).astype(F)
    g[..., 3], g[..., 7] = hits, (hits * (rng.random((H, W)) * 30).astype(F)).astype(F)
    colour = (rng.random((H, W, 3)) * 3).astype(F)
    colour[0, 0] = (-0.0, 0.0, 1.0)
    return rec, g, colour


@pytest.mark.parametrize("w,h,W,H", [(1, 1, 1, 1), (34, 3, 67, 5), (2, 2, 7, 7), (9, 6, 9, 6), (8, 5, 16, 10), (3, 2, 16, 9), (1, 1, 5, 4)])
@pytest.mark.parametrize("T", [1, 3])
def test_whole_rebuild_matches_numpy_bit_for_bit(host, w, h, W, H, T):
    """Ratios 2, 3.5 (7 from 2), 1 and ragged ones; all four corners and, at ratio 2, X = W - 1, where the nearest low pixel is w."""
    p = param_set(density=0.15, max_distance=20.0)
    n = 2
    rec, g, colour = frame(np.random.default_rng(w * 100 + W), w, h, W, H, T, n)
    got = host_rebuild(host, p, colour, rec, n, g, T)
    want, r = ref.rebuild(colour, rec, n, g, T, fog_ref.prepare(p))
    assert same(got, want) and np.isfinite(got).all() and (got[..., 3] == 1).all()
    if W == 2 * w:
        assert upsample_ref.coords(w, W)[1][-1] == w and upsample_ref.coords(h, H)[1][-1] == h
    # the corners, spelled out tap by tap
    s = ref.source(rec, n)
    u, xn = upsample_ref.coords(w, W)
    v, yn = upsample_ref.coords(h, H)
    for Y in (0, H - 1):
        for X in (0, W - 1):
            acc = np.zeros(4, F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qx, qy = int(xn[X]) + dx, int(yn[Y]) + dy
                    if 0 <= qx < w and 0 <= qy < h:
                        hs = F(F(F(1) - F(abs(F(F(qx) - u[X])) * F(0.5))) * F(F(1) - F(abs(F(F(qy) - v[Y])) * F(0.5))))
                        acc[:3] = (acc[:3] + (hs * s[qy, qx]).astype(F)).astype(F)
                        acc[3] = F(acc[3] + hs)
            assert acc[3] >= F(1 / 16)
            assert same(r[Y, X, :3], ((acc[:3] / acc[3]).astype(F) * F(F(1) - r[Y, X, 3])).astype(F)), (X, Y)


def test_equal_sizes_are_a_tent_and_not_the_identity(host):
    p = param_set(density=0.15, max_distance=20.0)
    rec, g, colour = frame(np.random.default_rng(3), 6, 4, 6, 4, 1, 2)
    rec[..., 3] = (rec[..., 3] * F(0.9)).astype(F)
    got = host_rebuild(host, p, colour, rec, 2, g, 1)
    assert not equal(got, fog_ref.compose(colour, rec, 2))
    flat = np.tile(np.array([0.5, 0.25, 1.0, 1.0], F), (4, 6, 1))  # constant records: the tent changes nothing but rounding
    got = host_rebuild(host, p, colour, flat, 2, g, 1)
    want, r = ref.rebuild(colour, flat, 2, g, 1, fog_ref.prepare(p))
    assert same(got, want) and np.allclose(r[..., :3] / (1 - r[..., 3:4]), np.array([0.5, 0.25, 1.0]), rtol=1e-6)


def test_a_clear_medium_is_the_source_bit_for_bit(host):
    p = param_set(density=0.0, ambient=1.0)
    k = fog_ref.prepare(p)
    rng = np.random.default_rng(9)
    w, h, W, H, T, n = 5, 3, 9, 6, 3, 2
    _, g, colour = frame(rng, w, h, W, H, T, n)
    colour[1, 1] = (-0.0, -0.0, -0.0)
    d = np.tile(np.array([0.6, 0.0, 0.8], F), (w * h, 1))
    rec = np.zeros((w * h, 4), F)
    for _ in range(n):  # records as the fog pass writes them at density 0: (0, 0, 0, 1) a sample
        rec = fog_ref.sample(k, d, np.ones(w * h, bool), np.full(w * h, 5, F), np.full(w * h, 0.5, F), np.ones((w * h, p["steps"]), bool), rec)
    assert not rec[:, :3].any() and (rec[:, 3] == n).all()
    rec = rec.reshape(h, w, 4)
    assert (ref.tau(k, g, T) == 1).all() and not ref.source(rec, n).any()
    got = host_rebuild(host, p, colour, rec, n, g, T)
    assert equal(got[..., :3], colour) and equal(got, ref.rebuild(colour, rec, n, g, T, k)[0])
    assert np.signbit(got[1, 1, :3]).all() and np.signbit(got[0, 0, 0])


def test_the_rebuild_is_exact_in_tau_and_within_the_midpoint_error_across_a_depth_edge(host):
    """A derivable case with no ray: every march point lit, xi = 0.5, one first-hit sample, the same ray direction everywhere.  Output
    16 x 6 from 8 x 3; output columns X < 7 lie at depth L1 = 4, the others at L2 = 16, so the edge (at 6.5) falls inside low pixel 3,
    which covers the output coordinates [5, 7).  The low records hold two samples: both at the pixel's depth, or one at each in column 3.
    The full-size records, one sample a pixel at its depth, are the truth.

    tau is the full-size record's transmittance bit for bit.  The inscatter of a sample is S sum_i T_i delta = (S / sigma)(1 - T)
    (1 - (sigma delta)^2 / 24 + O((sigma delta)^4)), the midpoint rule of DESIGN.md §22, so a low pixel's source term is S / sigma times
    1 - (sigma delta)^2 / 24 of ITS depth (between the two in the mixed column), and the rebuilt inscatter is the full-size one times a
    ratio of two such factors: off by at most (sigma Delta)^2 / 24 a side with Delta = L2 / steps, the longer step.  With sigma Delta = 0.3
    the bound is 7.5e-3 + 2^-20; rsrt_sky_exp2's published 2^-17 and the f32 sums are three orders below the slack the second side leaves.
    The plain tent upsample of the records as they are mixes inscatter of both depths and misses the bound at the edge columns."""
    steps, L1, L2, E = 8, 4.0, 16.0, 7
    p = param_set(density=0.15, max_distance=50.0, steps=steps, flags=0, light_irradiance=(4.0, 3.0, 2.0), ambient=(0.02, 0.03, 0.05), albedo=(0.9, 0.8, 0.7))
    k = fog_ref.prepare(p)
    w, h, W, H = 8, 3, 16, 6
    direction = np.array(fog_ref.unit((0.3, -0.2, 0.9)), F)

    def records(depths):  # depths [N, samples] -> records [N, 4]
        depths = np.asarray(depths, F)
        N = len(depths)
        rec = np.zeros((N, 4), F)
        for s in range(depths.shape[1]):
            rec = fog_ref.sample(k, np.tile(direction, (N, 1)), np.ones(N, bool), depths[:, s], np.full(N, 0.5, F), np.ones((N, steps), bool), rec)
        return rec

    mixed = E // 2
    low_depths = np.array([[L1, L1] if q < mixed else [L1, L2] if q == mixed else [L2, L2] for q in range(w)], F)
    low = np.tile(records(low_depths)[None], (h, 1, 1))
    depth = np.where(np.arange(W) < E, F(L1), F(L2)).astype(F)
    full = np.tile(records(depth[:, None])[None], (H, 1, 1))
    g = np.zeros((H, W, 8), F)
    g[..., 3], g[..., 7] = 1, depth[None, :]
    colour = np.full((H, W, 3), 0.5, F)
    got = host_rebuild(host, p, colour, low, 2, g, 1)
    want, r = ref.rebuild(colour, low, 2, g, 1, k)
    assert same(got, want)
    assert equal(r[..., 3], full[..., 3])  # tau: the full-size record's transmittance
    sigma_delta = float(F(p["density"])) * L2 / steps
    bound = 2 * sigma_delta ** 2 / 24 + 2.0 ** -20
    truth = full[..., :3].astype(np.float64)
    err = np.abs(r[..., :3].astype(np.float64) - truth) / truth
    print("sigma delta %.3f, bound %.3g, largest relative error %.3g (edge columns %.3g)" % (sigma_delta, bound, err.max(), err[:, E - 1:E + 1].max()))
    assert (truth > 0).all() and (err <= bound).all()
    raw = ref.tent_raw(low, 2, H, W)
    raw_err = np.abs(raw[..., :3] - truth) / truth
    print("plain tent: relative error at the edge columns %s" % raw_err[0, E - 1:E + 1].max(axis=-1))
    assert (raw_err[:, E - 1:E + 1] > bound).all()  # without the demodulation the edge columns miss the bound
    assert (raw_err[:, :E - 4] <= bound).all() and (raw_err[:, E + 2:] <= bound).all()  # (where no tap reaches the mixed column it is exact)


FOGUP_SYMBOL = "rsrt_fog_apply_upsampled"


def test_exports_layout_and_names():
    assert FOGUP_SYMBOL in state._SYMBOLS
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    integ = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    assert ("rsrt_status %s(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t fog_sample_total," % FOGUP_SYMBOL) in hdr
    rust = "pub fn %s(ctx: *mut RsrtContext, source: u32, sample_total: u32, fog_sample_total: u32," % FOGUP_SYMBOL
    for text in (hdr, integ):
        assert rust in text and "record_sample_total: u32, params: *const RsrtFogParams, device_out_rgba32f: *mut c_void," in text
    lib = C.CDLL(_build.build_hip())
    assert hasattr(lib, FOGUP_SYMBOL) and hasattr(lib, "rsrt_fog_apply")
    sig = inspect.signature(R.State.fog).parameters
    assert [n for n in sig if n != "self"] == ["source", "out_ptr", "stream", "sample_total", "fog_sample_total", "upsample", "record_sample_total"]
    assert sig["upsample"].default is False and sig["record_sample_total"].default is None
    up = open(os.path.join(util.ROOT, "include", "rsrt_fog_upsample.h")).read()
    assert "fmaf" not in up and "RSRT_FOGUP_SOURCE_MAX" in up
    assert "fog(uint32_t source = RSRT_EXPOSURE_MEAN, bool upsample = false)" in open(os.path.join(util.ROOT, "include", "rsrt_state.hpp")).read()


KERNELS = ("rt_fog_source_kernel", "rt_fog_rebuild_kernel")


def test_rebuild_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (names[0], k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "fog_upsample_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "fog_upsample_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_fog_upsample_compiles(tmp_path):
    build_cpp_demo(tmp_path)
