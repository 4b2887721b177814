"""The JPEG pass on the CPU (include/rsrt_jpeg.h, librsrt_host's rsrt_jpeg_encode_host, rsrt_jpeg_from_coefficients and rsrt_avi_mjpeg_write):
the header evaluated by g++ (tests/cpp/jpeg_host.cpp) and the host library against the numpy restatement (tests/jpeg_ref.py) bit for bit,
step by step and as whole files; crafted coefficient blocks at the entropy coder's edges; the files against an independent decoder and
encoder, Pillow's libjpeg; the Motion-JPEG AVI through a RIFF parser of the test's own; the interfaces; the host code under the
sanitizers as a program of its own; and the kernels' code objects.  No player is on the test machine: the AVI is checked as a chunk tree
whose every frame libjpeg decodes, not by playing it."""
import ctypes as C
import inspect
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as J
import util
import video_ref as V
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import _build, state

F = np.float32
SOURCE = os.path.join(util.ROOT, "tests", "cpp", "jpeg_host.cpp")
SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (5, 67), (64, 96)]  # (w, h)
SUBS = (J.S420, J.S444)
NAMES = {J.S420: "420", J.S444: "444"}
PIL_SUB = {J.S420: 2, J.S444: 0}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jpeg") / "libjpeg_host.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    for name, res, args in (("jpeg_ycc", None, [C.c_void_p, C.c_size_t, C.c_void_p]), ("jpeg_samples", None, [C.c_void_p, C.c_size_t, C.c_void_p]),
                            ("jpeg_fdct", None, [C.c_void_p, C.c_size_t, C.c_void_p]), ("jpeg_quantise", None, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p]),
                            ("jpeg_quantise_block", None, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]), ("jpeg_qtable", None, [C.c_uint32, C.c_uint32, C.c_void_p]),
                            ("jpeg_tables", None, [C.c_void_p] * 4), ("jpeg_block_bits", C.c_uint32, [C.c_void_p, C.c_int, C.c_uint32]),
                            ("jpeg_block_code", C.c_uint32, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]), ("jpeg_block_pred", C.c_int64, [C.c_uint64, C.c_uint32]),
                            ("jpeg_block_component", C.c_uint32, [C.c_uint64, C.c_uint32]), ("jpeg_blocks", C.c_uint64, [C.c_uint32] * 3),
                            ("jpeg_max_bytes", C.c_uint64, [C.c_uint32] * 3), ("jpeg_headers", C.c_uint64, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
                            ("jpeg_stuff", C.c_uint64, [C.c_void_p, C.c_uint64, C.c_void_p]), ("jpeg_params_ok", C.c_int, [C.c_void_p]),
                            ("jpeg_defaults", None, [C.c_void_p]), ("jpeg_layout", None, [C.c_void_p])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args

    class Host:
        pass
    Host.L = L

    def over(fn, x, shape=None, dtype=F, *extra):
        x = np.ascontiguousarray(x, F)
        out = np.empty(x.shape if shape is None else shape, dtype)
        fn(x.ctypes.data, *extra, out.ctypes.data)
        return out
    Host.ycc = staticmethod(lambda e: over(L.jpeg_ycc, e, None, F, np.asarray(e).size // 3))
    Host.samples = staticmethod(lambda x: over(L.jpeg_samples, x, None, F, np.asarray(x).size // 3))
    Host.fdct = staticmethod(lambda s: over(L.jpeg_fdct, s, None, F, np.asarray(s).size // 64))
    Host.quantise = staticmethod(lambda c, q, dc: over(L.jpeg_quantise, c, None, np.int32, np.asarray(c).size, q, dc))

    def quantise_block(c, chroma, quality):
        c, zz = np.ascontiguousarray(c, F), np.empty(64, np.int16)
        L.jpeg_quantise_block(c.ctypes.data, chroma, quality, zz.ctypes.data)
        return zz
    Host.quantise_block = staticmethod(quantise_block)

    def qtable(quality, chroma):
        out = np.empty(64, np.uint8)
        L.jpeg_qtable(quality, chroma, out.ctypes.data)
        return out
    Host.qtable = staticmethod(qtable)

    def block_code(zz, pred, chroma):
        zz, out = np.ascontiguousarray(zz, np.int16), np.zeros(208, np.uint8)
        n = L.jpeg_block_code(zz.ctypes.data, pred, chroma, out.ctypes.data)
        assert n == L.jpeg_block_bits(zz.ctypes.data, pred, chroma) and n <= 1658
        return n, out
    Host.block_code = staticmethod(block_code)
    return Host


def params(quality=90, subsampling=J.S420, flags=0, reserved=0):
    return state.JpegParams(quality, subsampling, flags, reserved)


def picture(w, h, seed, noise=0.0, special=False):
    """Display-referred linear RGB [h, w, 3]: smooth ramps and a soft disc whose levels the seed draws, optionally with Gaussian noise and
    the special values."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    disc = np.exp(-(((u - 0.6) ** 2 + (v - 0.4) ** 2) * 9.0))
    a = rng.uniform(0.0, 0.3, 3)
    img = np.stack([a[0] + 0.6 * u * u, a[1] + 0.6 * v * (1 - 0.5 * u), a[2] + 0.6 * disc], axis=-1)
    if noise:
        img = img + rng.normal(0.0, noise, img.shape)
    img = img.astype(F)
    if special:
        flat = img.reshape(-1)
        for k, value in enumerate((np.nan, np.inf, -np.inf, -0.0, -1.0, 3e38, 1.0, 1e-30)):
            flat[k::29] = value
    return img


def srgb_bytes(sdr):
    """What rsrt_display_colour_srgb8 makes of sdr: the rounded code."""
    return np.floor(V.code(sdr, V.BT709) + F(0.5)).astype(np.uint8)


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def psnr(a, b):
    e = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if e == 0 else 10.0 * np.log10(255.0 ** 2 / e)


def libjpeg_file(rgb8, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(rgb8, "RGB").save(b, "JPEG", quality=quality, subsampling=PIL_SUB[subsampling], optimize=False)
    return b.getvalue()


def crafted():
    """[(name, w, h, subsampling, coefficients [blocks, 64])]: the entropy coder's edges."""
    out = []

    def add(name, w, h, sub, fill):
        c = np.zeros((J.n_blocks(w, h, sub), 64), np.int16)
        fill(c)
        out.append((name, w, h, sub, c))

    def all_dc(c):
        c[:, 0] = np.arange(c.shape[0]) * 37 % 200 - 100

    def only_63(c):
        c[:, 63] = np.where(np.arange(c.shape[0]) % 2, -1, 1)

    def worst(c):  # 1658 bits a block: every AC at +-1023 (size 10, a 16-bit code), a DC difference of +-2047
        c[:, 1:] = np.where((np.arange(63)[None, :] + np.arange(c.shape[0])[:, None]) % 2, 1023, -1023)
        c[:, 0] = np.where(np.arange(c.shape[0]) % 2, 1023, -1024)

    def runs(c):
        for i, k in enumerate((16, 17, 32, 33)):  # runs of exactly 15, 16, 31 and 32 before coefficient k
            c[i::4, k] = (-1) ** i * (i + 1)
        c[2::4, 63] = 3  # ... and a run of 30 behind one of 31, ending without EOB

    def dc_steps(c):  # differences of 0, +-2047 and small ones, per component
        c[:, 0] = np.array([0, 0, 1023, 1023, -1024, -1024, 1023, 0, -1, 1, 1023, -1024])[np.arange(c.shape[0]) % 12]
    for sub in SUBS:
        add("all AC zero", 24, 16, sub, all_dc)
        add("only coefficient 63", 16, 16, sub, only_63)
        add("1658-bit blocks", 32, 16, sub, worst)
        add("runs of 15, 16, 31, 32", 32, 32, sub, runs)
        add("DC differences", 48, 16, sub, dc_steps)
    # a scan full of 0xFF bytes: the luma AC code for (run 0, size 10) is sixteen bits 0xFF82 .. and a value of 1023 is ten one-bits; at 4:4:4 8 x 8
    # three blocks whose total is steered to 8 k - 1, 8 k and 8 k + 1 bits by the last block's tail, the padding meeting an 0xFF at 8 k - 1
    base = np.zeros((3, 64), np.int16)
    base[0, 1:40] = 1023
    for extra in range(0, 12):
        c = base.copy()
        c[2, 1:1 + extra] = 1
        out.append(("0xFF runs, tail %d" % extra, 8, 8, J.S444, c))
    for extra in range(0, 4):  # ... and a scan that ends in ten one-bits (coefficient 63 at 1023, no EOB): whatever the padding, the last byte is 0xFF
        c = base.copy()
        c[2, 1:1 + extra] = 1
        c[2, 63] = 1023
        out.append(("0xFF runs, ones at the end, tail %d" % extra, 8, 8, J.S444, c))
    return out


# -- step by step -------------------------------------------------------------------------------------------------------------------------
def test_tables_equal_libjpegs_and_the_formulas(host):
    dct, zz, dc, ac = np.empty(64, F), np.empty(64, np.uint8), np.empty((2, 12), np.uint32), np.empty((2, 256), np.uint32)
    host.L.jpeg_tables(dct.ctypes.data, zz.ctypes.data, dc.ctypes.data, ac.ctypes.data)
    assert np.array_equal(dct.view(np.uint32), J.dct_matrix().reshape(-1).view(np.uint32))
    assert np.array_equal(zz, J.zigzag()) and sorted(zz) == list(range(64))
    for chroma in (0, 1):
        for table, got in ((J.huffman(0, chroma), dc[chroma]), (J.huffman(1, chroma), ac[chroma])):
            assert {s: (int(e) & 0xFFFF, int(e) >> 16) for s, e in enumerate(got) if e} == table
        assert len(J.huffman(0, chroma)) == 12 and len(J.huffman(1, chroma)) == 162
    # the largest block: a DC code of at most 9 bits and 11 value bits, 63 ACs of a 16-bit code and 10 value bits
    assert max(n for _, n in J.huffman(0, 0).values()) == 9 and max(n for t in (0, 1) for _, n in J.huffman(1, t).values()) == 16
    for quality in (1, 10, 49, 50, 51, 90, 100):
        for chroma in (0, 1):
            assert np.array_equal(host.qtable(quality, chroma), J.qtable(quality, chroma)), (quality, chroma)
        # ... and libjpeg's own at that quality
        q = decode(libjpeg_file(np.zeros((8, 8, 3), np.uint8), quality, J.S420)).quantization
        for chroma in (0, 1):
            lib = np.array(q[chroma])
            want = J.qtable(quality, chroma)
            assert np.array_equal(lib, want) or np.array_equal(lib, want[J.zigzag()]), (quality, chroma)  # (Pillow's order is its version's)
    assert J.qtable(100, 0).max() == 1 and J.qtable(1, 1).min() == 255 and np.array_equal(J.qtable(50, 0), J.annex_k()["q"][0])


def test_matrix_and_samples_equal_the_restatement(host):
    rng = np.random.default_rng(3)
    e = rng.random((4096, 3)).astype(F)
    assert np.array_equal(host.ycc(e).view(np.uint32), J.ycc(e).view(np.uint32))
    x = np.concatenate([picture(32, 32, 1, 0.03, special=True).reshape(-1, 3), (rng.random((512, 3)) * 1.5 - 0.1).astype(F)])
    s = host.samples(x)
    assert np.array_equal(s.view(np.uint32), J.samples(x).view(np.uint32)) and np.isfinite(s).all()
    assert s[:, 0].min() >= -128 and s[:, 0].max() <= 127 and np.abs(s[:, 1:]).max() <= 127.5 * (1 + 4 * 2.0 ** -24)  # (the header: an ulp or two over)
    # the corners of the cube: JFIF's codes to the last ulp or so
    for rgb, want in (((0, 0, 0), (-128, 0, 0)), ((1, 1, 1), (127, 0, 0)), ((1, 0, 0), (255 * 0.299 - 128, 255 * -0.299 / 1.772, 127.5)),
                      ((0, 0, 1), (255 * 0.114 - 128, 127.5, 255 * -0.114 / 1.402))):
        assert np.abs(host.samples(np.array([rgb], F))[0] - np.array(want)).max() < 1e-4, rgb


def test_a_grey_ramp_has_chroma_below_the_stated_bound_and_zero_coefficients(host):
    """The header says a grey does not give exactly zero chroma but stays below 1e-4 a sample and 1e-3 a coefficient, 0 after the quantiser."""
    g = np.linspace(0.0, 1.0, 64 * 64, dtype=F) ** 2
    s = host.samples(np.stack([g, g, g], axis=-1))
    assert np.abs(s[:, 1:]).max() < 1e-4
    assert np.abs(s[:, 1:]).max() > 0  # (not exact: the three weights' products do not sum to the channel in f32)
    c = host.fdct(s[:, 1].reshape(-1, 8, 8))
    assert np.abs(c).max() < 1e-3
    coefs = J.coefficients(np.stack([g, g, g], axis=-1).reshape(64, 64, 3), quality=100, subsampling=J.S444).reshape(-1, 3, 64)
    assert not coefs[:, 1:].any()


def test_the_hosts_420_chroma_is_the_centre_reduction_with_clamped_taps(host):
    """rsrt_jpeg_coefficients_host's Cb and Cr blocks at odd sizes against a reduction written out tap by tap here: every coordinate
    clamped to the picture, ((p00 + p01) + (p10 + p11)) * 0.25 in f32, then the header's own DCT and quantiser at quality 100."""
    for w, h in ((1, 1), (5, 3), (16, 16), (9, 17), (31, 33)):
        img = picture(w, h, 50 * w + h, 0.05)
        s = host.samples(img)
        mw, mh = -(-w // 16), -(-h // 16)
        got = R.host.jpeg_coefficients(img, 100, "420").reshape(mh, mw, 6, 64)
        for my in range(mh):
            for mx in range(mw):
                for k in (1, 2):
                    blk = np.empty((8, 8), F)
                    for cy in range(8):
                        for cx in range(8):
                            y0, y1 = min(16 * my + 2 * cy, h - 1), min(16 * my + 2 * cy + 1, h - 1)
                            x0, x1 = min(16 * mx + 2 * cx, w - 1), min(16 * mx + 2 * cx + 1, w - 1)
                            blk[cy, cx] = F(F(F(s[y0, x0, k] + s[y0, x1, k]) + F(s[y1, x0, k] + s[y1, x1, k])) * F(0.25))
                    assert np.array_equal(got[my, mx, 3 + k], host.quantise_block(host.fdct(blk), 1, 100)), (w, h, my, mx, k)


def test_dct_equals_the_restatement_and_keeps_the_stated_bound(host):
    rng = np.random.default_rng(5)
    blocks = [rng.uniform(-128, 127, (64, 8, 8)), rng.normal(0, 3, (16, 8, 8)), np.full((1, 8, 8), -128.0), np.full((1, 8, 8), 127.0), np.zeros((1, 8, 8))]
    basis = np.zeros((64, 8, 8))
    for k in range(64):  # single basis functions at full swing: the transform concentrates them in their coefficient
        v, u = divmod(k, 8)
        y, x = np.mgrid[0:8, 0:8]
        basis[k] = 127.5 * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)
    signs = np.where(rng.random((256, 8, 8)) < 0.5, -128.0, 127.0)  # +-128 blocks, and the worst sign pattern of every coefficient
    worst = np.where(basis >= 0, 127.0, -128.0)
    s = np.concatenate(blocks + [basis, signs, worst, -worst - 1]).astype(F)
    c = host.fdct(s)
    assert np.array_equal(c.view(np.uint32), J.fdct(s).view(np.uint32))
    ref = np.einsum("vy,nyx,ux->nvu", J.dct_matrix().astype(np.float64), s.astype(np.float64), J.dct_matrix().astype(np.float64))
    assert np.abs(c - ref).max() < 2e-3  # f32 chains of 16 terms of magnitude up to 1024
    assert c[:, 0, 0].min() >= -1024.001 and c[:, 0, 0].max() <= 1020.001 and np.abs(c.reshape(-1, 64)[:, 1:]).max() <= 1020.001  # the header's bound on |c| (a chroma DC: 8 * 127.5)
    assert abs(c[len(s) - 128 + 0, 0, 0] - 1016) < 1e-3 and np.abs(c.reshape(-1, 64)[:, 1:]).max() > 1019.9  # ... which is reached
    k = 64 + 16 + 3
    assert all(abs(c[k + i].reshape(-1)[i]) > 0.99 * np.abs(c[k + i]).max() for i in range(64))
    assert np.array_equal(c[64 + 16], np.where(np.arange(64).reshape(8, 8) == 0, c[64 + 16, 0, 0], 0)) or np.abs(c[64 + 16].reshape(-1)[1:]).max() < 1e-3  # a constant block: DC only


def test_the_quantisers_ties_and_clamps(host):
    for q in (1, 2, 3, 16, 99, 255):
        k = np.arange(-12, 13)
        ties = (k + 0.5) * q
        c = np.concatenate([ties, np.nextafter(ties.astype(F), F(np.inf)), np.nextafter(ties.astype(F), F(-np.inf)), [0.0, -0.0, 0.49 * q, -0.49 * q, 1e9, -1e9, 1023.5 * q, -1023.5 * q,
                                                                                                                          -1024.4 * q, np.inf, -np.inf]]).astype(F)
        for dc in (0, 1):
            got = host.quantise(c, q, dc)
            r = np.floor((np.abs(c) / F(q)).astype(F) + F(0.5))
            want = np.clip(np.where(c < 0, -r, r), -1024 if dc else -1023, 1023)
            assert np.array_equal(got, want.astype(np.int32)), (q, dc)
            assert got.min() == (-1024 if dc else -1023) and got.max() == 1023
        assert list(host.quantise(np.array([0.5 * q, -0.5 * q, 1.5 * q, -1.5 * q], F), q, 0)) == [1, -1, 2, -2]  # ties go away from zero
    rng = np.random.default_rng(6)
    c = rng.normal(0, 200, (8, 8)).astype(F)
    for chroma in (0, 1):
        for quality in (1, 50, 100):
            assert np.array_equal(host.quantise_block(c, chroma, quality), J.quantise(c, quality, chroma))


def test_scan_order_and_the_predictors_index_arithmetic(host):
    for sub in SUBS:
        last = {}
        for i in range(6 * 7 * 3):
            comp = host.L.jpeg_block_component(i, sub)
            assert comp == J.component(i, sub)
            assert host.L.jpeg_block_pred(i, sub) == J.pred(i, sub) == last.get(comp, -1)  # the running state the arithmetic replaces
            last[comp] = i
    assert [J.component(i, J.S420) for i in range(6)] == [0, 0, 0, 0, 1, 2] and [J.component(i, J.S444) for i in range(3)] == [0, 1, 2]


# -- whole files --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_whole_files_equal_the_restatement_and_decode(w, h):
    img = picture(w, h, 100 * w + h, 0.03, special=True)
    for sub in SUBS:
        for quality in (1, 50, 90, 100):
            got = R.host.encode_jpeg(img, quality, NAMES[sub])
            assert np.array_equal(R.host.jpeg_coefficients(img, quality, NAMES[sub]), J.coefficients(img, quality=quality, subsampling=sub))
            assert got == J.encode(img, quality=quality, subsampling=sub), (w, h, sub, quality)
            assert len(got) <= J.max_bytes(w, h, sub)
            im = decode(got)
            assert im.size == (w, h) and im.mode == "RGB" and im.format == "JPEG"


def test_crafted_blocks_byte_for_byte_and_through_libjpeg(host):
    totals = set()
    for name, w, h, sub, c in crafted():
        got = R.host.jpeg_from_coefficients(c, w, h, 90, NAMES[sub])
        assert got == J.from_coefficients(c, w, h, 90, sub), name
        assert decode(got).size == (w, h), name
        n = J.scan_bits(c, sub)[1]
        bits = [host.block_code(c[i], 0 if J.pred(i, sub) < 0 else int(c[J.pred(i, sub), 0]), 1 if J.component(i, sub) else 0)[0] for i in range(len(c))]
        assert sum(bits) == n and bits == [J.block_bits(c[i], 0 if J.pred(i, sub) < 0 else c[J.pred(i, sub), 0], 1 if J.component(i, sub) else 0) for i in range(len(c))]
        scan = dict(J.segments(got))["scan"]
        if name.startswith("1658"):
            assert max(bits) == 1658 and sub == J.S444 or max(bits) >= 1650
        if name.startswith("only coefficient 63"):  # three ZRLs, a run of 14, no EOB: DC size 0 (2 bits) + 3 * 11 + the code of 0xE1 + 1
            assert bits[0] == 2 + 3 * 11 + J.huffman(1, 0)[0xE1][1] + 1
        if name.startswith("0xFF"):
            totals.add(n % 8)
            assert scan.count(b"\xff\x00") >= 40 and b"\xff\x00\xff\x00" in scan  # (0xFF83 and ten one-bits: pairs of 0xFF, 26 bits apart)
    assert totals == set(range(8))  # every residue: 8 k, 8 k + 1 and 8 k - 1 among them
    # a padded last byte that comes out as 0xFF is stuffed like any other
    zz = np.zeros((3, 64), np.int16)
    found = 0
    for name, w, h, sub, c in crafted():
        if "ones at the end" in name:
            acc, n = J.scan_bits(c, sub)
            pad = -n % 8
            assert (acc << pad | (1 << pad) - 1) & 0xFF == 0xFF
            found += pad > 0
            assert R.host.jpeg_from_coefficients(c, w, h, 90, "444").endswith(b"\xff\x00\xff\xd9")
    assert found >= 2  # the padding met an 0xFF
    # refusals: a value outside the clamp, another count
    zz[0, 5] = 1024
    with pytest.raises(ValueError):
        R.host.jpeg_from_coefficients(zz, 8, 8, 90, "444")
    zz[0, 5], zz[1, 0] = -1023, -1025
    with pytest.raises(ValueError):
        R.host.jpeg_from_coefficients(zz, 8, 8, 90, "444")
    zz[1, 0] = -1024
    R.host.jpeg_from_coefficients(zz, 8, 8, 90, "444")
    with pytest.raises(ValueError):
        R.host.jpeg_from_coefficients(zz, 16, 8, 90, "444")


def test_headers_and_stuffing_by_hand(host):
    p = params(75, J.S420)
    out = np.zeros(700, np.uint8)
    assert host.L.jpeg_headers(out.ctypes.data, 300, 200, C.byref(p)) == J.HEADER_BYTES == 623
    assert out[:623].tobytes() == J.headers(300, 200, 75, J.S420)
    seg = J.segments(out[:623].tobytes() + b"\xff\xd9")
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA, "scan", 0xD9]
    assert seg[0][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00" and seg[3][1] == bytes([8, 0, 200, 1, 44, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [s[1][0] for s in seg[4:8]] == [0x00, 0x10, 0x01, 0x11]
    for raw, n_bits, want in ((b"\xff\x00\xff", 24, b"\xff\x00\x00\xff\x00"), (b"\xab\xfe", 15, b"\xab\xff\x00"), (b"\x80", 1, b"\xff\x00"), (b"\x12\x34", 16, b"\x12\x34"),
                              (b"\x12\x30", 12, b"\x12\x3f"), (b"", 0, b"")):
        src, dst = np.frombuffer(raw + b"\x00", np.uint8).copy(), np.zeros(16, np.uint8)
        n = host.L.jpeg_stuff(src.ctypes.data, n_bits, dst.ctypes.data)
        assert dst[:n].tobytes() == want and host.L.jpeg_stuff(src.ctypes.data, n_bits, None) == n


# -- the independent decoder and encoder ------------------------------------------------------------------------------------------------------
def compare(imgs, quality, sub):
    """(PSNR of ours, PSNR of libjpeg's, our size / libjpeg's) against the rounded sRGB bytes of the pictures imgs, libjpeg encoding those
    bytes; the squared errors and the sizes of all the pictures are pooled."""
    got, want, truth, sizes = [], [], [], [0, 0]
    for img in imgs:
        rgb8 = srgb_bytes(img)
        ours, ref = R.host.encode_jpeg(img, quality, NAMES[sub]), libjpeg_file(rgb8, quality, sub)
        a, b = decode(ours), decode(ref)
        assert a.size == b.size == (img.shape[1], img.shape[0]) and a.quantization == b.quantization
        got.append(np.asarray(a).reshape(-1)); want.append(np.asarray(b).reshape(-1)); truth.append(rgb8.reshape(-1))
        sizes = [sizes[0] + len(ours), sizes[1] + len(ref)]
    truth = np.concatenate(truth)
    return psnr(np.concatenate(got), truth), psnr(np.concatenate(want), truth), sizes[0] / sizes[1]


def pooled(w, h):
    """How many pictures of w x h a PSNR is taken over: one, except at 1 x 1 and 8 x 8.  One code in one channel of a 1 x 1 picture is
    3 dB, and a picture of one block stands or falls with a few coefficients' ties, so these two sizes are measured over as many
    pictures, of different levels, as make 1024 pixels, their squared errors pooled (at 256 pixels the 1 x 1 figure still moves by a
    tenth of a dB with the draw).  From 9 x 17 upward every picture is held to the bound by itself."""
    return -(-1024 // (w * h)) if (w, h) in ((1, 1), (8, 8)) else 1


@pytest.mark.parametrize("w,h", SIZES)
def test_libjpeg_decodes_every_size_as_well_as_its_own_files(w, h):
    for sub in SUBS:
        for quality in (10, 50, 90, 100):
            for noise in (0.0, 0.03):
                ours, ref, _ = compare([picture(w, h, 7 * w + h + 1000 * k, noise) for k in range(pooled(w, h))], quality, sub)
                print("%dx%d %s q%d noise %.2f: %.2f dB, libjpeg %.2f dB" % (w, h, NAMES[sub], quality, noise, ours, ref))
                assert ours >= ref - 1.5, (w, h, sub, quality, noise, ours, ref)


@pytest.mark.parametrize("w,h", [(32, 32), (48, 80), (64, 96)])
def test_whole_mcu_frames_match_libjpegs_quality_and_size(w, h):
    for sub in SUBS:
        for quality in (10, 50, 90, 100):
            for noise in (0.0, 0.03):
                ours, ref, ratio = compare([picture(w, h, 11 * w + h, noise)], quality, sub)
                print("%dx%d %s q%d noise %.2f: %.2f dB, libjpeg %.2f dB, size x %.3f" % (w, h, NAMES[sub], quality, noise, ours, ref, ratio))
                assert ours >= ref - 0.75, (w, h, sub, quality, noise, ours, ref)
                assert ratio <= 1.02, (w, h, sub, quality, noise, ratio)


# -- the AVI ----------------------------------------------------------------------------------------------------------------------------------
def riff(data, at=0, end=None):
    """[(id, form or None, payload or children, offset of the chunk's header)] of the chunks in data[at:end]."""
    out, end = [], len(data) if end is None else end
    while at < end:
        cid, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + n <= end, (cid, at, n)
        if cid in (b"RIFF", b"LIST"):
            out.append((cid, data[at + 8:at + 12], riff(data, at + 12, at + 8 + n), at))
        else:
            out.append((cid, None, data[at + 8:at + 8 + n], at))
        at += 8 + n + (n & 1)
        assert at <= end or at == end + 1
    return out


def read_avi(path):
    """{"avih", "strh", "strf": their fields, "frames": [bytes], "index": [(id, flags, offset, size)], "movi_at": offset of 'movi'}"""
    data = open(path, "rb").read()
    top = riff(data)
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][1] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    hdrl, movi, idx1 = top[0][2]
    assert (hdrl[0], hdrl[1]) == (b"LIST", b"hdrl") and (movi[0], movi[1]) == (b"LIST", b"movi") and idx1[0] == b"idx1"
    avih, strl = hdrl[2]
    assert avih[0] == b"avih" and len(avih[2]) == 56 and (strl[0], strl[1]) == (b"LIST", b"strl")
    strh, strf = strl[2]
    assert strh[0] == b"strh" and len(strh[2]) == 56 and strf[0] == b"strf" and len(strf[2]) == 40
    assert all(c[0] == b"00dc" for c in movi[2]) and all(c[3] % 2 == 0 for c in movi[2])  # every chunk begins at an even offset
    index = [struct.unpack("<4sIII", idx1[2][i:i + 16]) for i in range(0, len(idx1[2]), 16)]
    return {"avih": struct.unpack("<14I", avih[2]), "strh": struct.unpack("<4s4sIHHIIIIIIII4h", strh[2]), "strf": struct.unpack("<IiiHH4sIiiII", strf[2]),
            "frames": [c[2] for c in movi[2]], "index": index, "movi_at": movi[3] + 8, "chunks_at": [c[3] for c in movi[2]], "data": data}


def check_avi(path, n, w, h, fps):
    a = read_avi(path)
    largest = max(len(f) for f in a["frames"])
    assert len(a["frames"]) == n
    usec, _, pad, flags, total, initial, streams, buf, aw, ah = a["avih"][:10]
    assert (usec, pad, flags, total, initial, streams, buf, aw, ah) == (fps[1] * 1000000 // fps[0], 0, 0x10, n, 0, 1, largest, w, h) and a["avih"][10:] == (0, 0, 0, 0)
    s = a["strh"]
    assert s[:2] == (b"vids", b"MJPG") and (s[6], s[7], s[8], s[9], s[10]) == (fps[1], fps[0], 0, n, largest) and s[12] == 0 and s[13:] == (0, 0, w, h)
    assert a["strf"] == (40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    assert len(a["index"]) == n
    for (cid, flags, off, size), frame, at in zip(a["index"], a["frames"], a["chunks_at"]):
        assert (cid, flags, size) == (b"00dc", 0x10, len(frame)) and a["movi_at"] + off == at  # every entry points at its chunk, a key frame
        assert a["data"][at:at + 4] == b"00dc" and decode(frame).size == (w, h)
    return a


def test_avi_chunk_tree_index_and_frames(tmp_path):
    w, h = 24, 18
    frames = [R.host.encode_jpeg(picture(w, h, k, 0.02 * k), 80 + k, "420") for k in range(5)]
    assert any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames)  # both paddings
    path = str(tmp_path / "clip.avi")
    R.host.write_avi_mjpeg(path, frames, w, h, fps=(30000, 1001))
    a = check_avi(path, 5, w, h, (30000, 1001))
    assert a["frames"] == frames
    R.host.write_avi_mjpeg(path, frames[:1], w, h)  # one frame, the default rate; the file is rewritten
    check_avi(path, 1, w, h, (30, 1))
    # refusals: nothing is written
    L, no = R.host.lib(), os.fsencode(str(tmp_path / "no.avi"))
    ptrs, sizes = (C.c_char_p * 2)(frames[0], frames[1]), (C.c_size_t * 2)(len(frames[0]), len(frames[1]))
    assert L.rsrt_avi_mjpeg_write(no, ptrs, sizes, 0, w, h, 30, 1) == 1
    assert L.rsrt_avi_mjpeg_write(no, ptrs, (C.c_size_t * 2)(len(frames[0]), 0), 2, w, h, 30, 1) == 1
    assert L.rsrt_avi_mjpeg_write(no, (C.c_char_p * 2)(frames[0], None), sizes, 2, w, h, 30, 1) == 1
    assert L.rsrt_avi_mjpeg_write(no, ptrs, (C.c_size_t * 2)(len(frames[0]), (1 << 31) - 100), 2, w, h, 30, 1) == 1  # would reach 2 GiB (sizes are checked before bytes are read)
    assert L.rsrt_avi_mjpeg_write(no, None, sizes, 2, w, h, 30, 1) == 1 and L.rsrt_avi_mjpeg_write(None, ptrs, sizes, 2, w, h, 30, 1) == 1
    assert L.rsrt_avi_mjpeg_write(no, ptrs, sizes, 2, 0, h, 30, 1) == 1 and L.rsrt_avi_mjpeg_write(no, ptrs, sizes, 2, w, h, 0, 1) == 1
    assert not os.path.exists(no)
    assert L.rsrt_avi_mjpeg_write(os.fsencode(str(tmp_path / "none" / "x.avi")), ptrs, sizes, 2, w, h, 30, 1) == 2
    with pytest.raises(ValueError):
        R.host.write_avi_mjpeg(str(tmp_path / "no.avi"), [], w, h)


# -- interfaces -------------------------------------------------------------------------------------------------------------------------------
def test_params_struct_defaults_and_sizes(host):
    for kw, ok in (({}, True), ({"quality": 1}, True), ({"quality": 100}, True), ({"quality": 0}, False), ({"quality": 101}, False), ({"subsampling": 1}, True),
                   ({"subsampling": 2}, False), ({"flags": 1}, False), ({"reserved": 1}, False)):
        p = params(**kw)
        assert bool(host.L.jpeg_params_ok(C.byref(p))) == bool(J.params_ok(**dict(J.DEFAULTS, **kw))) == ok, kw
    lay = np.zeros(8, np.uint32)
    host.L.jpeg_layout(lay.ctypes.data)
    P = state.JpegParams
    assert list(lay) == [C.sizeof(P), P.subsampling.offset, P.flags.offset, P.reserved.offset, state.JPEG_420, state.JPEG_444, state.JPEG_BLOCK_BITS, state.JPEG_HEADER_BYTES]
    assert list(lay) == [16, 4, 8, 12, 0, 1, 1664, 623] and (J.S420, J.S444, J.BLOCK_BITS, J.HEADER_BYTES) == (0, 1, 1664, 623)
    p = P()
    host.L.jpeg_defaults(C.byref(p))
    d = state.JPEG_DEFAULTS
    assert {k: getattr(p, k) for k in ("quality", "subsampling", "flags", "reserved")} == J.DEFAULTS == dict(d, subsampling=state.JPEG_SUBSAMPLINGS[d["subsampling"]])
    assert J.DEFAULTS == {"quality": 90, "subsampling": 0, "flags": 0, "reserved": 0} and state.JPEG_SUBSAMPLINGS == J.SUBSAMPLINGS
    q = state.jpeg_params()
    assert (q.quality, q.subsampling, q.flags, q.reserved) == (90, 0, 0, 0)
    # sizes by hand: 1920 x 1080 is 120 x 68 MCUs of six blocks at 4:2:0 and 240 x 135 of three at 4:4:4; 208 bytes a block, each stuffed
    for (w, h, sub), blocks in {(1920, 1080, 0): 48960, (1920, 1080, 1): 97200, (1, 1, 0): 6, (1, 1, 1): 3, (16, 16, 0): 6, (17, 16, 0): 12, (16, 17, 1): 18, (65535, 1, 1): 8192 * 3}.items():
        assert host.L.jpeg_blocks(w, h, sub) == J.n_blocks(w, h, sub) == state.jpeg_blocks(w, h, sub) == blocks
        assert host.L.jpeg_max_bytes(w, h, sub) == J.max_bytes(w, h, sub) == state.jpeg_max_bytes(w, h, sub) == 623 + 416 * blocks + 2
    # the size the device refuses the host refuses too: a worst case of 2^32 bits, 2 581 111 blocks and more
    L, big, n = R.host.lib(), np.zeros(3, F), C.c_size_t(7)
    for w, h, sub, ok in ((65535, 8, 1, True), (65535, 840, 1, True), (65535, 848, 1, False), (65535, 65535, 0, False), (16 * 1638, 16 * 263, 0, False), (16 * 1638, 16 * 262, 0, True)):
        assert (J.n_blocks(w, h, sub) * 1664 < 1 << 32) == ok
        if not ok:  # (refused before anything is read or allocated)
            p = params(90, sub)
            assert L.rsrt_jpeg_encode_host(big.ctypes.data, w, h, C.byref(p), None, 0, C.byref(n)) == 1 and n.value == 7
            assert L.rsrt_jpeg_coefficients_host(big.ctypes.data, w, h, C.byref(p), big.ctypes.data, 64 * J.n_blocks(w, h, sub)) == 1
            assert L.rsrt_jpeg_from_coefficients(big.ctypes.data, 64 * J.n_blocks(w, h, sub), w, h, C.byref(p), None, 0, C.byref(n)) == 1
    for w, h in ((0, 5), (5, 0), (65536, 1), (1, 65536)):
        assert host.L.jpeg_max_bytes(w, h, 0) == J.max_bytes(w, h, 0) == state.jpeg_max_bytes(w, h) == 0
    sig = inspect.signature(R.State.display_jpeg).parameters
    names = ("source", "exposure", "white", "lut_strength", "shadows", "highlights", "bloom_intensity", "quality", "subsampling", "sample_total")
    assert list(sig)[1:11] == list(names) and [sig[k].default for k in names] == ["mean", None, None, None, None, None, 0.0, None, None, None]
    img = picture(9, 7, 1)
    assert R.host.encode_jpeg(img) == R.host.encode_jpeg(img, 90, "420") == R.host.encode_jpeg(img, 90, state.JPEG_420)
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling=2)):
        with pytest.raises(ValueError):
            R.host.encode_jpeg(img, **bad)
    # the host's size protocol: told with no room, refused with one byte too few and the buffer untouched, written into exactly the size
    L, p, n = R.host.lib(), params(), C.c_size_t(0)
    assert L.rsrt_jpeg_encode_host(img.ctypes.data, 9, 7, C.byref(p), None, 0, C.byref(n)) == 2 and n.value == len(R.host.encode_jpeg(img))
    buf = np.full(n.value, 7, np.uint8)
    assert L.rsrt_jpeg_encode_host(img.ctypes.data, 9, 7, C.byref(p), buf.ctypes.data, n.value - 1, C.byref(n)) == 2 and (buf == 7).all()
    assert L.rsrt_jpeg_encode_host(img.ctypes.data, 9, 7, C.byref(p), buf.ctypes.data, n.value, C.byref(n)) == 0 and buf.tobytes() == R.host.encode_jpeg(img)
    assert L.rsrt_jpeg_encode_host(None, 9, 7, C.byref(p), buf.ctypes.data, n.value, C.byref(n)) == 1 and L.rsrt_jpeg_encode_host(img.ctypes.data, 9, 7, None, None, 0, C.byref(n)) == 1


def test_libraries_export_the_jpeg_pass():
    lib = C.CDLL(_build.build_hip())
    assert all(hasattr(lib, n) for n in ("rsrt_display_jpeg", "rsrt_display_jpeg_coefficients", "rsrt_jpeg_encode_coefficients"))
    hostlib = C.CDLL(_build.build_host())
    assert all(hasattr(hostlib, n) for n in ("rsrt_jpeg_encode_host", "rsrt_jpeg_from_coefficients", "rsrt_jpeg_coefficients_host", "rsrt_avi_mjpeg_write"))
    assert all(hasattr(R.State, n) for n in ("display_jpeg", "jpeg_coefficients", "jpeg_encode")) and not hasattr(state.MultiState, "display_jpeg")
    assert all(hasattr(R.host, n) for n in ("encode_jpeg", "write_avi_mjpeg")) and hasattr(state, "JPEG_DEFAULTS") and hasattr(state, "JpegParams")
    hdr = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    integration = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    for n in ("rsrt_display_jpeg", "rsrt_display_jpeg_coefficients", "rsrt_jpeg_encode_coefficients"):
        assert "Rust: pub fn %s(" % n in hdr and n in integration
    assert "rsrt_avi_mjpeg_write" in integration and "rsrt_jpeg_encode_host" in integration
    cpp = open(os.path.join(util.ROOT, "include", "rsrt_state.hpp")).read()
    assert "display_jpeg(" in cpp and "jpeg_defaults()" in cpp


def test_jpeg_kernels_use_no_scratch():
    import test_code_object
    md = test_code_object.kernel_metadata()
    names = sorted(n for n in md if "rt_jpeg_" in n)
    assert len(names) == 5 and sum("rt_jpeg_blocks_kernel" in n for n in names) == 2, names  # <420>, <444>, count, scan, pack
    assert all(any(k in n for n in names) for k in ("rt_jpeg_count_kernel", "rt_jpeg_scan_kernel", "rt_jpeg_pack_kernel"))
    for n in names:
        k = md[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k.get("sgpr_spill_count", 0) == 0, (n, k)


def build_cpp_demo(tmp_path):
    exe = str(tmp_path / "jpeg_demo")
    pkg = os.path.join(util.ROOT, "rsoderh-raytracing_amd")
    _build.build_host()
    _build.build_hip()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "jpeg_demo.cpp"), "-o", exe, "-L", pkg, "-lrsrt", "-lrsrt_host",
           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_cpp_state_jpeg_compiles(tmp_path):
    build_cpp_demo(tmp_path)


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    """jpeg_host.cpp as a program of its own (-DJPEG_HOST_MAIN, with the host library's image_io.cpp) under -fsanitize=address,undefined: the
    host encoder and the sequential coder over the sizes, special values and crafted blocks above.  On the CPU, outside Python."""
    exe = str(tmp_path / "jpeg_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DJPEG_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-Wextra", "-I", os.path.join(util.ROOT, "include"), SOURCE, os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "host", "image_io.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "jpeg_host: ok" in r.stdout, r.stdout
