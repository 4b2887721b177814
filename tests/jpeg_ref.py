"""The JPEG pass (include/rsrt_jpeg.h) restated in numpy and plain integers, step for step: the display colour of a pixel over
video_ref's restatement of the colour display's chain and of the continuous sRGB code, JFIF's matrix, the level-shifted float samples, the
clamped 4:2:0 reduction, the 8 x 8 DCT as sixteen-term chains in float32 in the header's order over a matrix computed here in float64,
the IJG scaling of the Annex K tables, the quantiser, the order of the blocks with its index arithmetic for the DC predictor, the
Huffman code and the file.  The Annex K tables are not read from the header: they are taken out of a file that Pillow's libjpeg wrote
(quality 50 scales the quantisation tables by one, and without optimize= its Huffman tables are the standard's typical ones).  The CPU
evaluation of the header (tests/test_jpeg.py) and the GPU kernels (tests/test_jpeg_gpu.py) both equal this byte for byte."""
import functools
import io

import numpy as np

import video_ref

F = np.float32
S420, S444 = 0, 1
SUBSAMPLINGS = {"420": S420, "444": S444}
DEFAULTS = {"quality": 90, "subsampling": S420, "flags": 0, "reserved": 0}
HEADER_BYTES = 623
BLOCK_BITS = 1664


def params_ok(quality, subsampling, flags=0, reserved=0):
    return 1 <= quality <= 100 and subsampling in (S420, S444) and flags == 0 and reserved == 0


def zigzag():
    """natural index v * 8 + u of zigzag position k"""
    out = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]
        out += [v * 8 + u for v, u in (cells if d % 2 else cells[::-1])]
    return np.array(out)


def segments(data):
    """[(marker, payload)] of a JPEG file up to and with SOS, then ("scan", the entropy-coded bytes) and (0xD9, b"")."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        m, n = data[i + 1], data[i + 2] << 8 | data[i + 3]
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9"
    out.append(("scan", data[i:-2]))
    out.append((0xD9, b""))
    return out


@functools.lru_cache(None)
def annex_k():
    """{"q": [luma, chroma] natural order, "dht": {(class, id): (bits, vals)}} out of a file libjpeg wrote."""
    from PIL import Image
    b = io.BytesIO()
    Image.new("RGB", (16, 16), (10, 200, 30)).save(b, "JPEG", quality=50, subsampling=2, optimize=False)
    q, dht, zz = {}, {}, zigzag()
    for m, p in segments(b.getvalue()):
        if m == 0xDB:
            for j in range(0, len(p), 65):
                t = np.zeros(64, np.int64)
                t[zz] = list(p[j + 1:j + 65])
                q[p[j]] = t
        if m == 0xC4:
            j = 0
            while j < len(p):
                bits = list(p[j + 1:j + 17])
                dht[(p[j] >> 4, p[j] & 15)] = (bits, list(p[j + 17:j + 17 + sum(bits)]))
                j += 17 + sum(bits)
    return {"q": [q[0], q[1]], "dht": dht}


@functools.lru_cache(None)
def huffman(ac, chroma):
    """{symbol: (code, length)} by T.81 Annex C."""
    bits, vals = annex_k()["dht"][(ac, chroma)]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def qtable(quality, chroma):
    """Step 5's divisors, natural order, int64 [64]."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((annex_k()["q"][chroma] * s + 50) // 100, 1, 255)


@functools.lru_cache(None)
def dct_matrix():
    u, x = np.mgrid[0:8, 0:8]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16.0)
    d[0, :] = np.sqrt(0.125)
    return d.astype(F)


def ycc(e):
    """Step 2's matrix on E' [..., 3]."""
    e = np.asarray(e, F)
    y = (((F(0.299) * e[..., 0]).astype(F) + (F(0.587) * e[..., 1]).astype(F)).astype(F) + (F(0.114) * e[..., 2]).astype(F)).astype(F)
    return np.stack([y, ((e[..., 2] - y).astype(F) / F(1.772)).astype(F), ((e[..., 0] - y).astype(F) / F(1.402)).astype(F)], axis=-1)


def samples(sdr):
    """Steps 1 and 2: sdr [h, w, 3] -> sY, sCb, sCr [h, w, 3], float32."""
    c = ycc(video_ref.signal(sdr, video_ref.BT709))
    return np.stack([((F(255) * c[..., 0]).astype(F) - F(128)).astype(F), (F(255) * c[..., 1]).astype(F), (F(255) * c[..., 2]).astype(F)], axis=-1)


def fdct(s):
    """Step 4 on blocks [..., 8 (y), 8 (x)] -> [..., 8 (v), 8 (u)]."""
    s, d = np.asarray(s, F), dct_matrix()
    t = (d[:, 0] * s[..., :, 0:1]).astype(F)  # [.., y, u]
    for k in range(1, 8):
        t = (t + (d[:, k] * s[..., :, k:k + 1]).astype(F)).astype(F)
    c = (d[:, 0:1] * t[..., 0:1, :]).astype(F)  # [.., v, u]
    for k in range(1, 8):
        c = (c + (d[:, k:k + 1] * t[..., k:k + 1, :]).astype(F)).astype(F)
    return c


def quantise(c, quality, chroma):
    """Step 5 on coefficients [..., 8, 8] -> int16 [..., 64] in zigzag order."""
    c = np.asarray(c, F).reshape(c.shape[:-2] + (64,))
    q = qtable(quality, chroma).astype(F)
    r = np.floor(((np.abs(c) / q).astype(F) + F(0.5)).astype(F))
    r = np.where(c < 0, -r, r)
    lo = np.full(64, -1023.0)
    lo[0] = -1024.0
    return np.clip(r, lo, 1023.0).astype(np.int16)[..., zigzag()]


def geometry(w, h, subsampling):
    side, per = (8, 3) if subsampling == S444 else (16, 6)
    return side, per, -(-w // side), -(-h // side)


def n_blocks(w, h, subsampling):
    _, per, mw, mh = geometry(w, h, subsampling)
    return per * mw * mh


def max_bytes(w, h, subsampling):
    return HEADER_BYTES + 2 * (BLOCK_BITS // 8) * n_blocks(w, h, subsampling) + 2 if 1 <= w <= 65535 and 1 <= h <= 65535 else 0


def component(i, subsampling):
    return i % 3 if subsampling == S444 else max(0, i % 6 - 3)


def pred(i, subsampling):
    """Step 6: the block whose DC predicts block i's, or -1."""
    if subsampling == S444:
        return i - 3 if i >= 3 else -1
    k = i % 6
    if 1 <= k <= 3:
        return i - 1
    if i < 6:
        return -1
    return i - 3 if k == 0 else i - 6


def coefficients(sdr, quality=90, subsampling=S420, **_):
    """Steps 1 to 5 of a picture sdr [h, w, 3]: int16 [blocks, 64], scan order."""
    h, w = sdr.shape[:2]
    side, per, mw, mh = geometry(w, h, subsampling)
    s = samples(sdr)
    ys, xs = np.clip(np.arange(mh * side), 0, h - 1), np.clip(np.arange(mw * side), 0, w - 1)
    s = s[ys[:, None], xs[None, :]]  # every coordinate clamped to the picture

    def blocks(plane):  # [H, W] -> [H / 8, W / 8, 8, 8]
        return plane.reshape(plane.shape[0] // 8, 8, plane.shape[1] // 8, 8).transpose(0, 2, 1, 3)
    y = quantise(fdct(blocks(s[..., 0])), quality, 0)
    if subsampling == S420:
        c = [quantise(fdct(blocks(video_ref.reduce(s[..., k], video_ref.CENTRE))), quality, 1) for k in (1, 2)]
        y = y.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64)
        out = np.concatenate([y, c[0][:, :, None], c[1][:, :, None]], axis=2)
    else:
        c = [quantise(fdct(blocks(s[..., k])), quality, 1) for k in (1, 2)]
        out = np.stack([y, c[0], c[1]], axis=2)
    return np.ascontiguousarray(out.reshape(-1, 64))


def size_of(v):
    return int(abs(int(v))).bit_length()


def block_code(zz, pdc, chroma):
    """Step 7: [(bits, length)] of a block."""
    def value(v, n):
        return (v if v >= 0 else v - 1) & ((1 << n) - 1)
    dc, ac = huffman(0, chroma), huffman(1, chroma)
    d = int(zz[0]) - int(pdc)
    out = [dc[size_of(d)], (value(d, size_of(d)), size_of(d))]
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        out += [ac[0xF0]] * (run // 16)
        out += [ac[(run % 16) << 4 | size_of(v)], (value(v, size_of(v)), size_of(v))]
        run = 0
    if int(zz[63]) == 0:
        out.append(ac[0x00])
    return out


def block_bits(zz, pdc, chroma):
    return sum(n for _, n in block_code(zz, pdc, chroma))


def scan_bits(coefs, subsampling):
    """(the scan as one integer, its bit count)"""
    coefs = np.asarray(coefs).reshape(-1, 64)
    acc, n = 0, 0
    for i in range(coefs.shape[0]):
        p = pred(i, subsampling)
        for bits, length in block_code(coefs[i], 0 if p < 0 else coefs[p][0], 1 if component(i, subsampling) else 0):
            acc, n = acc << length | bits, n + length
    return acc, n


def headers(w, h, quality, subsampling):
    zz = zigzag()
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in (0, 1):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in qtable(quality, t)[zz])
    out += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x11 if subsampling == S444 else 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for ac, chroma in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = annex_k()["dht"][(ac, chroma)]
        out += b"\xff\xc4" + bytes([0, 19 + len(vals), ac << 4 | chroma]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def from_coefficients(coefs, w, h, quality=90, subsampling=S420, **_):
    """Steps 6 to 8: the file of coefficients [blocks, 64]."""
    acc, n = scan_bits(coefs, subsampling)
    pad = -n % 8
    raw = (acc << pad | (1 << pad) - 1).to_bytes((n + pad) // 8, "big")
    return headers(w, h, quality, subsampling) + raw.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def encode(sdr, **jpeg):
    """rsrt_jpeg_encode_host: the file of a picture sdr [h, w, 3]."""
    q = dict(DEFAULTS, **jpeg)
    assert params_ok(**q)
    return from_coefficients(coefficients(sdr, **q), sdr.shape[1], sdr.shape[0], **q)


def display(sums, total, exposure, white=(1.0, 1.0, 1.0), lut=None, strength=0.0, gain=None, intensity=0.0, b=None, **jpeg):
    """rsrt_display_jpeg on the host: (the file, the coefficients)."""
    q = dict(DEFAULTS, **jpeg)
    sdr = video_ref.source(sums, total, exposure, white, lut, strength, gain, intensity, b)
    c = coefficients(sdr, **q)
    return from_coefficients(c, sdr.shape[1], sdr.shape[0], **q), c
