"""The local exposure pass and the graded display (include/rsrt_local.h) restated in numpy: a pixel's log-luminance q from its float's
bit pattern, the bilateral grid and its three tents in uint32, the slice, the gain and rsrt_local_exp2 in float32, operation for
operation and in the header's order, and the graded display pixel over bloom_ref's restatement of the display transform.  The CPU
evaluation of the header (tests/test_local.py) and the GPU kernels (tests/test_local_gpu.py) both equal it bit for bit."""
import numpy as np

import bloom_ref
import exposure_ref

F = np.float32
GZ = 32
Q_LO = 111 << 8
Q_MAX = 8191
SKIPPED = 0xffffffff
CELLS = (8, 16, 32, 64)
DEFAULTS = {"cell": 32, "shadows": 0.5, "highlights": 0.5, "key": 0.18, "max_stops": 4.0}
EXP2_C = (F(0.6930321455), F(0.2413797677), F(0.05203237012), F(0.01355574746))


def params_ok(shadows, highlights, key, max_stops, flags=0):
    s, h, k, m = F(shadows), F(highlights), F(key), F(max_stops)
    return bool(0 <= s <= 1 and 0 <= h <= 1 and np.isfinite(k) and k > 0 and 0 <= m <= 16 and flags == 0)


def cells(n, cell):
    return (n + cell - 1) // cell


def q_of_luminance(lum):
    """rsrt_local_q of every luminance, whatever its sign: uint32."""
    b = (np.asarray(lum, F).view(np.uint32) >> 15).astype(np.int64)
    return (np.clip(b, Q_LO, Q_LO + Q_MAX) - Q_LO).astype(np.uint32)


def q_map(sums, total):
    """rsrt_local_q_of per pixel: [h, w] uint32, SKIPPED where !(L > 0)."""
    lum = exposure_ref.luminance(sums, total)
    with np.errstate(all="ignore"):
        counted = lum > 0
    return np.where(counted, q_of_luminance(lum), np.uint32(SKIPPED)).astype(np.uint32)


def raw_grid(q, cell):
    """[32, gy, gx, 2] uint32 (count, sum of q) of a q map [h, w]."""
    h, w = q.shape
    gy, gx = cells(h, cell), cells(w, cell)
    y, x = np.nonzero(q != SKIPPED)
    v = q[y, x].astype(np.int64)
    at = ((v >> 8) * gy + y // cell) * gx + x // cell
    n = GZ * gy * gx
    grid = np.stack([np.bincount(at, minlength=n), np.bincount(at, weights=v.astype(np.float64), minlength=n).astype(np.int64)], axis=-1)
    assert grid.max(initial=0) < 1 << 32
    return grid.astype(np.uint32).reshape(GZ, gy, gx, 2)


def blur(grid):
    """The 1-2-1 tent along x, then y, then z, zero outside, in uint32."""
    g = np.asarray(grid, np.uint32)
    for axis in (2, 1, 0):
        pad = [(0, 0)] * 4
        pad[axis] = (1, 1)
        p = np.pad(g, pad)
        n = g.shape[axis]
        sl = lambda a: tuple(slice(a, a + n) if k == axis else slice(None) for k in range(4))  # noqa: E731
        g = (p[sl(0)] + np.uint32(2) * p[sl(1)] + p[sl(2)]).astype(np.uint32)
    return g


def grid_of(sums, total, cell):
    """The blurred grid of an image of sums, as rsrt_local_exposure_download returns it."""
    return blur(raw_grid(q_map(sums, total), cell))


def axis(u, g):
    """i0, i1, t of clamped coordinates u (float32) along g cells."""
    i0 = u.astype(np.int64)
    return i0, np.minimum(i0 + 1, g - 1), (u - i0.astype(F)).astype(F)


def coord(i, cell, g):
    return np.clip(((i.astype(F) + F(0.5)) / F(cell) - F(0.5)).astype(F), F(0), F(g - 1)).astype(F)


def slice_parts(grid, q, cell):
    """num, den of the slice at every pixel of the q map (float32; garbage where q is SKIPPED)."""
    h, w = q.shape
    gz, gy, gx, _ = grid.shape
    x0, x1, tx = axis(coord(np.arange(w), cell, gx), gx)
    y0, y1, ty = axis(coord(np.arange(h), cell, gy), gy)
    qq = np.where(q == SKIPPED, 0, q).astype(np.int64)
    z0, z1, tz = axis(np.clip((qq.astype(F) / F(256) - F(0.5)).astype(F), F(0), F(GZ - 1)).astype(F), GZ)
    xs, ys, zs = (x0[None, :], x1[None, :]), (y0[:, None], y1[:, None]), (z0, z1)
    wx, wy, wz = ((F(1) - tx).astype(F)[None, :], tx[None, :]), ((F(1) - ty).astype(F)[:, None], ty[:, None]), ((F(1) - tz).astype(F), tz)
    num, den = np.zeros((h, w), F), np.zeros((h, w), F)
    for k in range(8):
        kz, ky, kx = k >> 2, (k >> 1) & 1, k & 1
        wk = ((wz[kz] * wy[ky]).astype(F) * wx[kx]).astype(F)
        c = grid[zs[kz], ys[ky], xs[kx]]
        num = (num + (wk * c[..., 1].astype(F)).astype(F)).astype(F)
        den = (den + (wk * c[..., 0].astype(F)).astype(F)).astype(F)
    return num, den


def base_of(grid, q, cell):
    num, den = slice_parts(grid, q, cell)
    with np.errstate(all="ignore"):
        return (num / den).astype(F)


def exp2(e):
    """rsrt_local_exp2 of float32 e, |e| <= 16."""
    e = np.asarray(e, F)
    n = e.astype(np.int32)  # truncates
    n = np.where(n.astype(F) > e, n - 1, n).astype(np.int32)
    f = (e - n.astype(F)).astype(F)
    p = np.full(e.shape, EXP2_C[3], F)
    for c in (EXP2_C[2], EXP2_C[1], EXP2_C[0], F(1)):
        p = ((p * f).astype(F) + c).astype(F)
    return (p * ((n + 127).astype(np.uint32) << np.uint32(23)).view(F)).astype(F)


def mid_of(key, exposure):
    with np.errstate(all="ignore"):
        return F(q_of_luminance(F(F(key) / F(exposure))))


def gain_of_base(base, mid, shadows, highlights, max_stops):
    with np.errstate(all="ignore"):
        d = ((np.asarray(base, F) - F(mid)).astype(F) * (F(1) / F(256))).astype(F)
        s = np.where(d > 0, F(highlights), F(shadows)).astype(F)
        m = F(max_stops)
        v = (-(s * d).astype(F)).astype(F)
        e = np.where(v < -m, -m, np.where(v > m, m, v)).astype(F)
        return exp2(e)


def gains(sums, total, exposure, grid, cell, shadows=DEFAULTS["shadows"], highlights=DEFAULTS["highlights"], key=DEFAULTS["key"],
          max_stops=DEFAULTS["max_stops"]):
    """rsrt_local_gain_download: [h, w] float32, 1 at skipped pixels."""
    assert params_ok(shadows, highlights, key, max_stops)
    q = q_map(sums, total)
    base = np.where(q == SKIPPED, F(0), base_of(grid, q, cell)).astype(F)  # (a skipped pixel has no base: 0 / 0)
    return np.where(q == SKIPPED, F(1), gain_of_base(base, mid_of(key, exposure), shadows, highlights, max_stops)).astype(F)


def display(sums, total, exposure, gain, intensity=0.0, b=None):
    """rsrt_display_pixel_local per pixel: [h, w, 4] uint8 from sums [h, w, >=3], the gains [h, w] and, with intensity > 0, the bloom
    image b [ceil(h/2), ceil(w/2), >=3]."""
    h, w = sums.shape[:2]
    with np.errstate(all="ignore"):
        mean = (np.asarray(sums, F)[..., :3] / F(total)).astype(np.float16).astype(F)
        hdr = (mean * F(exposure)).astype(F)
        up = bloom_ref.up(np.asarray(b, F)[..., :3], h, w) if intensity > 0 else np.zeros((h, w, 3), F)
        hdr = (hdr + (F(intensity) * up).astype(F)).astype(F)
        hdr = (hdr * np.asarray(gain, F)[..., None]).astype(F)
    return bloom_ref.tone_map_encode(hdr)


def synthetic(h, w, seed, specials=True):
    """Sums [h, w, 4] float32 as an accumulator holds them (to be read with total 1 or 3), in the style of bloom_ref.synthetic but
    with the range a local exposure is for: a dim lognormal room (around 2^-4), a window of sky 2^6 brighter in the right quarter,
    bright dots, some exact zeros and, where the frame has room, the special pixels — NaN, +inf, -inf, a negative, -0, a denormal and
    3e38.  Returns (sums, {name: flat pixel index})."""
    rng = np.random.default_rng(seed)
    s = np.empty((h, w, 4), F)
    s[..., :3] = np.exp(rng.normal(-3.0, 1.0, (h, w, 3))).astype(F)
    s[..., 3] = 1
    if w >= 4:
        s[: max(1, (2 * h) // 3), (3 * w) // 4:, :3] *= F(64)  # the window
    n = h * w
    flat = s.reshape(-1, 4)
    for i in rng.choice(n, size=max(1, n // 40), replace=False):  # the dots
        flat[i, :3] = np.exp(rng.normal(6.0, 2.0, 3)).astype(F)
    if n >= 16:
        for i in rng.choice(n, size=max(1, n // 50), replace=False):  # black: skipped
            flat[i, :3] = 0
    special = {}
    if specials and n >= 16:
        names = ["nan", "inf", "neg_inf", "negative", "neg_zero", "denormal", "huge"]
        special = {k: int(i) for k, i in zip(names, rng.choice(n, size=len(names), replace=False))}
        flat[special["nan"], 1] = np.nan
        flat[special["inf"], 2] = np.inf
        flat[special["neg_inf"], 0] = -np.inf
        flat[special["negative"], :3] = (-3.0, 0.5, -0.25)
        flat[special["neg_zero"], :3] = -0.0
        flat[special["denormal"], :3] = 1e-41
        flat[special["huge"], :3] = 3e38
    return s, special
