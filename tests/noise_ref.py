"""The noise estimate (include/rsrt_noise.h) restated in numpy float32, operation for operation: the per-pixel error from a snapshot's
sums and the accumulator's, the per-tile sum as a wave makes it — lane l of 64 adds pixels l, l + 64, ... of the tile in that order,
six butterfly adds follow — and the summary over the tile map.  The CPU evaluation of the header (tests/test_noise.py) and the GPU
kernel (tests/test_noise_gpu.py) both equal it bit for bit."""
import numpy as np

F = np.float32
EPS = F(1e-3)
TILE = (16, 16)


def tile_ok(tile_w, tile_h):
    t = tile_w * tile_h
    return tile_w > 0 and tile_h > 0 and t % 64 == 0 and t <= 4096


def pixel_error(s1, n1, s2, n2):
    """[H, W] float32 from the snapshot's sums s1 [H, W, >=3] of n1 samples and the accumulator's sums s2 of n2."""
    with np.errstate(all="ignore"):
        a = np.asarray(s1, F)[..., :3] / F(n1)
        m = np.asarray(s2, F)[..., :3] / F(n2)
        d = np.abs(m - a)
        num = (d[..., 0] + d[..., 1]) + d[..., 2]
        s = (m[..., 0] + m[..., 1]) + m[..., 2]
        e = num / np.sqrt(np.where(s > 0, s, F(0)) + EPS)
        return np.where(np.isnan(e), F(np.inf), e).astype(F)


def tile_errors(e, tile=TILE):
    """[tiles_y, tiles_x] float32: the mean of the pixel errors e [H, W] over each tile's pixels inside the frame."""
    tw, th = tile
    assert tile_ok(tw, th)
    H, W = e.shape
    ty, tx = -(-H // th), -(-W // tw)
    pad = np.zeros((ty * th, tx * tw), F)
    pad[:H, :W] = e
    inside = np.zeros(pad.shape, bool)
    inside[:H, :W] = True
    # [ty, tx, T] in the order of the index inside the tile, then [ty, tx, T / 64, 64]: row j holds the pixels lane l takes in step j
    blocks = lambda a: a.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty, tx, (tw * th) // 64, 64)  # noqa: E731
    eb, ib = blocks(pad), blocks(inside)
    with np.errstate(all="ignore"):
        v = np.zeros((ty, tx, 64), F)
        for j in range(eb.shape[2]):  # sequentially down the columns; a pixel outside the frame adds nothing
            v = np.where(ib[:, :, j], v + eb[:, :, j], v)
        lanes = np.arange(64)
        for k in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lanes ^ k]
        assert (v.view(np.uint32) == v[:, :, :1].view(np.uint32)).all()  # f32 addition commutes: every lane ends with the same bits
        count = ib.sum(axis=(2, 3)).astype(F)
        return (v[:, :, 0] / count).astype(F)


def summary(tiles, threshold=0.0):
    """What rsrt_noise_download reports: the maximum, the sequential f32 mean and the tiles above the threshold (an inf always is)."""
    flat = np.asarray(tiles, F).ravel()
    total = F(0)
    with np.errstate(all="ignore"):
        for t in flat:
            total = F(total + t)
        mean = F(total / F(flat.size))
    above = int(((flat > F(threshold)) | np.isposinf(flat)).sum())
    return {"max_error": float(flat.max()), "mean_error": float(mean), "tiles_x": tiles.shape[1], "tiles_y": tiles.shape[0], "tiles_above": above}


def estimate(s1, n1, s2, n2, tile=TILE, threshold=0.0):
    tiles = tile_errors(pixel_error(s1, n1, s2, n2), tile)
    return tiles, summary(tiles, threshold)


def synthetic(h, w, n1, n2, seed):
    """Sums of n1 and of n2 samples [h, w, 4] float32 as an accumulator holds them (alpha = the count), with the special pixels where
    the frame has room: a zero pixel, a negative sum, an inf and a NaN (each in either buffer)."""
    rng = np.random.default_rng(seed)
    first = rng.gamma(2.0, 0.4, (h, w, 3)).astype(F) * F(n1)
    rest = rng.gamma(2.0, 0.4, (h, w, 3)).astype(F) * F(n2 - n1)
    s1 = np.empty((h, w, 4), F)
    s2 = np.empty((h, w, 4), F)
    s1[..., :3], s1[..., 3] = first, n1
    s2[..., :3], s2[..., 3] = first + rest, n2
    flat1, flat2 = s1.reshape(-1, 4), s2.reshape(-1, 4)
    n = h * w
    special = {}
    if n >= 16:
        special = {"zero": n // 7, "negative": n // 5, "inf": n // 3, "nan": n // 2, "nan_snapshot": n - 1}
        flat1[special["zero"], :3] = 0
        flat2[special["zero"], :3] = 0
        flat2[special["negative"], :3] = (-3.0, -0.5, 0.25)
        flat2[special["inf"], 1] = np.inf
        flat2[special["nan"], 2] = np.nan
        flat1[special["nan_snapshot"], 0] = np.nan
    return s1, s2, special
