"""Edge inputs of the image-space passes (the denoiser, the variance guidance, the display and the binary16 mean): named cases of
(sums, aov) in the layout of test_denoise.synthetic — sums [H, W, 4] (the accumulator: radiance sums, alpha), aov [H, W, 8] (albedo
sums, hits, normal sums, distance sums) — with their sample totals S and T.  Each case starts from an ordinary frame and sets the
values where binary16 and float32 run out: far and tiny depths, zero and near-epsilon albedo, misses, huge and subnormal radiance.
Every case's inputs are finite."""
import collections
import os
import re

import numpy as np

import denoise_ref
import util

F = np.float32
S_TOTAL, T_TOTAL = 4, 4  # T a power of two: a mean of distance_sum / T is exactly the value a case asks for

# image shapes (h, w) around the levels' 64 x 4 workgroup, and a thin image whose level-8 step (128) is wider than itself
SHAPES = [(4, 64), (5, 65), (3, 63), (1, 257), (257, 1), (2, 3)]
NARROW = (9, 7)

# mean first-hit distances at and around the binary16 limit: 65504 is the largest finite value, 65520 the first that rounds to inf
FAR_DEPTHS = [65503.0, 65504.0, 65519.99, 65520.0, 1e5, 1e7]

Case = collections.namedtuple("Case", "name sums aov S T")


def base(h, w, seed):
    """An ordinary frame: albedo near 0.5, unit normals, depths of 3 to 5, moderate noisy radiance, every sample a hit."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    alb = np.where((xs < (w + 1) // 2)[..., None], F([0.6, 0.45, 0.35]), F([0.35, 0.5, 0.65]))
    sums = np.zeros((h, w, 4), np.float32)
    sums[..., :3] = (alb * S_TOTAL * (1.0 + rng.uniform(-0.5, 0.5, (h, w, 3)))).astype(np.float32)
    sums[..., 3] = 1.0
    aov = np.zeros((h, w, 8), np.float32)
    aov[..., :3] = alb * T_TOTAL
    aov[..., 3] = T_TOTAL
    nrm = np.where((ys < (h + 1) // 2)[..., None], F([0, 1, 0]), F([0, 0.6, 0.8]))
    aov[..., 4:7] = nrm * T_TOTAL
    aov[..., 7] = ((3.0 + 2.0 * xs / max(w - 1, 1)) * T_TOTAL).astype(np.float32)
    return sums, aov


def _spots(h, w, k):
    """k pixel positions spread over the image (distinct where it has room)."""
    idx = np.linspace(0, h * w - 1, k + 2)[1:-1].astype(np.int64)
    return [(int(i) // w, int(i) % w) for i in idx]


def _block(h, w):
    """A block of about a third of each side, in the middle (at least one pixel)."""
    y0, x0 = h // 3, w // 3
    return slice(y0, max(y0 + 1, 2 * h // 3)), slice(x0, max(x0 + 1, 2 * w // 3))


def _depth(aov, where, z):
    """Mean distance z at `where`, every sample a hit there (T_TOTAL a power of two: z * T / T == z)."""
    aov[where + (3,)] = T_TOTAL
    aov[where + (7,)] = F(z) * F(T_TOTAL)


def cases(h, w, seed=0):
    """Every named edge case on an h x w image."""
    out = []

    def add(name, fn):
        sums, aov = base(h, w, seed)
        fn(sums, aov)
        assert np.isfinite(sums).all() and np.isfinite(aov).all(), name
        out.append(Case(name, sums, aov, S_TOTAL, T_TOTAL))

    cy, cx = h // 2, w // 2
    by, bx = _block(h, w)
    # far depth: single pixels, a block, the whole frame
    for z in FAR_DEPTHS:
        add("far_pixel_%g" % z, lambda s, a, z=z: _depth(a, (cy, cx), z))
        add("far_block_%g" % z, lambda s, a, z=z: _depth(a, (by, bx), z))
        add("far_frame_%g" % z, lambda s, a, z=z: _depth(a, (slice(None), slice(None)), z))

    def far_mix(s, a):
        for (y, x), z in zip(_spots(h, w, len(FAR_DEPTHS)), FAR_DEPTHS):
            _depth(a, (y, x), z)
    add("far_mix", far_mix)

    # tiny depth and normals: means in binary16's subnormal range (below 6.1e-5), down to its smallest step 2^-24 and under it
    def tiny_depth(s, a):
        z = np.array([6.0e-5, 3.0e-5, 1.0e-6, 2.0 ** -24, 2.0 ** -25, 1.0e-9], np.float32)
        a[..., 7] = z[(np.arange(h)[:, None] + np.arange(w)[None, :]) % len(z)] * F(T_TOTAL)
    add("tiny_depth", tiny_depth)

    def tiny_normals(s, a):
        a[by, bx, 4:7] = F([1.0e-5, -3.0e-7, 2.0 ** -24]) * F(T_TOTAL)
        a[by, bx, 7] = F(1.0e-5) * F(T_TOTAL)
    add("tiny_normals", tiny_normals)

    # albedo
    add("albedo_zero", lambda s, a: a.__setitem__((Ellipsis, slice(0, 3)), 0.0))
    add("albedo_zero_channel", lambda s, a: a.__setitem__((by, bx, 1), 0.0))
    eps = denoise_ref.ALBEDO_EPS
    for tag, v in (("below", np.nextafter(eps, F(0))), ("at", eps), ("above", np.nextafter(eps, F(1)))):
        add("albedo_eps_" + tag, lambda s, a, v=v: a.__setitem__((by, bx, slice(0, 3)), F(v) * F(T_TOTAL)))

    def hits_mixed(s, a):
        hits = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % (T_TOTAL + 1)  # 0 .. T, 0 and T included
        a[..., 3] = hits
        a[..., :3] = a[..., :3] / F(T_TOTAL) * hits[..., None]
        a[..., 4:7] = a[..., 4:7] / F(T_TOTAL) * hits[..., None]
        a[..., 7] = a[..., 7] / F(T_TOTAL) * hits
    add("hits_mixed", hits_mixed)
    add("all_miss", lambda s, a: a.__setitem__(Ellipsis, 0.0))

    # radiance
    for v in (1e19, 1e30, 3e38):
        def firefly(s, a, v=v):
            for y, x in _spots(h, w, 3):
                s[y, x, :3] = F(v)
        add("firefly_%g" % v, firefly)

    def subnormal_radiance(s, a):
        s[by, bx, :3] = F([1.0e-39, 3.0e-39, 7.0e-40])
        s[cy, :, 0] = F(1.4e-45)  # the smallest f32 subnormal
    add("subnormal_radiance", subnormal_radiance)
    add("zero_radiance", lambda s, a: s.__setitem__((Ellipsis, slice(0, 3)), 0.0))
    return out


def moment_records(h, w, seed=0):
    """Temporal moment records (mu1, mu2, frames, scale) with frames 1 .. 6 (below and at RSRT_SV_MIN_FRAMES = 4, and above),
    mu2 both above and below mu1^2, and scale in (0, 1]."""
    rng = np.random.default_rng(seed)
    mu1 = rng.uniform(0, 2, (h, w))
    frames = 1 + np.arange(h * w).reshape(h, w) % 6
    m = np.stack([mu1, mu1 * mu1 + rng.normal(0.05, 0.1, (h, w)), frames, rng.uniform(0.05, 1, (h, w))], -1)
    return m.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- display and binary16 mean
DISPLAY_S = 7  # the display edges' sample total


def display_edges():
    """An accumulator for the display pass and the binary16 mean: test_display's edge pixels (negative, zero, f16 overflow, f16
    subnormal means, the overflow edge), a block of means straddling 65504 (the last finite binary16) and 65520 (the first that rounds
    to inf), and a block of means in binary16's subnormal range, on an ordinary picture.  -> sums [32, 48, 4] for DISPLAY_S samples."""
    S = F(DISPLAY_S)
    rng = np.random.default_rng(1)
    img = np.zeros((32, 48, 4), np.float32)
    img[..., :3] = (rng.uniform(0, 1, (32, 48, 3)) ** 4 * 40).astype(np.float32)
    img[..., 3] = 1.0
    img[0, 0, :3] = [-1, 2, 3]
    img[0, 1, :3] = [0, 0, 0]
    img[0, 2, :3] = [1e9, 1e9, 1e9]
    img[0, 3, :3] = [1e-7, 3e-6, 6e-5]
    img[0, 4, :3] = [65519.9 * 7, 65520 * 7, 65504 * 7]
    # means straddling the binary16 overflow: 65488 (the last step below), 65504, halfway to 65536 and one f32 ulp either side, beyond
    means = [65488.0, 65503.0, 65504.0, 65505.0, 65519.0, np.nextafter(F(65520), F(0)), 65520.0, np.nextafter(F(65520), F(1e9)),
             65536.0, 1e6, -65504.0, -65520.0]
    hi = np.array(means, np.float32)
    for k in range(3):
        img[4:8, 0:len(hi), k] = np.roll(hi, k)[None, :] * S
    # binary16 subnormal means: 2^-24 (the smallest), half of it (a tie to even: 0), 1.5 * 2^-24 (a tie: 2^-23), just below the
    # smallest normal 2^-14, and ordinary subnormals
    sub = np.array([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 3.0e-5, 1.0e-6, 6.0e-8, 2.9e-8, -1.0e-6, 0.0],
                   np.float32)
    for k in range(3):
        img[10:14, 0:len(sub), k] = np.roll(sub, k)[None, :] * S
    return img


# ---------------------------------------------------------------------------------------------------- far geometry
SCENE_SCALE = 2.0 ** 15  # exact in f32: default.toml's spheres, about 4 units from its camera, end up about 1.3e5 units away


def scaled_default_scene(out_dir, k=SCENE_SCALE):
    """default.toml with every position, radius, plane vector, the camera position and the mesh's vertices multiplied by k, written
    into out_dir (scenes/default.toml and the cube.obj it names as ../cube.obj).  -> the scene's path."""
    num = re.compile(r"-?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?")
    os.makedirs(os.path.join(out_dir, "scenes"), exist_ok=True)
    lines = []
    for ln in open(util.scene_path("default")):
        key = ln.split("=")[0].strip()
        if key in ("pos", "radius", "forward", "right"):
            head, tail = ln.split("=", 1)
            ln = head + "=" + num.sub(lambda m: repr(float(m.group()) * k), tail)
        lines.append(ln)
    path = os.path.join(out_dir, "scenes", "default.toml")
    open(path, "w").write("".join(lines))
    obj = []
    for ln in open(os.path.join(util.ASSETS, "cube.obj")):
        if ln.startswith("v "):
            ln = "v " + " ".join(repr(float(x) * k) for x in ln.split()[1:]) + "\n"
        obj.append(ln)
    open(os.path.join(out_dir, "cube.obj"), "w").write("".join(obj))
    return path
