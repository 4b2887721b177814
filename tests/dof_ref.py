"""numpy float32 restatement of the depth-of-field pass (include/rsrt_dof.h, rsrt_dof) for the tests.  Every step is one IEEE binary32
operation in the order the header documents it (the centre ray through temporal_ref, which restates its fused operations), so the
results are compared bit for bit.  The tap loop is vectorised over the pixels and looped over the taps in the published order."""
import numpy as np

import temporal_ref
from rsoderh_raytracing_amd import types as T

F = np.float32
MAX_RADIUS = 16
DEFAULTS = {"focus_distance": 1.0, "aperture": 0.01, "max_radius": 8, "flags": 0}  # the header's documented defaults
Camera = temporal_ref.Camera


def dist_table():
    """D[dy + 16, dx + 16]: the correctly rounded f32 sqrt(dx^2 + dy^2) (IEEE sqrt of an exactly represented integer)."""
    d = np.arange(-MAX_RADIUS, MAX_RADIUS + 1)
    return np.sqrt((d[:, None] ** 2 + d[None, :] ** 2).astype(F))


def params_ok(focus_distance, aperture, max_radius, flags):
    with np.errstate(all="ignore"):
        f, a = F(focus_distance), F(aperture)
    return bool(np.isfinite(f) and f > 0 and np.isfinite(a) and a >= 0 and 1 <= max_radius <= MAX_RADIUS and flags == 0)


def camera_record(cam):
    """The rsrt_camera record (State.camera) of a temporal_ref.Camera."""
    rec = np.zeros(1, T.CAMERA)
    rec["pos"][0] = cam.pos
    rec["rot_transform"][0][:, :3] = cam.rot
    rec["fov_y"][0] = cam.fov_y
    return rec


def depth(rec, cam):
    """z [h, w] along the optical axis from the records [h, w, 8]; +inf where there is no hit."""
    rec = np.asarray(rec, F)
    h, w = rec.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    c = temporal_ref.dot(temporal_ref.center_ray(cam, w, h, x, y), -cam.rot[2])
    with np.errstate(all="ignore"):
        z = (rec[..., 7] / rec[..., 3]) * c
    return np.where(rec[..., 3] > 0, z, F(np.inf)).astype(F)


def coc(rec, cam, focus_distance, aperture, max_radius):
    """The signed blur radius r [h, w], in pixels."""
    rec = np.asarray(rec, F)
    A, R = F(aperture) * F(rec.shape[0]), F(max_radius)
    with np.errstate(all="ignore"):
        t = F(focus_distance) / depth(rec, cam)
        r = A * (F(1.0) - t)
    r = np.where(rec[..., 3] > 0, r, A)
    r = np.where(r < -R, -R, np.where(r > R, R, r))
    return np.where(np.isnan(r), F(0.0), r).astype(F)


def prepare(sums, total, rec, cam, focus_distance, aperture, max_radius):
    """The prepared texels [h, w, 4]: (sum.rgb / total, r)."""
    with np.errstate(all="ignore"):
        c = np.asarray(sums, F)[..., :3] / F(total)
    return np.concatenate([c, coc(rec, cam, focus_distance, aperture, max_radius)[..., None]], axis=-1).astype(F)


def gather(prep, max_radius):
    """The lens blur of prepared texels [h, w, 4] -> [h, w, 4] (rgb, 1)."""
    prep = np.asarray(prep, F)
    h, w = prep.shape[:2]
    R, D = int(max_radius), dist_table()
    pad = np.zeros((h + 2 * R, w + 2 * R, 4), F)
    pad[R:R + h, R:R + w] = prep
    inside = np.zeros((h + 2 * R, w + 2 * R), bool)
    inside[R:R + h, R:R + w] = True
    r_p = prep[..., 3]
    abs_p = np.abs(r_p)
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = F(-0.0)  # (-0) + x == x for every x: the first term is added exactly
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                q = pad[R + dy:R + dy + h, R + dx:R + dx + w]
                r_q = q[..., 3]
                a = np.abs(r_q)
                a = np.where(r_q > r_p, np.minimum(a, abs_p), a)
                a = np.maximum(a, F(0.5))
                k = (a + F(0.5)) - D[dy + MAX_RADIUS, dx + MAX_RADIUS]
                k = np.minimum(np.maximum(k, F(0.0)), F(1.0))
                wgt = k * (F(0.25) / (a * a))
                use = inside[R + dy:R + dy + h, R + dx:R + dx + w] & (k != 0)  # skipped, not added as zero
                if not use.any():
                    continue
                acc[..., :3] = np.where(use[..., None], acc[..., :3] + wgt[..., None] * q[..., :3], acc[..., :3])
                acc[..., 3] = np.where(use, acc[..., 3] + wgt, acc[..., 3])
        out = acc[..., :3] / acc[..., 3:4]
    return np.concatenate([out, np.ones((h, w, 1), F)], axis=-1).astype(F)


def dof(sums, total, rec, cam, focus_distance=DEFAULTS["focus_distance"], aperture=DEFAULTS["aperture"], max_radius=DEFAULTS["max_radius"]):
    """One rsrt_dof: (lens image [h, w, 4], r [h, w])."""
    p = prepare(sums, total, rec, cam, focus_distance, aperture, max_radius)
    return gather(p, max_radius), p[..., 3]


def records_at_depth(z, cam, hits=1):
    """Records [h, w, 8] whose depth() is about z [h, w] (exactly, where the division by the cosine is exact): `hits` hits each at the
    distance z / cosine; z = inf: no hit."""
    z = np.asarray(z, F)
    h, w = z.shape
    y, x = np.mgrid[0:h, 0:w]
    c = temporal_ref.dot(temporal_ref.center_ray(cam, w, h, x, y), -cam.rot[2])
    rec = np.zeros((h, w, 8), F)
    hit = np.isfinite(z)
    n = np.broadcast_to(np.asarray(hits, F), z.shape)
    with np.errstate(all="ignore"):
        rec[..., 3] = np.where(hit, n, F(0))
        rec[..., 7] = np.where(hit, (z / c) * n, F(0))
    rec[..., :3] = 0.5 * rec[..., 3:4]
    rec[..., 6] = rec[..., 3]
    return rec


def default_camera():
    """A camera that looks a little off every axis (pos, rot with rot[j] = column j, fov_y)."""
    yaw, pitch = 0.3, -0.2
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Camera([0.5, 1.0, -2.0], m.T.astype(F), 0.9)


def synthetic(h, w, seed, focus_distance=2.0, tile=16):
    """A frame for the pass: (sums [h, w, 4], records [h, w, 8], camera, {name: flat pixel index}).  The sums are bloom_ref.synthetic's
    (lognormal radiance, bright dots, and where the frame has room NaN, +-inf, negative, -0, denormal and huge pixels), to be read with
    total 1 or 3.  The records have 0, 1 or several hits a pixel and depths from a quarter of focus_distance to eight times it, in
    blocks of `tile` pixels of which every third lies on the focus plane (depth = focus_distance where the cosine divides exactly,
    else within a few ulp: |r| far below 0.5), so that whole tiles are in focus next to tiles that are not; a few pixels have depth
    0 and a few a negative distance."""
    import bloom_ref
    sums, special = bloom_ref.synthetic(h, w, seed)
    rng = np.random.default_rng(seed + 77)
    cam = default_camera()
    z = (F(focus_distance) * np.exp(rng.uniform(np.log(0.25), np.log(8.0), (h, w)))).astype(F)
    by, bx = np.mgrid[0:h, 0:w]
    block = (by // tile) * 5 + (bx // tile)
    z[block % 3 == 1] = F(focus_distance)
    hits = rng.choice([1, 1, 2, 5], size=(h, w)).astype(F)
    sky = rng.random((h, w)) < 0.15
    sky[block % 3 == 1] = False
    if h * w >= 16:
        sky[block % 7 == 3] = True  # whole sky blocks too
    z[sky] = np.inf
    rec = records_at_depth(z, cam, hits)
    flat = rec.reshape(-1, 8)
    n = h * w
    if n >= 16:
        odd = rng.choice(n, size=3, replace=False)
        flat[odd[0], 3], flat[odd[0], 7] = 2, 0.0   # depth 0: -R through the clamp
        flat[odd[1], 3], flat[odd[1], 7] = 1, -3.0  # a negative distance: behind everything
        flat[odd[2], 3], flat[odd[2], 7] = 0, 5.0   # a distance without a hit: sky
    return sums, rec, cam, special
