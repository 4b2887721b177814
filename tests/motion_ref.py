"""numpy float32 restatement of the camera motion blur pass (include/rsrt_motion.h, rsrt_motion_blur) for the tests.  Every step is one
IEEE binary32 operation in the order the header documents it (the centre ray and the projection through temporal_ref), so the results
are compared bit for bit.  The tap loop is vectorised over the pixels and looped over the taps in the published order."""
import numpy as np

import temporal_ref
from rsoderh_raytracing_amd import types as T

F = np.float32
TILE = 16
MAX_RADIUS = 16
MAX_TAPS = 32
DEPTH_EXTENT = F(0.05)
DEFAULTS = {"shutter": 0.5, "max_radius": 16, "taps": 16, "flags": 0}  # the header's documented defaults
Camera = temporal_ref.Camera


def params_ok(shutter, max_radius, taps, flags):
    with np.errstate(all="ignore"):
        s = F(shutter)
    return bool(np.isfinite(s) and 0 <= s <= 1 and 1 <= max_radius <= MAX_RADIUS and 2 <= taps <= MAX_TAPS and taps % 2 == 0 and flags == 0)


def camera_record(cam):
    """The rsrt_camera record (State.camera) of a temporal_ref.Camera."""
    rec = np.zeros(1, T.CAMERA)
    rec["pos"][0] = cam.pos
    rec["rot_transform"][0][:, :3] = cam.rot
    rec["fov_y"][0] = cam.fov_y
    return rec


def velocity(rec, cam, prev, shutter, max_radius):
    """(u [h, w, 2], l [h, w], z [h, w]) from the records [h, w, 8], the camera and the camera one frame earlier."""
    rec = np.asarray(rec, F)
    h, w = rec.shape[:2]
    surface = rec[..., 3] > 0
    with np.errstate(all="ignore"):
        zz = np.where(surface, rec[..., 7] / rec[..., 3], F(np.inf)).astype(F)
    z = np.where(np.isnan(zz), F(np.inf), zz).astype(F)
    u = np.zeros((h, w, 2), F)
    l = np.zeros((h, w), F)
    if cam.same(prev):
        return u, l, z
    y, x = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        d = temporal_ref.center_ray(cam, w, h, x, y)
        X = cam.pos + zz[..., None] * d
        e = np.where(surface[..., None], X - prev.pos, d).astype(F)
        fx, fy, front = temporal_ref.project(prev, w, h, e)
        hs = F(0.5) * F(shutter)
        vx, vy = (x.astype(F) - fx) * hs, (y.astype(F) - fy) * hs
        ok = front & np.isfinite(vx) & np.isfinite(vy)
        vx, vy = np.where(ok, vx, F(0)), np.where(ok, vy, F(0))
        ln = np.sqrt(vx * vx + vy * vy)
        ok = ok & np.isfinite(ln)
        R = F(max_radius)
        over = ok & (ln > R)
        s = R / ln
        vx, vy, ln = np.where(over, vx * s, vx), np.where(over, vy * s, vy), np.where(over, R, ln)
    u[..., 0] = np.where(ok, vx, F(0))
    u[..., 1] = np.where(ok, vy, F(0))
    l = np.where(ok, ln, F(0)).astype(F)
    return u, l, z


def prepare(sums, total, rec, cam, prev, shutter, max_radius):
    """The prepared texels [h, w, 7]: (sum.rgb / total, l, z, ux, uy)."""
    with np.errstate(all="ignore"):
        c = np.asarray(sums, F)[..., :3] / F(total)
    u, l, z = velocity(rec, cam, prev, shutter, max_radius)
    return np.concatenate([c, l[..., None], z[..., None], u], axis=-1).astype(F)


def tiles_of(n):
    return (n + TILE - 1) // TILE


def tile_max(prep):
    """Every tile's dominant velocity [tiles_y, tiles_x, 3] (ux, uy, l): the first texel in row-major order with the greatest l."""
    prep = np.asarray(prep, F)
    h, w = prep.shape[:2]
    out = np.zeros((tiles_of(h), tiles_of(w), 3), F)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            t = prep[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1, 7)
            i = int(np.argmax(t[:, 3]))  # (the first of equal maxima)
            if t[i, 3] > 0:
                out[ty, tx] = (t[i, 5], t[i, 6], t[i, 3])
    return out


def neighbour_max(tiles):
    """Every tile's neighbour maximum [tiles_y, tiles_x, 3]: the first of its 3 x 3 tiles, in row-major order, with the greatest l."""
    tiles = np.asarray(tiles, F)
    ny, nx = tiles.shape[:2]
    out = np.zeros_like(tiles)
    for ty in range(ny):
        for tx in range(nx):
            t = tiles[max(ty - 1, 0):ty + 2, max(tx - 1, 0):tx + 2].reshape(-1, 3)
            out[ty, tx] = t[int(np.argmax(t[:, 2]))]
    return out


def tap_at(n, i, taps):
    """Tap i of `taps` along the neighbour maxima n [..., 3]: integer offsets ox, oy and the distance."""
    t = F(2 * i + 1) / F(taps) - F(1.0)
    ox = np.floor(t * n[..., 0] + F(0.5)).astype(np.int64)
    oy = np.floor(t * n[..., 1] + F(0.5)).astype(np.int64)
    return ox, oy, np.abs(t) * n[..., 2]


def cone(d, spread):
    return np.minimum(np.maximum(F(1.0) - d / spread, F(0.0)), F(1.0))


def foreground(z_p, z_q):
    with np.errstate(all="ignore"):
        f = F(0.5) + (z_p - z_q) / (DEPTH_EXTENT * np.where(z_p < z_q, z_p, z_q))
    f = np.where(f > 0, np.where(f > 1, F(1.0), f), F(0.0))
    return np.where(z_q == z_p, F(0.5), f).astype(F)


def gather(prep, taps, nmax=None, order=None):
    """The motion image of prepared texels [h, w, 7] -> [h, w, 4] (rgb, 1).  nmax: the neighbour maxima (default: the prepared
    texels' own); order: the taps' order (default the published one, 0 .. taps - 1)."""
    prep = np.asarray(prep, F)
    h, w = prep.shape[:2]
    if nmax is None:
        nmax = neighbour_max(tile_max(prep))
    y, x = np.mgrid[0:h, 0:w]
    n = nmax[y // TILE, x // TILE]  # [h, w, 3]
    blur = n[..., 2] >= F(0.5)
    c_p, l_p, z_p = prep[..., :3], prep[..., 3], prep[..., 4]
    s_p = np.maximum(l_p, F(0.5))
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = F(-0.0)
    fn = F(taps)
    with np.errstate(all="ignore"):
        for i in (range(taps) if order is None else order):
            ox, oy, dist = tap_at(n, i, taps)
            qx, qy = x + ox, y + oy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            q = prep[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
            f = foreground(z_p, q[..., 4])
            b = F(1.0) - f
            wgt = f * cone(dist, np.maximum(q[..., 3], F(0.5))) + b * cone(dist, s_p)
            use = inside & (wgt != 0)
            acc[..., :3] = np.where(use[..., None], acc[..., :3] + wgt[..., None] * q[..., :3], acc[..., :3])
            acc[..., 3] = np.where(use, acc[..., 3] + wgt, acc[..., 3])
        rest = F(1.0) - acc[..., 3] / fn
        out = acc[..., :3] / fn + rest[..., None] * c_p
    out = np.where(blur[..., None], out, c_p)
    return np.concatenate([out, np.ones((h, w, 1), F)], axis=-1).astype(F)


def motion(sums, total, rec, cam, prev, shutter=DEFAULTS["shutter"], max_radius=DEFAULTS["max_radius"], taps=DEFAULTS["taps"]):
    """One rsrt_motion_blur: (motion image [h, w, 4], velocities [h, w, 3] (ux, uy, l), tile maxima [tiles_y, tiles_x, 3])."""
    p = prepare(sums, total, rec, cam, prev, shutter, max_radius)
    t = tile_max(p)
    uvl = np.concatenate([p[..., 5:7], p[..., 3:4]], axis=-1)
    return gather(p, taps, neighbour_max(t)), uvl, t


def default_camera():
    """A camera that looks a little off every axis (pos, rot with rot[j] = column j: the camera's right, up and backward axes)."""
    yaw, pitch = 0.3, -0.2
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Camera([0.5, 1.0, -2.0], m.T.astype(F), 0.9)


def earlier(cam, yaw=0.0, dolly=0.0, truck=0.0):
    """The camera one frame before `cam`: turned back by `yaw` (radians) about the world's up axis (+y) and moved back by `dolly`
    along cam's forward axis and by `truck` along its right axis."""
    c, s = np.cos(-yaw), np.sin(-yaw)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    rot = (ry @ cam.rot.astype(np.float64).T).T.astype(F)
    pos = cam.pos.astype(np.float64) - dolly * (-cam.rot[2].astype(np.float64)) - truck * cam.rot[0].astype(np.float64)
    return Camera(pos.astype(F), rot if yaw else cam.rot, cam.fov_y)


def camera_pair(yaw=0.015, dolly=-0.02, truck=0.05):
    """(cur, prev): yaw plus translation.  The camera moved sideways and BACKWARDS, so a point nearer than 0.02 lies behind prev."""
    cur = default_camera()
    return cur, earlier(cur, yaw, dolly, truck)


def records_at_distance(dist, hits=1):
    """Records [h, w, 8] with `hits` hits each at ray distance dist [h, w]; inf: no hit."""
    dist = np.asarray(dist, F)
    rec = np.zeros(dist.shape + (8,), F)
    hit = np.isfinite(dist)
    n = np.broadcast_to(np.asarray(hits, F), dist.shape)
    with np.errstate(all="ignore"):
        rec[..., 3] = np.where(hit, n, F(0))
        rec[..., 7] = np.where(hit, dist * n, F(0))
    rec[..., :3] = 0.5 * rec[..., 3:4]
    rec[..., 6] = rec[..., 3]
    return rec


def synthetic(h, w, seed, yaw=0.015, dolly=-0.02, truck=0.05):
    """A frame for the pass: (sums [h, w, 4], records [h, w, 8], cur, prev, {name: flat pixel index}).  Lognormal radiance to be read
    with total 1 or 3.  The left part of the frame (two tile columns where there are three, else half) is slow: far surfaces (40 .. 80)
    and sky, which the pair's small yaw moves by less than half a pixel at these sizes.  The rest is fast: blocks of near (0.3 .. 1) and
    far surfaces, sky pixels sprinkled over them.  Where the frame has room (h w >= 16) single pixels of the fast part hold a depth of
    0, a point behind the previous camera (nearer than the camera moved back), a point just in front of it (a velocity far over the
    clamp), a far and a near surface and a distance without a hit (sky), and two pixels anywhere an inf and a NaN colour.  The
    returned dict names where each was placed."""
    rng = np.random.default_rng(seed)
    cur, prev = camera_pair(yaw, dolly, truck)
    sums = np.ones((h, w, 4), F)
    sums[..., :3] = np.exp(rng.normal(-1.0, 1.0, (h, w, 3))).astype(F)
    by, bx = np.mgrid[0:h, 0:w]
    fast = bx >= (2 * TILE if w >= 3 * TILE else w // 2)
    far = np.exp(rng.uniform(np.log(40.0), np.log(80.0), (h, w)))
    near = np.exp(rng.uniform(np.log(0.3), np.log(1.0), (h, w)))
    dist = np.where(fast & ((by // 4 + bx // 4) % 2 == 0), near, far).astype(F)
    dist[rng.random((h, w)) < 0.15] = np.inf
    dist[(by // TILE + bx // TILE) % 4 == 3] = np.inf  # whole sky blocks too
    hits = rng.choice([1, 1, 2, 5], size=(h, w)).astype(F)
    rec = records_at_distance(dist, hits)
    placed = {}
    flat, fs = rec.reshape(-1, 8), sums.reshape(-1, 4)
    if h * w >= 16:
        odd = rng.choice(np.flatnonzero(fast.reshape(-1)), size=6, replace=False)
        flat[odd[0], 3], flat[odd[0], 7] = 2, 0.0      # depth 0
        flat[odd[1], 3], flat[odd[1], 7] = 1, 0.001    # behind the previous camera
        flat[odd[2], 3], flat[odd[2], 7] = 1, 0.03     # just in front of it: far over the clamp
        flat[odd[3], 3], flat[odd[3], 7] = 1, 60.0     # a far surface,
        flat[odd[4], 3], flat[odd[4], 7] = 2, 1.0      # a near one (depth 0.5)
        flat[odd[5], 3], flat[odd[5], 7] = 0, 5.0      # and a distance without a hit: sky
        col = rng.choice(h * w, size=2, replace=False)
        fs[col[0], 0] = np.inf
        fs[col[1], 1] = np.nan
        placed = {"zero_depth": int(odd[0]), "behind": int(odd[1]), "over_clamp": int(odd[2]), "far": int(odd[3]), "near": int(odd[4]),
                  "sky": int(odd[5]), "inf_colour": int(col[0]), "nan_colour": int(col[1])}
    return sums, rec, cur, prev, placed


def contains(sums, rec, cur, prev, placed, shutter, max_radius):
    """Which of the listed cases the frame really holds under these parameters: {name: bool}."""
    rec = np.asarray(rec, F)
    h, w = rec.shape[:2]
    u, l, z = velocity(rec, cur, prev, shutter, max_radius)
    y, x = np.mgrid[0:h, 0:w]
    d = temporal_ref.center_ray(cur, w, h, x, y)
    surface = rec[..., 3] > 0
    with np.errstate(all="ignore"):
        e = np.where(surface[..., None], cur.pos + z[..., None] * d - prev.pos, d).astype(F)
    _, _, front = temporal_ref.project(prev, w, h, e)
    at = lambda a, k: a.reshape(-1)[placed[k]]  # noqa: E731
    c = np.asarray(sums, F)[..., :3]
    return {"sky": bool(np.isinf(at(z, "sky"))), "near": bool(at(z, "near") < 2), "far": bool(at(z, "far") > 30),
            "zero_depth": bool(at(z, "zero_depth") == 0), "behind": bool(not at(front, "behind") and at(l, "behind") == 0),
            "over_clamp": bool(at(l, "over_clamp") == F(max_radius)), "under_half": bool(((l > 0) & (l < 0.5)).any()),
            "inf_colour": bool(np.isinf(c).any()), "nan_colour": bool(np.isnan(c).any())}
