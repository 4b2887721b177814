"""numpy float32 restatement of the temporal pass (include/rsrt_temporal.h, rsrt_temporal_accumulate) for the tests.  Every step is one
IEEE binary32 operation in the order the C code performs it (the centre ray's fused operations through denoise_ref.fma32), so the
results are compared bit for bit.  Per pixel it also returns what happened there, as the header's RSRT_TP_* code."""
import numpy as np

import oracle
from denoise_ref import fma32

F = np.float32
MIN_WEIGHT = F(0.01)
DEFAULTS = {"max_history": 32, "depth_tolerance": 0.05, "normal_tolerance": 0.9}  # the header's documented defaults

FIRST, IDENTITY, REPROJECTED, SKY, BEHIND, OUT_OF_VIEW, PLANE_REJECTED, NORMAL_REJECTED, LOW_WEIGHT = range(9)
CODE_NAMES = ["first", "identity", "reprojected", "sky", "behind", "out_of_view", "plane_rejected", "normal_rejected", "low_weight"]


class Camera:
    """pos (3,), rot: rot_transform's 3x3 with rot[j] = column j, fov_y; m = rsrt_sinf(fov_y / 2).  From an rsrt_camera record (the
    State's camera) or from the parts."""

    def __init__(self, pos, rot, fov_y):
        self.pos = np.asarray(pos, np.float32).reshape(3).copy()
        self.rot = np.asarray(rot, np.float32).reshape(3, -1)[:, :3].copy()
        self.fov_y = F(np.asarray(fov_y, np.float32).reshape(-1)[0])
        self.m = F(oracle.detmath("sin", float(self.fov_y / F(2.0))))

    @classmethod
    def from_record(cls, cam):
        cam = np.asarray(cam).reshape(-1)[0]
        return cls(cam["pos"], cam["rot_transform"], cam["fov_y"])

    def same(self, o):
        return (self.pos.view(np.uint32) == o.pos.view(np.uint32)).all() and (self.rot.view(np.uint32) == o.rot.view(np.uint32)).all() \
            and self.fov_y.view(np.uint32) == o.fov_y.view(np.uint32)


def center_ray(cam, w, h, x, y):
    """start_path's camera ray of pixels (x, y) with zero jitter: [..., 3]."""
    fx, fy = np.asarray(x).astype(np.float32), np.asarray(y).astype(np.float32)
    sx = ((fx / F(w)) * F(2.0) - F(1.0)) * F(1.0)
    sy = ((fy / F(h)) * F(2.0) - F(1.0)) * F(-1.0)
    aspect = F(w) / F(h)
    v = [(sx * cam.m) * aspect, sy * cam.m, np.full(sx.shape, F(-1.0))]
    r = cam.rot
    a = [fma32(r[2, i], v[2], fma32(r[1, i], v[1], r[0, i] * v[0])) for i in range(3)]
    inv = F(1.0) / np.sqrt(fma32(a[2], a[2], fma32(a[1], a[1], a[0] * a[0])))
    return np.stack([a[0] * inv, a[1] * inv, a[2] * inv], axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def project(cam, w, h, e):
    """e [..., 3] into camera cam: fx, fy and whether it lies in front."""
    r = cam.rot
    vx, vy, vz = (dot(r[k], e) for k in range(3))
    depth = -vz
    front = depth > 0
    with np.errstate(all="ignore"):
        aspect = F(w) / F(h)
        sx = vx / ((depth * cam.m) * aspect)
        sy = vy / (depth * cam.m)
        fx = ((sx + F(1.0)) * F(0.5)) * F(w)
        fy = ((F(1.0) - sy) * F(0.5)) * F(h)
    return fx, fy, front


def current(sums, aov, S, T):
    """c [H, W, 3], features [H, W, 4] and the surface mask of the current frame."""
    c = np.asarray(sums, np.float32)[..., :3] / F(S)
    aov = np.asarray(aov, np.float32)
    surface = F(2.0) * aov[..., 3] >= F(T)
    with np.errstate(all="ignore"):
        f = aov[..., 4:8] / aov[..., 3:4]
    f = np.where(surface[..., None], f, np.float32([0, 0, 0, -1]))
    return c, f, surface


def temporal(sums, aov, S, T, cam, prev_cam, prev_col, prev_feat, max_history=32, depth_tolerance=0.05, normal_tolerance=0.9):
    """One rsrt_temporal_accumulate: sums [H, W, 4] (the accumulator), aov [H, W, 8], cameras (Camera; prev_cam None: first frame),
    the previous history [H, W, 4] and features [H, W, 4] -> (history [H, W, 4], features [H, W, 4], codes [H, W])."""
    H, W = np.asarray(sums).shape[:2]
    c, f, surface = current(sums, aov, S, T)
    Sf = F(S)
    h = np.zeros((H, W, 3), np.float32)
    nh = np.zeros((H, W), np.float32)
    code = np.full((H, W), FIRST, np.int32)
    if prev_cam is not None and cam.same(prev_cam):
        h, nh = prev_col[..., :3].astype(np.float32), prev_col[..., 3].astype(np.float32)
        code[:] = IDENTITY
    elif prev_cam is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        d = center_ray(cam, W, H, xs, ys)
        X = cam.pos + f[..., 3:4] * d
        e = np.where(surface[..., None], X - prev_cam.pos, d)
        fx, fy, front = project(prev_cam, W, H, e)
        inview = (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
        go = front & inview
        fx, fy = np.where(go, fx, F(0)), np.where(go, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = fx - flx, fy - fly
        one = F(1.0)
        tw = [(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]
        tol = F(depth_tolerance) * f[..., 3]
        wsum = np.zeros((H, W), np.float32)
        acc = np.zeros((H, W, 4), np.float32)
        plane_rej = np.zeros((H, W), bool)
        normal_rej = np.zeros((H, W), bool)
        pc = np.asarray(prev_col, np.float32)
        pf = np.asarray(prev_feat, np.float32)
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inside = go & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            hq, fq = pc[cy, cx], pf[cy, cx]
            ok = inside & (hq[..., 3] > 0) & ((fq[..., 3] >= 0) == surface)
            dq = center_ray(prev_cam, W, H, cx, cy)
            eq = (prev_cam.pos + fq[..., 3:4] * dq) - X
            with np.errstate(all="ignore"):
                pd = dot(f, eq)
                pfail = surface & ~(np.abs(pd) <= tol)
                nfail = surface & ~pfail & ~(dot(f, fq) >= F(normal_tolerance))
            plane_rej |= ok & pfail
            normal_rej |= ok & nfail
            ok &= ~pfail & ~nfail
            wsum = np.where(ok, wsum + tw[t], wsum)
            acc = np.where(ok[..., None], acc + tw[t][..., None] * hq, acc)
        hist = go & (wsum >= MIN_WEIGHT)
        with np.errstate(all="ignore"):
            hh = acc[..., :3] / wsum[..., None]
            nn = acc[..., 3] / wsum
        nn = np.where(nn > F(max_history), F(max_history), nn)
        h = np.where(hist[..., None], hh, F(0))
        nh = np.where(hist, nn, F(0))
        code = np.where(~front, BEHIND, np.where(~inview, OUT_OF_VIEW, np.where(
            hist, np.where(surface, REPROJECTED, SKY),
            np.where(plane_rej, PLANE_REJECTED, np.where(normal_rej, NORMAL_REJECTED, LOW_WEIGHT))))).astype(np.int32)
    used = (code == IDENTITY) | (code == REPROJECTED) | (code == SKY)
    with np.errstate(all="ignore"):
        blend = (h * nh[..., None] + c * Sf) / (nh + Sf)[..., None]
    out = np.empty((H, W, 4), np.float32)
    out[..., :3] = np.where(used[..., None], blend, c)
    out[..., 3] = np.where(used, nh + Sf, Sf)
    return out, f.astype(np.float32), code


class Sequence:
    """The pass's state over frames, as the library keeps it: the last history, features and camera (reset: none)."""

    def __init__(self, **params):
        self.params = params
        self.reset()

    def reset(self):
        self.cam = self.col = self.feat = None

    def frame(self, sums, aov, S, T, cam):
        out, f, code = temporal(sums, aov, S, T, cam, self.cam, self.col, self.feat, **self.params)
        self.cam, self.col, self.feat = cam, out, f
        return out, code
