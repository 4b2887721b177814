"""The volumetric fog pass (include/rsrt_fog.h, rsrt_fog_render, rsrt_fog_apply) restated in numpy: the constants rsrt_fog_prepare makes
of a parameter set, the phase term, the march and the per-sample sum, the compose step and the sun of a sky as the fog's light, in
float32, operation for operation and in the header's order.  The camera rays are denoise_ref.camera_rays', the hits and the shadow
queries the checker's (oracle.cast_rays mode 0 and mode 1).  The CPU evaluation of the header (tests/test_fog.py, tests/cpp/fog_host.cpp)
and the HIP kernels (tests/test_fog_gpu.py) equal it bit for bit."""
import ctypes as C

import numpy as np

import denoise_ref
import oracle
import sky_ref

F = np.float32
JITTER = 1
MAX_STEPS = 64
MAX_DENSITY = F(1.0e6)
MAX_ANISOTROPY = F(0.95)
UNIT_TOLERANCE = F(1.0e-3)
LARGEST = np.finfo(F).max
HEADROOM = F(0.99)
LOG2E = sky_ref.LOG2E
PIF = sky_ref.PIF
DEFAULTS = {"density": 0.05, "albedo": (1.0, 1.0, 1.0), "anisotropy": 0.6, "light_dir": (0.0, 1.0, 0.0), "light_irradiance": (1.0, 1.0, 1.0),
            "ambient": (0.0, 0.0, 0.0), "max_distance": 50.0, "steps": 16, "flags": JITTER}
FIELDS = ("density", "albedo", "anisotropy", "light_dir", "light_irradiance", "ambient", "max_distance", "steps", "flags")
# the order of rsrt_fog_constants' 17 floats and 2 words
CONSTANTS = (("sigma2", 1), ("sigma_s", 3), ("s_amb", 3), ("phase_norm", 1), ("one_gg", 1), ("two_g", 1), ("light_dir", 3), ("light_irradiance", 3),
             ("max_distance", 1))


def params(**kw):
    """DEFAULTS with `kw` over them, every float rounded to float32; the vectors are one number for all channels or three."""
    assert set(kw) <= set(FIELDS), kw
    p = dict(DEFAULTS, **kw)
    for n in ("albedo", "light_dir", "light_irradiance", "ambient"):
        p[n] = tuple(float(x) for x in np.broadcast_to(np.asarray(p[n], F), (3,)))
    for n in ("density", "anisotropy", "max_distance"):
        p[n] = float(F(p[n]))
    return p


def unit(v):
    """A float32 unit vector along v (normalised in float64, then rounded: well within the accepted length)."""
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in (v / np.sqrt((v * v).sum())).astype(F))


def source_bound(p):
    """rsrt_fog_source_bound: S, which no channel's S_sun + S_amb exceeds."""
    with np.errstate(all="ignore"):
        g = F(p["anisotropy"])
        two_a = F(F(2) * (-g if g < F(0) else g))
        q_lo = F(F(F(F(1) + F(g * g)) - two_a) - F(two_a * UNIT_TOLERANCE))
        phase_hi = F(F(F(F(1) - F(g * g)) / F(F(4) * PIF)) / F(q_lo * np.sqrt(q_lo)))
        s = F(F(p["density"]) * max3(p["albedo"]))
        return F(F(F(s * phase_hi) * max3(p["light_irradiance"])) + F(s * max3(p["ambient"])))


def max3(v):
    """rsrt_fog_max3."""
    v = np.asarray(v, F)
    m = v[0] if v[0] > v[1] else v[1]
    return m if m > v[2] else v[2]


def length_bound(p):
    """rsrt_fog_length_bound: W_hi, which delta times the sum of a march's transmittances does not exceed."""
    with np.errstate(all="ignore"):
        den, dist = F(p["density"]), F(p["max_distance"])
        delta_hi = F(dist / F(p["steps"]))
        w = F(delta_hi + F(F(1) / F(den + F(F(den * den) * F(F(0.5) * delta_hi)))))
        return w if w < dist else dist


def sample_finite(p):
    """rsrt_fog_sample_finite."""
    with np.errstate(all="ignore"):
        S, limit = source_bound(p), F(HEADROOM * LARGEST)
        return bool(F(F(p["steps"]) * S) <= limit and F(S * length_bound(p)) <= limit)


def params_ok(p):
    """rsrt_fog_params_ok."""
    with np.errstate(all="ignore"):
        amount = lambda v: bool(F(0) <= F(v) <= LARGEST)  # noqa: E731
        d = np.asarray(p["light_dir"], F)
        off = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])) - F(1)
        den, dist, g = F(p["density"]), F(p["max_distance"]), F(p["anisotropy"])
        return bool(F(0) <= den <= MAX_DENSITY and all(F(0) <= F(a) <= F(1) for a in p["albedo"]) and -MAX_ANISOTROPY <= g <= MAX_ANISOTROPY and
                    -UNIT_TOLERANCE <= off <= UNIT_TOLERANCE and all(amount(v) for v in p["light_irradiance"]) and all(amount(v) for v in p["ambient"]) and
                    F(0) < dist <= LARGEST and F(F(den * LOG2E) * dist) <= F(F(0.5) * LARGEST) and 1 <= p["steps"] <= MAX_STEPS and
                    (p["flags"] & ~JITTER) == 0 and sample_finite(p))


def prepare(p):
    """rsrt_fog_prepare: a dict of float32 arrays and scalars named as rsrt_fog_constants' fields."""
    den, g = F(p["density"]), F(p["anisotropy"])
    k = {"sigma2": F(den * LOG2E)}
    k["sigma_s"] = (den * np.asarray(p["albedo"], F)).astype(F)
    k["s_amb"] = (k["sigma_s"] * np.asarray(p["ambient"], F)).astype(F)
    k["phase_norm"] = F(F(F(1) - F(g * g)) / F(F(4) * PIF))
    k["one_gg"] = F(F(1) + F(g * g))
    k["two_g"] = F(F(2) * g)
    k["light_dir"] = np.asarray(p["light_dir"], F)
    k["light_irradiance"] = np.asarray(p["light_irradiance"], F)
    k["max_distance"] = F(p["max_distance"])
    k["steps"], k["flags"] = int(p["steps"]), int(p["flags"])
    return k


def constants_vector(k):
    """rsrt_fog_constants' 17 floats in order."""
    return np.concatenate([np.asarray(k[n], F).reshape(-1) for n, _ in CONSTANTS]).astype(F)


def cos_theta(k, d):
    d, l = np.asarray(d, F), k["light_dir"]
    return (((d[..., 0] * l[0]).astype(F) + (d[..., 1] * l[1]).astype(F)).astype(F) + (d[..., 2] * l[2]).astype(F)).astype(F)


def phase(k, cos):
    """rsrt_fog_phase."""
    q = (k["one_gg"] - (k["two_g"] * np.asarray(cos, F)).astype(F)).astype(F)
    return (k["phase_norm"] / (q * np.sqrt(q)).astype(F)).astype(F)


def sun(k, ph):
    """rsrt_fog_sun: [..., 3]."""
    ph = np.asarray(ph, F)
    return ((k["sigma_s"] * ph[..., None]).astype(F) * k["light_irradiance"]).astype(F)


def segment(k, hit, t_hit):
    hit, t_hit = np.asarray(hit, bool), np.asarray(t_hit, F)
    with np.errstate(invalid="ignore"):
        return np.where(hit & (t_hit < k["max_distance"]), t_hit, k["max_distance"]).astype(F)


def delta(k, L):
    return (np.asarray(L, F) / F(k["steps"])).astype(F)


def t_of(i, xi, dl):
    return ((F(i) + np.asarray(xi, F)).astype(F) * np.asarray(dl, F)).astype(F)


def point(o, d, t):
    return (np.asarray(o, F) + (np.asarray(d, F) * np.asarray(t, F)[..., None]).astype(F)).astype(F)


def transmittance(k, t):
    with np.errstate(over="ignore"):
        return sky_ref.exp2(-((k["sigma2"] * np.asarray(t, F)).astype(F)))


def sample(k, d, hit, t_hit, xi, lit, rec):
    """rsrt_fog_sample for N rays: d [N, 3], hit, t_hit, xi [N], lit [N, steps] -> rec [N, 4] + this sample."""
    L = segment(k, hit, t_hit)
    dl = delta(k, L)
    s_sun = sun(k, phase(k, cos_theta(k, d)))
    both = (s_sun + k["s_amb"]).astype(F)
    total = np.zeros((len(L), 3), F)
    for i in range(k["steps"]):
        T = transmittance(k, t_of(i, xi, dl))
        s = np.where(np.asarray(lit)[:, i, None], both, k["s_amb"][None, :]).astype(F)
        total = (total + (T[:, None] * s).astype(F)).astype(F)
    out = np.array(rec, F)
    out[:, :3] = (out[:, :3] + (total * dl[:, None]).astype(F)).astype(F)
    out[:, 3] = (out[:, 3] + transmittance(k, L)).astype(F)
    return out


def jitter(width, px, py, sample_index):
    """xi under RSRT_FOG_JITTER: the random_uniform draw that follows the camera ray's two."""
    L = oracle.lib()
    u = np.empty(px.size, np.uint32)
    for i, pix in enumerate((np.asarray(py, np.uint32) * np.uint32(width) + np.asarray(px, np.uint32)).tolist()):
        s = C.c_uint32(oracle.rng_seed(pix, int(sample_index)))
        L.orc_rng_next_u32(C.byref(s))
        L.orc_rng_next_u32(C.byref(s))
        u[i] = L.orc_rng_next_u32(C.byref(s))
    return denoise_ref._uniform(u)


def records(oscene, cam, width, height, sample_begin, sample_count, p, rec=None, rows=None):
    """What rsrt_fog_render adds for samples [sample_begin, sample_begin + sample_count): (records [H, W, 4] f32 starting from `rec`
    (zeros when None), lit [sample_count, H, W, steps] bool).  rows: only these rows of the frame are computed (the others stay as
    they were, their `lit` False)."""
    k = prepare(p)
    out = np.zeros((height, width, 4), np.float32) if rec is None else np.array(rec, np.float32)
    ys = np.arange(height) if rows is None else np.asarray(rows)
    py, px = np.meshgrid(ys, np.arange(width), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    at = py * width + px
    flat = out.reshape(-1, 4)
    lit_all = np.zeros((sample_count, height * width, k["steps"]), bool)
    for n, s in enumerate(range(sample_begin, sample_begin + sample_count)):
        o, d = denoise_ref.camera_rays(cam, width, height, px, py, s)
        xi = jitter(width, px, py, s) if k["flags"] & JITTER else np.full(px.size, F(0.5))
        hit = oracle.cast_rays(oscene, o, d, mode=0)
        did, t_hit = hit["did_hit"] != 0, hit["distance"].astype(F)
        dl = delta(k, segment(k, did, t_hit))
        pts = np.stack([point(o, d, t_of(i, xi, dl)) for i in range(k["steps"])], axis=1)  # [N, steps, 3]
        dirs = np.broadcast_to(k["light_dir"], pts.shape)
        lit = (oracle.cast_rays(oscene, pts.reshape(-1, 3), dirs.reshape(-1, 3), mode=1)["did_hit"] == 0).reshape(px.size, k["steps"])
        flat[at] = sample(k, d, did, t_hit, xi, lit, flat[at])
        lit_all[n, at] = lit
    return out, lit_all.reshape(sample_count, height, width, k["steps"])


def compose(colour, rec, n):
    """rsrt_fog_compose: colour [..., 3] (already divided by its sample total), rec [..., 4], n the fog sample total -> [..., 4], alpha 1."""
    colour, rec, n = np.asarray(colour, F), np.asarray(rec, F), F(n)
    m = (rec / n).astype(F)
    clear = (m[..., 3] == 1) & (m[..., 0] == 0) & (m[..., 1] == 0) & (m[..., 2] == 0)
    rgb = ((colour * m[..., 3:4]).astype(F) + m[..., :3]).astype(F)
    rgb = np.where(clear[..., None], colour, rgb)
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), F)], axis=-1).astype(F)


def source_colour(img, total=1):
    """The source's colour as every pass reads it: sum / sample_total for the mean, the image itself (total 1) otherwise."""
    return (np.asarray(img, F)[..., :3] / F(total)).astype(F)


def light_from_sky(sky_params, env_height):
    """rsrt_fog_light_from_sky: (dir [3], irradiance [3]) float32."""
    k = sky_ref.prepare(sky_params, env_height)
    half = sky_ref.sinf(F(F(0.5) * k["r_eff"]))
    omega = F(F(F(4) * PIF) * F(half * half))
    with np.errstate(over="ignore"):
        return np.asarray(k["sun_dir"], F), sky_ref.sat((np.asarray(k["sun_radiance"], F) * omega).astype(F))
