"""The procedural daylight sky (include/rsrt_sky.h) restated in numpy: rsrt_detmath.h's sin, cos and atan2, rsrt_sky_exp2, the
constants rsrt_sky_prepare makes of a parameter set, a row's and a column's shares and the per-texel function, in float32, operation
for operation and in the header's order.  The CPU evaluations of the header (tests/test_sky.py: librsrt_host.so's rsrt_sky_fill and
tests/cpp/sky_host.cpp's per-texel loop) and the GPU kernel (tests/test_sky_gpu.py) equal it bit for bit.  The sun's float64
illuminance sum at the end is what the test of the disc takes its margin from."""
import numpy as np

F = np.float32
PIF = F(3.14159265358979323846)
PIO2F = F(1.57079632679489661923)
PIO4F = F(0.78539816339744830962)
SHADER_PI = F(3.14159)
LOG2E = F(1.44269504088896340736)
LARGEST = np.finfo(F).max
MIN_COS, MIN_F, MIN_Y = F(2.0 ** -10), F(1.0e-6), F(1.0e-4)
MIN_ELEVATION, MAX_ELEVATION = F(0.017453292519943295), PIO2F
DEFAULTS = {"sun_azimuth": 0.0, "sun_elevation": float(PIO4F), "turbidity": 3.0, "ground_albedo": (float(F(0.2)),) * 3, "scale": 1.0 / 64,
            "sun_illuminance": 128.0, "sun_radius": float(F(0.00465)), "flags": 0}
FIELDS = ("sun_azimuth", "sun_elevation", "turbidity", "ground_albedo", "scale", "sun_illuminance", "sun_radius", "flags")
EXP2_C = (F(0.6930321455), F(0.2413797677), F(0.05203237012), F(0.01355574746))
PEREZ = np.array([[[0.1787, -1.4630], [-0.3554, 0.4275], [-0.0227, 5.3251], [0.1206, -2.5771], [-0.0670, 0.3703]],
                  [[-0.0193, -0.2592], [-0.0665, 0.0008], [-0.0004, 0.2125], [-0.0641, -0.8989], [-0.0033, 0.0452]],
                  [[-0.0167, -0.2608], [-0.0950, 0.0092], [-0.0079, 0.2102], [-0.0441, -1.6537], [-0.0109, 0.0529]]], F)
ZENITH_X = np.array([[0.00166, -0.00375, 0.00209, 0.0], [-0.02903, 0.06377, -0.03202, 0.00394], [0.11693, -0.21196, 0.06052, 0.25886]], F)
ZENITH_Y = np.array([[0.00275, -0.00610, 0.00317, 0.0], [-0.04214, 0.08970, -0.04153, 0.00516], [0.15346, -0.26756, 0.06670, 0.26688]], F)
XYZ_TO_RGB = np.array([[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415], [0.0557, -0.2040, 1.0570]], F)
TAU_R = np.array([0.0421, 0.1001, 0.2490], F)
LAMBDA = np.array([1.651, 2.175, 2.907], F)
# the order of rsrt_sky_constants' 33 floats
CONSTANTS = (("A", 3), ("B", 3), ("C", 3), ("D", 3), ("E", 3), ("zenith", 3), ("inv_f0", 3), ("sun_dir", 3), ("sun_radiance", 3), ("r_eff", 1),
             ("ramp", 1), ("ground", 3), ("scale", 1))


def params(**kw):
    """DEFAULTS with `kw` over them, every float rounded to float32."""
    assert set(kw) <= set(FIELDS), kw
    p = dict(DEFAULTS, **kw)
    p["ground_albedo"] = tuple(float(F(a)) for a in p["ground_albedo"])
    for n in ("sun_azimuth", "sun_elevation", "turbidity", "scale", "sun_illuminance", "sun_radius"):
        p[n] = float(F(p[n]))
    return p


def params_ok(p):
    """rsrt_sky_params_ok."""
    fin = lambda v: bool(np.isfinite(F(v)))  # noqa: E731
    amount = lambda v: fin(v) and F(v) >= 0  # noqa: E731
    return bool(fin(p["sun_azimuth"]) and MIN_ELEVATION <= F(p["sun_elevation"]) <= MAX_ELEVATION and F(2) <= F(p["turbidity"]) <= F(10) and
                all(amount(a) for a in p["ground_albedo"]) and amount(p["scale"]) and amount(p["sun_illuminance"]) and
                F(0) <= F(p["sun_radius"]) <= F(0.1) and p["flags"] == 0)


# -- rsrt_detmath.h ------------------------------------------------------------------------------------------------------------
DP1, DP2, DP3, FOPI = F(0.78515625), F(2.4187564849853515625e-4), F(3.77489497744594108e-8), F(1.27323954473516)


def _sin_poly(r, z):
    p = (F(-1.9515295891e-4) * z + F(8.3321608736e-3)).astype(F)
    p = (p * z - F(1.6666654611e-1)).astype(F)
    return (p * z * r + r).astype(F)


def _cos_poly(z):
    p = (F(2.443315711809948e-5) * z - F(1.388731625493765e-3)).astype(F)
    p = (p * z + F(4.166664568298827e-2)).astype(F)
    p = (p * z * z).astype(F)
    p = (p - F(0.5) * z).astype(F)
    return (p + F(1)).astype(F)


def _reduce(x):
    ax = np.abs(np.asarray(x, F))
    assert (ax <= 8192).all()
    j = (ax * FOPI).astype(F).astype(np.int64)
    j = j + (j & 1)
    y = j.astype(F)
    r = (((ax - y * DP1).astype(F) - y * DP2).astype(F) - y * DP3).astype(F)
    return r, (r * r).astype(F), j & 7


def sinf(x):
    """rsrt_sinf of float32 x, |x| <= 8192."""
    x = np.asarray(x, F)
    r, z, j = _reduce(x)
    neg = (x < 0) ^ (j > 3)
    j = np.where(j > 3, j - 4, j)
    v = np.where((j == 1) | (j == 2), _cos_poly(z), _sin_poly(r, z)).astype(F)
    return np.where(neg, -v, v).astype(F)


def cosf(x):
    """rsrt_cosf of float32 x, |x| <= 8192."""
    x = np.asarray(x, F)
    r, z, j = _reduce(x)
    neg = j > 3
    j = np.where(j > 3, j - 4, j)
    neg = neg ^ (j > 1)
    v = np.where((j == 1) | (j == 2), _sin_poly(r, z), _cos_poly(z)).astype(F)
    return np.where(neg, -v, v).astype(F)


def atanf(xx):
    xx = np.asarray(xx, F)
    neg = xx < 0
    x = np.abs(xx)
    big, mid = x > F(2.414213562373095), x > F(0.4142135623730950)
    with np.errstate(all="ignore"):
        xr = np.where(big, -(F(1) / x).astype(F), np.where(mid, ((x - F(1)).astype(F) / (x + F(1)).astype(F)).astype(F), x)).astype(F)
    y = np.where(big, PIO2F, np.where(mid, PIO4F, F(0))).astype(F)
    z = (xr * xr).astype(F)
    p = (F(8.05374449538e-2) * z - F(1.38776856032e-1)).astype(F)
    p = (p * z + F(1.99777106478e-1)).astype(F)
    p = (p * z - F(3.33329491539e-1)).astype(F)
    y = (y + (p * z * xr + xr).astype(F)).astype(F)
    return np.where(neg, -y, y).astype(F)


def atan2f(y, x):
    """rsrt_atan2f of finite float32 y, x."""
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    with np.errstate(all="ignore"):
        w = np.where(x < 0, np.where(y < 0, -PIF, PIF), F(0)).astype(F)
        general = (w + atanf((y / x).astype(F))).astype(F)
    out = np.where(y == 0, np.where(x < 0, PIF, F(0)), general)
    out = np.where(x == 0, np.where(y > 0, PIO2F, np.where(y < 0, -PIO2F, F(0))), out)
    return out.astype(F)


# -- rsrt_sky.h ----------------------------------------------------------------------------------------------------------------
def exp2(t):
    """rsrt_sky_exp2 of float32 t."""
    t = np.asarray(t, F)
    with np.errstate(invalid="ignore"):
        zero = ~(t >= F(-126))
    c = np.where(zero, F(0), np.minimum(t, F(126))).astype(F)
    n = c.astype(np.int32)  # truncates
    n = np.where(n.astype(F) > c, n - 1, n).astype(np.int32)
    f = (c - n.astype(F)).astype(F)
    p = np.full(c.shape, EXP2_C[3], F)
    for k in (EXP2_C[2], EXP2_C[1], EXP2_C[0], F(1)):
        p = ((p * f).astype(F) + k).astype(F)
    return np.where(zero, F(0), (p * ((n + 127).astype(np.uint32) << np.uint32(23)).view(F)).astype(F)).astype(F)


def exp(x):
    return exp2((np.asarray(x, F) * LOG2E).astype(F))


def sat(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(x, F) < LARGEST, x, LARGEST).astype(F)


def perez_zenith(A, B, cos_t):
    with np.errstate(over="ignore"):
        return (F(1) + (A * exp((B / cos_t).astype(F))).astype(F)).astype(F)


def perez_sun(C, D, E, g, cos_g):
    return ((F(1) + (C * exp((D * g).astype(F))).astype(F)).astype(F) + (E * (cos_g * cos_g).astype(F)).astype(F)).astype(F)


def _cubic(c, ts):
    return ((((c[0] * ts).astype(F) + c[1]).astype(F) * ts + c[2]).astype(F) * ts + c[3]).astype(F)


def _zenith_chroma(m, T, ts):
    return (((_cubic(m[0], ts) * (T * T).astype(F)).astype(F) + (_cubic(m[1], ts) * T).astype(F)).astype(F) + _cubic(m[2], ts)).astype(F)


def prepare(p, height):
    """rsrt_sky_prepare: a dict of float32 arrays and scalars named as rsrt_sky_constants' fields."""
    T, el, az = F(p["turbidity"]), F(p["sun_elevation"]), F(p["sun_azimuth"])
    k = {}
    for i, n in enumerate("ABCDE"):
        k[n] = ((PEREZ[:, i, 0] * T).astype(F) + PEREZ[:, i, 1]).astype(F)
    ts = F(PIO2F - el)
    se, ce = sinf(el), cosf(el)
    k["sun_dir"] = np.array([ce * cosf(az), se, ce * sinf(az)], F)
    chi = F(F(F(4) / F(9) - T / F(120)) * F(PIF - F(F(2) * ts)))
    tan_chi = F(sinf(chi) / cosf(chi))
    k["zenith"] = np.array([F(F(F(F(F(4.0453) * T) - F(4.9710)) * tan_chi) - F(F(0.2155) * T)) + F(2.4192), _zenith_chroma(ZENITH_X, T, ts),
                            _zenith_chroma(ZENITH_Y, T, ts)], F)
    f0 = (perez_zenith(k["A"], k["B"], F(1)) * perez_sun(k["C"], k["D"], k["E"], ts, se)).astype(F)
    k["inv_f0"] = (F(1) / np.maximum(f0, MIN_F)).astype(F)
    r_min = F(F(F(1.5) * PIF) / F(height))
    k["r_eff"] = max(F(p["sun_radius"]), r_min)
    k["ramp"] = F(F(height) / PIF)
    half = sinf(F(F(0.5) * k["r_eff"]))
    omega = F(F(F(4) * PIF) * F(half * half))
    m = F(F(1) / F(se + F(F(0.025) * exp(F(F(-11) * se)))))
    beta = F(F(F(0.04608) * T) - F(0.04586))
    tau = (TAU_R + (beta * LAMBDA).astype(F)).astype(F)
    E, scale = F(p["sun_illuminance"]), F(p["scale"])
    with np.errstate(over="ignore"):
        e = (E * exp(-(tau * m).astype(F))).astype(F)
        rad = sat((sat((e / omega).astype(F)) * scale).astype(F))
    k["sun_radiance"] = rad if E > 0 else np.zeros(3, F)
    k["ground"] = np.array(p["ground_albedo"], F)
    k["scale"] = scale
    return k


def constants_vector(k):
    """The 33 floats of rsrt_sky_constants."""
    return np.concatenate([np.atleast_1d(np.asarray(k[n], F)) for n, _ in CONSTANTS]).astype(F)


def rows(k, height):
    """rsrt_sky_row_of of every row: st, ct [H] and p [H, 3]."""
    theta = (SHADER_PI * ((np.arange(height).astype(F) + F(0.5)).astype(F) / F(height)).astype(F)).astype(F)
    st, ct = sinf(theta), cosf(theta)
    c = np.maximum(ct, MIN_COS).astype(F)
    return st, ct, perez_zenith(k["A"][None, :], k["B"][None, :], c[:, None])


def cols(width):
    """rsrt_sky_col_of of every column: cp, sp [W]."""
    u = ((np.arange(width).astype(F) + F(0.5)).astype(F) / F(width)).astype(F)
    phi = (((F(2) * u).astype(F) - F(1)).astype(F) * SHADER_PI).astype(F)
    return cosf(phi), sinf(phi)


def directions(width, height):
    """[H, W, 3] float32: the direction of every texel."""
    st, ct, _ = rows({"A": np.zeros(3, F), "B": np.zeros(3, F)}, height)
    cp, sp = cols(width)
    return np.stack([(st[:, None] * cp[None, :]).astype(F), np.broadcast_to(ct[:, None], (height, width)), (st[:, None] * sp[None, :]).astype(F)], axis=-1)


def angle_to_sun(k, width, height):
    """g and dir . sun of every texel, [H, W] float32 each."""
    d = directions(width, height)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    sx, sy, sz = k["sun_dir"]
    cx = ((dy * sz).astype(F) - (dz * sy).astype(F)).astype(F)
    cy = ((dz * sx).astype(F) - (dx * sz).astype(F)).astype(F)
    cz = ((dx * sy).astype(F) - (dy * sx).astype(F)).astype(F)
    cross = np.sqrt((((cx * cx).astype(F) + (cy * cy).astype(F)).astype(F) + (cz * cz).astype(F)).astype(F)).astype(F)
    dot = (((dx * sx).astype(F) + (dy * sy).astype(F)).astype(F) + (dz * sz).astype(F)).astype(F)
    return atan2f(cross, dot), dot


def coverage(k, g):
    c = (((k["r_eff"] - g).astype(F) * k["ramp"]).astype(F) + F(0.5)).astype(F)
    return np.clip(c, F(0), F(1)).astype(F)


def fill(width, height, p):
    """rsrt_sky_fill / rsrt_environment_sky: [H, W, 4] float32, alpha 0."""
    assert params_ok(p)
    k = prepare(p, height)
    _, ct, rp = rows(k, height)
    g, dot = angle_to_sun(k, width, height)
    cos_g = np.clip(dot, F(-1), F(1)).astype(F)
    v = []
    for i in range(3):
        f = (rp[:, i][:, None] * perez_sun(k["C"][i], k["D"][i], k["E"][i], g, cos_g)).astype(F)
        v.append(((k["zenith"][i] * f).astype(F) * k["inv_f0"][i]).astype(F))
    Y, x, y = v[0], v[1], np.maximum(v[2], MIN_Y).astype(F)
    X = ((Y * x).astype(F) / y).astype(F)
    Z = ((Y * ((F(1) - x).astype(F) - y).astype(F)).astype(F) / y).astype(F)
    below = np.broadcast_to((ct < 0)[:, None], (height, width))
    cover = np.where(below, F(0), coverage(k, g)).astype(F)
    out = np.zeros((height, width, 4), F)
    with np.errstate(over="ignore"):
        for i in range(3):
            m = XYZ_TO_RGB[i]
            s = (((m[0] * X).astype(F) + (m[1] * Y).astype(F)).astype(F) + (m[2] * Z).astype(F)).astype(F)
            s = np.where(s > 0, s, F(0)).astype(F)
            s = np.where(below, sat((s * k["ground"][i]).astype(F)), s).astype(F)
            s = sat((s * k["scale"]).astype(F))
            out[..., i] = sat((s + (cover * k["sun_radiance"][i]).astype(F)).astype(F))
    return out


# -- the disc's illuminance in float64 -----------------------------------------------------------------------------------------------
def solid_angles(width, height):
    """The solid angle of every row's texels under the fill's own mapping (its PI = 3.14159), float64 [H]: exact band areas."""
    pi = float(SHADER_PI)
    edges = pi * np.arange(height + 1, dtype=np.float64) / height
    return (np.cos(edges[:-1]) - np.cos(edges[1:])) * (2.0 * pi / width)


def disc_illuminance_f64(width, height, p):
    """The sum over texels of coverage * disc radiance * solid angle / scale in float64, as a fraction of the attenuated illuminance
    (per channel the same number): what the one-texel ramp and the texel grid make of a disc whose exact integral is 1."""
    el, az = float(F(p["sun_elevation"])), float(F(p["sun_azimuth"]))
    pi = float(SHADER_PI)
    theta = pi * (np.arange(height) + 0.5) / height
    phi = (2.0 * (np.arange(width) + 0.5) / width - 1.0) * pi
    d = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None, :], np.broadcast_to(np.cos(theta)[:, None], (height, width)),
                  np.sin(theta)[:, None] * np.sin(phi)[None, :]], axis=-1)
    s = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    g = np.arctan2(np.linalg.norm(np.cross(d, s), axis=-1), d @ s)
    r_eff = max(float(F(p["sun_radius"])), 1.5 * np.pi / height)
    cover = np.clip((r_eff - g) * height / np.pi + 0.5, 0.0, 1.0) * (d[..., 1] >= 0)
    omega = 2.0 * np.pi * (1.0 - np.cos(r_eff))
    return float((cover * solid_angles(width, height)[:, None]).sum() / omega)


# -- what the CPU and the GPU tests share ----------------------------------------------------------------------------------------------
SIZES = [(8, 4), (37, 19), (64, 32), (256, 128)]  # (w, h); 37 x 19: no multiple of a wave, and a middle row on the shader's almost-horizon
CASES = {"defaults": {}, "sun_at_zenith": {"sun_elevation": float(MAX_ELEVATION)}, "sun_at_1_degree": {"sun_elevation": float(MIN_ELEVATION)},
         "turbidity_2": {"turbidity": 2.0}, "turbidity_10": {"turbidity": 10.0}, "no_disc": {"sun_illuminance": 0.0},
         "black_ground": {"ground_albedo": (0.0, 0.0, 0.0)}, "turned": {"sun_azimuth": 2.1, "sun_elevation": 0.6, "ground_albedo": (0.3, 0.2, 0.1)}}
# every refusal of rsrt_sky_params_ok, as overrides of the defaults
REFUSED = {"nan_azimuth": {"sun_azimuth": float("nan")}, "inf_azimuth": {"sun_azimuth": float("inf")}, "nan_elevation": {"sun_elevation": float("nan")},
           "low_elevation": {"sun_elevation": float(np.nextafter(MIN_ELEVATION, F(0)))}, "high_elevation": {"sun_elevation": float(np.nextafter(MAX_ELEVATION, F(2)))},
           "negative_elevation": {"sun_elevation": -0.5}, "nan_turbidity": {"turbidity": float("nan")},
           "low_turbidity": {"turbidity": float(np.nextafter(F(2), F(0)))}, "high_turbidity": {"turbidity": float(np.nextafter(F(10), F(11)))},
           "negative_albedo": {"ground_albedo": (0.2, -0.1, 0.2)}, "nan_albedo": {"ground_albedo": (0.2, 0.2, float("nan"))},
           "inf_albedo": {"ground_albedo": (float("inf"), 0.2, 0.2)}, "negative_scale": {"scale": -1.0}, "inf_scale": {"scale": float("inf")},
           "nan_scale": {"scale": float("nan")}, "negative_illuminance": {"sun_illuminance": -1.0}, "inf_illuminance": {"sun_illuminance": float("inf")},
           "nan_illuminance": {"sun_illuminance": float("nan")}, "negative_radius": {"sun_radius": -0.001}, "wide_radius": {"sun_radius": float(np.nextafter(F(0.1), F(1)))},
           "nan_radius": {"sun_radius": float("nan")}, "flags": {"flags": 1}}
_cache = {}


def reference(case, width, height):
    """fill() of CASES[case], computed once a session and read-only."""
    key = (case, width, height)
    if key not in _cache:
        _cache[key] = fill(width, height, params(**CASES[case]))
        _cache[key].setflags(write=False)
    return _cache[key]


def fnv1a(data):
    """FNV-1a over the bytes of an array, as tests/cpp/*_demo.cpp print it."""
    h = 1469598103934665603
    for b in np.ascontiguousarray(data).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
    return h
