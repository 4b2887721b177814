/*
 * rsrt_sky.h — arithmetic of the procedural daylight sky (rsrt_environment_sky in include/rsrt.h, rsrt_sky_fill in
 * include/rsrt_host.h), as shared inline code.
 *
 * The sky is the analytic model of Preetham, Shirley, Smits, "A Practical Analytic Model for Daylight" (SIGGRAPH 1999): the
 * luminance distribution of Perez, Seals, Michalsky (1993) for the luminance Y and the chromaticities x, y, scaled by their zenith
 * values, and a sun disc attenuated per channel over the relative optical air mass of Rozenberg (1966).  Like rsrt_dof.h this is part
 * of the published numeric contract: plain f32 + - * / sqrt and compares (-ffp-contract=off, nothing fused) in exactly the order
 * written here, sin / cos / atan2 from rsrt_detmath.h and e^x from rsrt_sky_exp2 below, so a numpy restatement reproduces every bit
 * (tests/sky_ref.py holds it) and the CPU fill and the HIP kernel agree bit for bit.
 *
 * Symbols: T the turbidity, ts the sun's zenith angle (RSRT_PIO2F - sun_elevation), t the view zenith angle, g the angle between
 * view and sun.
 *   Perez:  F(t, g) = (1 + A e^(B / cos t)) (1 + C e^(D g) + E cos^2 g);  each of Y, x, y is  zenith * F(t, g) / F(0, ts).
 *   A .. E are linear in T (RSRT_SKY_PEREZ: slope, intercept), the zenith chromaticities cubic in ts and quadratic in T
 *   (RSRT_SKY_ZENITH_X / _Y, evaluated in Horner form), the zenith luminance, in kcd/m^2,
 *     Yz = (4.0453 T - 4.9710) tan chi - 0.2155 T + 2.4192,  chi = (4/9 - T/120) (pi - 2 ts),  tan = sin / cos.
 *   Yxy -> XYZ:  X = Y x / y,  Z = Y (1 - x - y) / y;  XYZ -> linear sRGB by RSRT_SKY_XYZ_TO_RGB;  each channel clamped at 0 from below.
 * Texel (x, y) of a W x H map looks along the shader's equirectangular_uv_to_direction at its centre ((x + .5) / W, (y + .5) / H):
 *   phi = (2 u - 1) PI,  theta = PI v,  dir = (sin theta cos phi, cos theta, sin theta sin phi)  with the shader's PI = 3.14159 —
 *   the mapping next-event estimation uses to turn a picked texel into a direction, so the sky is evaluated for the direction its
 *   light is cast from.  The sun is at (cos el cos az, sin el, cos el sin az).  (An azimuth beyond rsrt_sinf's range, |az| > 8192,
 *   has sine and cosine 0 there: the sun's direction shrinks to (0, sin el, 0), and everything stays finite.)
 *   g = rsrt_atan2f(|dir x sun|, dir . sun): no acos, the sun sits at g -> 0;  cos g = dir . sun clamped to [-1, 1].
 * Below the horizon (dir.y < 0): the sky value with cos t clamped up to the horizon, times ground_albedo per channel; no disc.
 * The sun disc: sun_illuminance E (klx above the atmosphere) is attenuated per channel by e^(-tau_c m),
 *   m = 1 / (cos ts + 0.025 e^(-11 cos ts)),  tau_c = RSRT_SKY_TAU_R[c] + (0.04608 T - 0.04586) RSRT_SKY_LAMBDA[c]  (Rayleigh plus
 *   Angstrom's aerosol term, beta lambda^-1.3, at the wavelengths of R, G, B).
 *   The radius is widened to r_eff = max(sun_radius, 1.5 pi / H) so that a coarse map cannot lose the sun between texel centres, and
 *   the radiance is E / (2 pi (1 - cos r_eff)), so widening keeps the illuminance.  1 - cos r is evaluated as 2 sin^2(r / 2): the
 *   same number, without the cancellation that costs 1 - cos 0.00465 half a percent in f32.
 *   The edge is a linear ramp one texel wide: coverage = clamp((r_eff - g) H / pi + 0.5, 0, 1).  E = 0 gives a sky without a disc.
 *   (A ramp of width w around a radius R integrates to the area of a disc of radius sqrt(R^2 + w^2 / 12): at R = 1.5 texels the map
 *   carries 1 + 1/27 of the illuminance, 4.2 to 4.5 % over with the texel grid counted in — tests/test_sky.py measures it in float64.)
 * scale multiplies everything.  Its default 1/64 keeps the default disc, about 1.9e6 kcd/m^2, at 2.9e4: under the binary16 range
 * (65504) of the displayed mean for maps of 2048 x 1024 and above, where the disc is not widened.
 *
 * Every output is finite and >= 0 for every parameter set rsrt_sky_params_ok accepts.  The divisions and how each is guarded:
 *   B / cos t      cos t is clamped up to RSRT_SKY_MIN_COS (2^-10); B < 0 for every accepted T, so towards the horizon the quotient
 *                  runs to -2^10 |B| and rsrt_sky_exp2 returns exactly 0 below its clamp
 *   / F(0, ts)     F(0, ts) > 0.16 for T in [2, 10] (its first factor is smallest at T = 2: 1 - 1.1056 e^-0.2833); it is clamped up
 *                  to RSRT_SKY_MIN_F all the same, and the reciprocal is taken once, in rsrt_sky_prepare
 *   / y            the chromaticity y is clamped up to RSRT_SKY_MIN_Y
 *   air mass       cos ts >= sin 1 degree > 0 and the exponential is >= 0: the denominator is > 0.017
 *   / disc         4 pi sin^2(r_eff / 2) > 0 because r_eff >= 1.5 pi / H > 0
 *   tan chi        chi <= (4/9 - 2/120) pi < pi / 2: cos chi > 0.22
 * A product that overflows (an albedo, scale or illuminance near the largest float) saturates at the largest finite float instead of
 * reaching inf, so nothing downstream meets inf * 0.
 *
 * rsrt_sky_exp2(t) is rsrt_local_exp2's polynomial and construction (include/rsrt_local.h) with the exponent clamped: exactly 0
 * for t < -126 (and NaN), t = 126 above 126; so its values are 0 or in [2^-126, 2^126], never subnormal.  Exact at integers,
 * monotone non-decreasing, and within 3.4e-6 (2^-18.2) of 2^t relatively — measured against float64 over every t = k 2^-10 in
 * [-126, 2] and the float neighbours of the integers there; the sky only uses t <= 0.  tests/test_sky.py asserts 2^-17: the
 * polynomial's own published error, 2^-18.2, plus its five roundings of 2^-24 each, rounded up to a power of two.
 * e^x = rsrt_sky_exp2(x RSRT_SKY_LOG2E).
 */
#ifndef RSRT_SKY_H
#define RSRT_SKY_H

#include <stddef.h>
#include <stdint.h>

#include "rsrt_detmath.h"
#include "rsrt_local.h" /* RSRT_LOCAL_EXP2_C1 .. C4, rsrt_exposure_as_float */
#include "rsrt_types.h" /* rsrt_sky_params */

/* rsrt_sky_params defaults */
#define RSRT_SKY_SUN_AZIMUTH 0.0f
#define RSRT_SKY_SUN_ELEVATION 0.78539816339744830962f /* 45 degrees */
#define RSRT_SKY_TURBIDITY 3.0f
#define RSRT_SKY_GROUND_ALBEDO 0.2f                    /* each channel */
#define RSRT_SKY_SCALE 0.015625f                       /* 1/64: the default disc under the binary16 range, see above */
#define RSRT_SKY_SUN_ILLUMINANCE 128.0f                /* klx */
#define RSRT_SKY_SUN_RADIUS 0.00465f
#define RSRT_SKY_FLAGS 0u
/* what rsrt_sky_params_ok accepts */
#define RSRT_SKY_MIN_ELEVATION 0.017453292519943295f   /* 1 degree */
#define RSRT_SKY_MAX_ELEVATION RSRT_PIO2F              /* 90 degrees */
#define RSRT_SKY_MIN_TURBIDITY 2.0f
#define RSRT_SKY_MAX_TURBIDITY 10.0f
#define RSRT_SKY_MAX_SUN_RADIUS 0.1f
/* the guards */
#define RSRT_SKY_MIN_COS 0.0009765625f                 /* 2^-10 */
#define RSRT_SKY_MIN_F 1.0e-6f
#define RSRT_SKY_MIN_Y 1.0e-4f
#define RSRT_SKY_LARGEST 3.40282346638528859812e38f    /* the largest finite float */

#define RSRT_SKY_SHADER_PI ((float)3.14159)            /* shader.wgsl:239, the texel -> direction mapping only */
#define RSRT_SKY_LOG2E 1.44269504088896340736f

/* A .. E of Y, x, y: {slope, intercept} in T */
static const float RSRT_SKY_PEREZ[3][5][2] = {
    {{0.1787f, -1.4630f}, {-0.3554f, 0.4275f}, {-0.0227f, 5.3251f}, {0.1206f, -2.5771f}, {-0.0670f, 0.3703f}},
    {{-0.0193f, -0.2592f}, {-0.0665f, 0.0008f}, {-0.0004f, 0.2125f}, {-0.0641f, -0.8989f}, {-0.0033f, 0.0452f}},
    {{-0.0167f, -0.2608f}, {-0.0950f, 0.0092f}, {-0.0079f, 0.2102f}, {-0.0441f, -1.6537f}, {-0.0109f, 0.0529f}}};
/* the zenith chromaticities: rows for T^2, T, 1; columns the coefficients of ts^3, ts^2, ts, 1 */
static const float RSRT_SKY_ZENITH_X[3][4] = {{0.00166f, -0.00375f, 0.00209f, 0.0f},
                                              {-0.02903f, 0.06377f, -0.03202f, 0.00394f},
                                              {0.11693f, -0.21196f, 0.06052f, 0.25886f}};
static const float RSRT_SKY_ZENITH_Y[3][4] = {{0.00275f, -0.00610f, 0.00317f, 0.0f},
                                              {-0.04214f, 0.08970f, -0.04153f, 0.00516f},
                                              {0.15346f, -0.26756f, 0.06670f, 0.26688f}};
static const float RSRT_SKY_XYZ_TO_RGB[3][3] = {{3.2406f, -1.5372f, -0.4986f}, {-0.9689f, 1.8758f, 0.0415f}, {0.0557f, -0.2040f, 1.0570f}};
static const float RSRT_SKY_TAU_R[3] = {0.0421f, 0.1001f, 0.2490f};  /* Rayleigh optical depth at R, G, B */
static const float RSRT_SKY_LAMBDA[3] = {1.651f, 2.175f, 2.907f};    /* lambda^-1.3, lambda in micrometres */

/* everything that depends on the parameters (and the map's height) alone: rsrt_sky_prepare makes it once on the host, the kernel
 * takes it by value */
typedef struct rsrt_sky_constants {
    float A[3], B[3], C[3], D[3], E[3]; /* the Perez coefficients of Y, x, y */
    float zenith[3];                    /* Yz in kcd/m^2, xz, yz */
    float inv_f0[3];                    /* 1 / F(0, ts) */
    float sun_dir[3];
    float sun_radiance[3];              /* of the disc, attenuated, scale included; 0 without a disc */
    float r_eff;                        /* the widened radius */
    float ramp;                         /* H / pi: texels a radian */
    float ground[3];
    float scale;
} rsrt_sky_constants;

/* what a row of the map shares: sin and cos of its theta and the first Perez factor 1 + A e^(B / cos t) of Y, x, y */
typedef struct rsrt_sky_row { float st, ct, p[3]; } rsrt_sky_row;
/* what a column shares: cos and sin of its phi */
typedef struct rsrt_sky_col { float cp, sp; } rsrt_sky_col;

RSRT_HD int rsrt_sky_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }
/* finite and >= 0 */
RSRT_HD int rsrt_sky_amount(float x) { return x >= 0.0f && x < __builtin_inff(); }

RSRT_HD int rsrt_sky_params_ok(const rsrt_sky_params *p)
{
    return rsrt_sky_finite(p->sun_azimuth) && p->sun_elevation >= RSRT_SKY_MIN_ELEVATION && p->sun_elevation <= RSRT_SKY_MAX_ELEVATION &&
           p->turbidity >= RSRT_SKY_MIN_TURBIDITY && p->turbidity <= RSRT_SKY_MAX_TURBIDITY && rsrt_sky_amount(p->ground_albedo[0]) &&
           rsrt_sky_amount(p->ground_albedo[1]) && rsrt_sky_amount(p->ground_albedo[2]) && rsrt_sky_amount(p->scale) &&
           rsrt_sky_amount(p->sun_illuminance) && p->sun_radius >= 0.0f && p->sun_radius <= RSRT_SKY_MAX_SUN_RADIUS && p->flags == 0u;
}

/* 2^t, clamped: 0 for t < -126 or NaN, 2^126 from 126 up */
RSRT_HD float rsrt_sky_exp2(float t)
{
    if (!(t >= -126.0f)) return 0.0f;
    if (t > 126.0f) t = 126.0f;
    int n = (int)t;
    if ((float)n > t) n = n - 1;
    const float f = t - (float)n;
    float p = RSRT_LOCAL_EXP2_C4;
    p = p * f + RSRT_LOCAL_EXP2_C3;
    p = p * f + RSRT_LOCAL_EXP2_C2;
    p = p * f + RSRT_LOCAL_EXP2_C1;
    p = p * f + 1.0f;
    return p * rsrt_exposure_as_float((uint32_t)(n + 127) << 23);
}
RSRT_HD float rsrt_sky_exp(float x) { return rsrt_sky_exp2(x * RSRT_SKY_LOG2E); }

/* min(x, the largest finite float); a NaN becomes it too */
RSRT_HD float rsrt_sky_sat(float x) { return x < RSRT_SKY_LARGEST ? x : RSRT_SKY_LARGEST; }

/* the two factors of F: 1 + A e^(B / cos t), cos t already clamped, and 1 + C e^(D g) + E cos^2 g */
RSRT_HD float rsrt_sky_perez_zenith(float A, float B, float cos_t) { return 1.0f + A * rsrt_sky_exp(B / cos_t); }
RSRT_HD float rsrt_sky_perez_sun(float C, float D, float E, float g, float cos_g) { return (1.0f + C * rsrt_sky_exp(D * g)) + E * (cos_g * cos_g); }

/* c[0] ts^3 + c[1] ts^2 + c[2] ts + c[3] */
RSRT_HD float rsrt_sky_cubic(const float c[4], float ts) { return ((c[0] * ts + c[1]) * ts + c[2]) * ts + c[3]; }
RSRT_HD float rsrt_sky_zenith_chroma(const float m[3][4], float T, float ts)
{
    return (rsrt_sky_cubic(m[0], ts) * (T * T) + rsrt_sky_cubic(m[1], ts) * T) + rsrt_sky_cubic(m[2], ts);
}

/* p must pass rsrt_sky_params_ok; height > 0 is the map's */
RSRT_HD void rsrt_sky_prepare(const rsrt_sky_params *p, uint32_t height, rsrt_sky_constants *k)
{
    const float T = p->turbidity;
    for (int c = 0; c < 3; c++) {
        k->A[c] = RSRT_SKY_PEREZ[c][0][0] * T + RSRT_SKY_PEREZ[c][0][1];
        k->B[c] = RSRT_SKY_PEREZ[c][1][0] * T + RSRT_SKY_PEREZ[c][1][1];
        k->C[c] = RSRT_SKY_PEREZ[c][2][0] * T + RSRT_SKY_PEREZ[c][2][1];
        k->D[c] = RSRT_SKY_PEREZ[c][3][0] * T + RSRT_SKY_PEREZ[c][3][1];
        k->E[c] = RSRT_SKY_PEREZ[c][4][0] * T + RSRT_SKY_PEREZ[c][4][1];
    }
    const float ts = RSRT_PIO2F - p->sun_elevation;
    const float se = rsrt_sinf(p->sun_elevation), ce = rsrt_cosf(p->sun_elevation); /* se = cos ts */
    k->sun_dir[0] = ce * rsrt_cosf(p->sun_azimuth);
    k->sun_dir[1] = se;
    k->sun_dir[2] = ce * rsrt_sinf(p->sun_azimuth);
    const float chi = (4.0f / 9.0f - T / 120.0f) * (RSRT_PIF - 2.0f * ts);
    const float tan_chi = rsrt_sinf(chi) / rsrt_cosf(chi);
    k->zenith[0] = ((4.0453f * T - 4.9710f) * tan_chi - 0.2155f * T) + 2.4192f;
    k->zenith[1] = rsrt_sky_zenith_chroma(RSRT_SKY_ZENITH_X, T, ts);
    k->zenith[2] = rsrt_sky_zenith_chroma(RSRT_SKY_ZENITH_Y, T, ts);
    for (int c = 0; c < 3; c++) {
        const float f0 = rsrt_sky_perez_zenith(k->A[c], k->B[c], 1.0f) * rsrt_sky_perez_sun(k->C[c], k->D[c], k->E[c], ts, se);
        k->inv_f0[c] = 1.0f / (f0 < RSRT_SKY_MIN_F ? RSRT_SKY_MIN_F : f0);
    }
    const float r_min = 1.5f * RSRT_PIF / (float)height;
    k->r_eff = p->sun_radius < r_min ? r_min : p->sun_radius;
    k->ramp = (float)height / RSRT_PIF;
    const float half = rsrt_sinf(0.5f * k->r_eff);
    const float omega = (4.0f * RSRT_PIF) * (half * half); /* 2 pi (1 - cos r_eff) */
    const float m = 1.0f / (se + 0.025f * rsrt_sky_exp(-11.0f * se));
    const float beta = 0.04608f * T - 0.04586f;
    for (int c = 0; c < 3; c++) {
        const float tau = RSRT_SKY_TAU_R[c] + beta * RSRT_SKY_LAMBDA[c];
        const float e = p->sun_illuminance * rsrt_sky_exp(-(tau * m));
        k->sun_radiance[c] = p->sun_illuminance > 0.0f ? rsrt_sky_sat(rsrt_sky_sat(e / omega) * p->scale) : 0.0f;
        k->ground[c] = p->ground_albedo[c];
    }
    k->scale = p->scale;
}

RSRT_HD rsrt_sky_row rsrt_sky_row_of(const rsrt_sky_constants *k, uint32_t y, uint32_t height)
{
    rsrt_sky_row r;
    const float theta = RSRT_SKY_SHADER_PI * (((float)y + 0.5f) / (float)height);
    r.st = rsrt_sinf(theta);
    r.ct = rsrt_cosf(theta);
    const float c = r.ct < RSRT_SKY_MIN_COS ? RSRT_SKY_MIN_COS : r.ct;
    for (int i = 0; i < 3; i++) r.p[i] = rsrt_sky_perez_zenith(k->A[i], k->B[i], c);
    return r;
}

RSRT_HD rsrt_sky_col rsrt_sky_col_of(uint32_t x, uint32_t width)
{
    rsrt_sky_col c;
    const float phi = (2.0f * (((float)x + 0.5f) / (float)width) - 1.0f) * RSRT_SKY_SHADER_PI;
    c.cp = rsrt_cosf(phi);
    c.sp = rsrt_sinf(phi);
    return c;
}

/* the disc's share of a texel at the angle g from the sun: a linear ramp one texel wide around r_eff */
RSRT_HD float rsrt_sky_coverage(const rsrt_sky_constants *k, float g)
{
    const float c = (k->r_eff - g) * k->ramp + 0.5f;
    return c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
}

/* one texel from its row's and its column's shares: rgb */
RSRT_HD void rsrt_sky_texel(const rsrt_sky_constants *k, rsrt_sky_row r, rsrt_sky_col c, float out[3])
{
    const float dx = r.st * c.cp, dy = r.ct, dz = r.st * c.sp;
    const float sx = k->sun_dir[0], sy = k->sun_dir[1], sz = k->sun_dir[2];
    const float cx = dy * sz - dz * sy, cy = dz * sx - dx * sz, cz = dx * sy - dy * sx;
    const float cross = rsrt_sqrtf((cx * cx + cy * cy) + cz * cz);
    const float dot = (dx * sx + dy * sy) + dz * sz;
    const float g = rsrt_atan2f(cross, dot);
    const float cos_g = dot < -1.0f ? -1.0f : (dot > 1.0f ? 1.0f : dot);
    float v[3];
    for (int i = 0; i < 3; i++) v[i] = (k->zenith[i] * (r.p[i] * rsrt_sky_perez_sun(k->C[i], k->D[i], k->E[i], g, cos_g))) * k->inv_f0[i];
    const float Y = v[0], x = v[1], y = v[2] < RSRT_SKY_MIN_Y ? RSRT_SKY_MIN_Y : v[2];
    const float X = (Y * x) / y, Z = (Y * ((1.0f - x) - y)) / y;
    const int below = dy < 0.0f;
    const float cover = below ? 0.0f : rsrt_sky_coverage(k, g);
    for (int i = 0; i < 3; i++) {
        float s = (RSRT_SKY_XYZ_TO_RGB[i][0] * X + RSRT_SKY_XYZ_TO_RGB[i][1] * Y) + RSRT_SKY_XYZ_TO_RGB[i][2] * Z;
        s = s > 0.0f ? s : 0.0f;
        if (below) s = rsrt_sky_sat(s * k->ground[i]);
        s = rsrt_sky_sat(s * k->scale);
        out[i] = rsrt_sky_sat(s + cover * k->sun_radiance[i]);
    }
}

/* texel (x, y) of a width x height map, every share formed on the spot: what rsrt_sky_fill loops over */
RSRT_HD void rsrt_sky_at(const rsrt_sky_constants *k, uint32_t x, uint32_t y, uint32_t width, uint32_t height, float out[3])
{
    rsrt_sky_texel(k, rsrt_sky_row_of(k, y, height), rsrt_sky_col_of(x, width), out);
}

#endif
