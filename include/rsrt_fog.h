/*
 * rsrt_fog.h — arithmetic of the volumetric fog pass (rsrt_fog_render, rsrt_fog_apply in include/rsrt.h), as shared inline code.
 *
 * The medium is homogeneous: one extinction coefficient sigma_t (`density`) everywhere between the camera and the surfaces.  It is lit
 * by single scattering from ONE directional light (light_dir, light_irradiance) through the Henyey-Greenstein phase function, plus a
 * constant isotropic ambient term.  Like rsrt_dof.h and rsrt_sky.h this is part of the published numeric contract: plain f32 + - * /,
 * rsrt_sqrtf, compares and rsrt_sky_exp2 (-ffp-contract=off, nothing fused) in exactly the order written here, so a numpy restatement
 * reproduces every bit (tests/fog_ref.py holds it) and the CPU evaluation and the HIP kernels agree bit for bit.
 *
 * Constants (rsrt_fog_prepare, once on the host):
 *   sigma' = density * log2 e;   sigma_s[c] = density * albedo[c];   S_amb[c] = sigma_s[c] * ambient[c];
 *   phase_norm = (1 - g g) / (4 pi);   one_gg = 1 + g g;   two_g = 2 g.
 * Per pixel and per sample k, with (o, d) the camera ray rsrt_render casts for (pixel, k):
 *   xi       0.5, or under RSRT_FOG_JITTER the random_uniform draw that follows the camera ray's two (in [0, 1], both ends included)
 *   L        min(t_hit, max_distance) on a hit (the closest hit as rsrt_cast_rays mode 0 takes it), max_distance on a miss
 *   delta    L / (float)steps
 *   q        one_gg - two_g * (d . light_dir),  the dot product summed as (x + y) + z
 *   phase    phase_norm / (q * rsrt_sqrtf(q))
 *   S_sun[c] (sigma_s[c] * phase) * light_irradiance[c]
 *   for i = 0 .. steps - 1, in order:
 *     t_i  = ((float)i + xi) * delta
 *     x_i  = o + d * t_i                                  one multiply and one add a component
 *     lit  = the shadow query from x_i along light_dir finds no hit (the tree walk alone, rsrt_cast_rays mode 1)
 *     T_i  = rsrt_sky_exp2(-(sigma' * t_i))
 *     sum[c] = sum[c] + T_i * (lit ? S_sun[c] + S_amb[c] : S_amb[c])
 *   inscatter[c] = sum[c] * delta;   transmittance = rsrt_sky_exp2(-(sigma' * L))
 *   record = record + (inscatter rgb, transmittance), in increasing k.
 * The sum is the midpoint rule (xi = 0.5) of the integral of T(t) S(t) over [0, L]; a sky pixel is seen through max_distance of fog.
 * Compose (rsrt_fog_apply), with n the fog sample total:  Tm = rec.w / n,  I[c] = rec[c] / n,  out[c] = colour[c] * Tm + I[c], alpha 1;
 * a pixel with Tm == 1 and I == 0 (density 0) is the source's colour itself, so a clear medium gives the source bit for bit.
 *
 * What is left out: the light's own attenuation on its way to x_i.  A homogeneous medium without bounds would put out a light at
 * infinity altogether, so the light reaches every unoccluded point at full strength; light_irradiance is what arrives.  Nor is there
 * multiple scattering, a height or density field, or fog inside the integrator: surfaces are lit as if the air were clear.
 *
 * Finiteness.  One sample's every quantity — q, phase, S_sun, S_amb, T_i, the running sum, inscatter, transmittance — is finite for
 * every parameter set rsrt_fog_params_ok accepts and a unit ray direction.  Each field within its own range is not enough (S_sun
 * overflows to inf for density 1e6 and the largest irradiance, and T_i is exactly 0 beyond rsrt_sky_exp2's clamp: 0 * inf), so
 * rsrt_fog_params_ok also bounds the products, from the expressions above:
 *   sigma' t  <= sigma' * max_distance (1 + 2^-22), held to half the largest float; rsrt_sky_exp2 returns exactly 0 below its clamp.
 *   q         |d . light_dir| <= 1.001 for a unit d and a light_dir within the accepted length (len <= 1.0005), so
 *             q >= q_lo = ((1 + g g) - 2 |g|) - (2 |g|) * 1e-3,  which is > 5.9e-4 for |g| <= 0.95.
 *   phase     <= phase_hi = phase_norm / (q_lo * rsrt_sqrtf(q_lo)):  the phase at cos = +-1 with q's lower bound in place of q.
 *   source    S_sun[c] + S_amb[c] <= S = (s * phase_hi) * max_c light_irradiance[c] + s * max_c ambient[c],  s = density * max_c albedo[c].
 *   sum       T_i <= 1, so sum[c] <= (float)steps * S: also what a hit at t = 0 (delta = 0, every T_i = 1) multiplies by 0.
 *   inscatter sum[c] * delta <= S * W with W = delta * (T_0 + T_1 + ...), delta = L / steps <= delta_hi = max_distance / (float)steps.
 *             W <= steps * delta = L <= max_distance.  And T_0 <= 1, while for i >= 1, xi >= 0 and the convex e^(-sigma t) the term
 *             delta e^(-sigma i delta) is at most the integral over [(i - 1/2) delta, (i + 1/2) delta], so the terms after the first sum
 *             to at most e^(-sigma delta / 2) / sigma <= 1 / (sigma + sigma^2 delta / 2)  (e^-x <= 1 / (1 + x)); the bound grows with
 *             delta, so  W <= W_hi = min(max_distance, delta_hi + 1 / (density + (density * density) * (0.5 * delta_hi))).
 * rsrt_fog_params_ok requires (float)steps * S <= RSRT_FOG_HEADROOM * largest float and S * W_hi <= the same; the one per cent of
 * headroom is far above what the f32 roundings of the march (64 terms) and rsrt_sky_exp2's 2^-17 can add.  (density 0: W_hi =
 * max_distance, S = 0.)  A record is a sum over samples of such non-negative finite terms: over very many samples it may overflow, and
 * then it is +inf, never NaN; rsrt_fog_apply then shows +inf in that channel.
 */
#ifndef RSRT_FOG_H
#define RSRT_FOG_H

#include <stddef.h>
#include <stdint.h>

#include "rsrt_detmath.h"
#include "rsrt_sky.h"   /* rsrt_sky_exp2, rsrt_sky_prepare, RSRT_SKY_LOG2E */
#include "rsrt_types.h" /* rsrt_fog_params */

#define RSRT_FOG_JITTER 1u /* rsrt_fog_params.flags: the march offset xi is drawn per (pixel, sample) instead of 0.5 */
#define RSRT_FOG_MAX_STEPS 64u
/* rsrt_fog_params defaults */
#define RSRT_FOG_DENSITY 0.05f
#define RSRT_FOG_ALBEDO 1.0f /* each channel */
#define RSRT_FOG_ANISOTROPY 0.6f
#define RSRT_FOG_AMBIENT 0.0f /* each channel */
#define RSRT_FOG_MAX_DISTANCE 50.0f
#define RSRT_FOG_STEPS 16u
#define RSRT_FOG_FLAGS RSRT_FOG_JITTER
/* what rsrt_fog_params_ok accepts */
#define RSRT_FOG_MAX_DENSITY 1.0e6f
#define RSRT_FOG_MAX_ANISOTROPY 0.95f
#define RSRT_FOG_UNIT_TOLERANCE 1.0e-3f
#define RSRT_FOG_LARGEST 3.40282346638528859812e38f /* the largest finite float */
#define RSRT_FOG_HEADROOM 0.99f /* of it: what the bounds of one sample's sum and inscatter may reach ("Finiteness" above) */

/* everything that depends on the parameters alone: rsrt_fog_prepare makes it once on the host, the kernel takes it by value */
typedef struct rsrt_fog_constants {
    float sigma2;     /* sigma' = density * log2 e */
    float sigma_s[3]; /* density * albedo */
    float s_amb[3];   /* sigma_s * ambient */
    float phase_norm; /* (1 - g g) / (4 pi) */
    float one_gg;     /* 1 + g g */
    float two_g;      /* 2 g */
    float light_dir[3];
    float light_irradiance[3];
    float max_distance;
    uint32_t steps;
    uint32_t flags;
} rsrt_fog_constants;

/* finite and >= 0 */
RSRT_HD int rsrt_fog_amount(float x) { return x >= 0.0f && x <= RSRT_FOG_LARGEST; }
RSRT_HD int rsrt_fog_unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }

RSRT_HD float rsrt_fog_max3(const float v[3])
{
    const float m = v[0] > v[1] ? v[0] : v[1];
    return m > v[2] ? m : v[2];
}
/* S of "Finiteness" above: no channel's S_sun + S_amb exceeds it.  |anisotropy| <= RSRT_FOG_MAX_ANISOTROPY is the caller's to check */
RSRT_HD float rsrt_fog_source_bound(const rsrt_fog_params *p)
{
    const float g = p->anisotropy, two_a = 2.0f * (g < 0.0f ? -g : g);
    const float q_lo = ((1.0f + g * g) - two_a) - two_a * RSRT_FOG_UNIT_TOLERANCE;
    const float phase_hi = ((1.0f - g * g) / (4.0f * RSRT_PIF)) / (q_lo * rsrt_sqrtf(q_lo));
    const float s = p->density * rsrt_fog_max3(p->albedo);
    return (s * phase_hi) * rsrt_fog_max3(p->light_irradiance) + s * rsrt_fog_max3(p->ambient);
}
/* W_hi of "Finiteness" above: delta times the sum of a march's transmittances does not exceed it */
RSRT_HD float rsrt_fog_length_bound(const rsrt_fog_params *p)
{
    const float delta_hi = p->max_distance / (float)p->steps;
    const float w = delta_hi + 1.0f / (p->density + (p->density * p->density) * (0.5f * delta_hi));
    return w < p->max_distance ? w : p->max_distance;
}
/* one sample's running sum and inscatter stay finite; the ranges of the single fields are the caller's to check first */
RSRT_HD int rsrt_fog_sample_finite(const rsrt_fog_params *p)
{
    const float S = rsrt_fog_source_bound(p), limit = RSRT_FOG_HEADROOM * RSRT_FOG_LARGEST;
    return (float)p->steps * S <= limit && S * rsrt_fog_length_bound(p) <= limit;
}

RSRT_HD int rsrt_fog_params_ok(const rsrt_fog_params *p)
{
    const float len2 = (p->light_dir[0] * p->light_dir[0] + p->light_dir[1] * p->light_dir[1]) + p->light_dir[2] * p->light_dir[2];
    const float off = len2 - 1.0f;
    return p->density >= 0.0f && p->density <= RSRT_FOG_MAX_DENSITY && rsrt_fog_unit_interval(p->albedo[0]) && rsrt_fog_unit_interval(p->albedo[1]) &&
           rsrt_fog_unit_interval(p->albedo[2]) && p->anisotropy >= -RSRT_FOG_MAX_ANISOTROPY && p->anisotropy <= RSRT_FOG_MAX_ANISOTROPY &&
           off >= -RSRT_FOG_UNIT_TOLERANCE && off <= RSRT_FOG_UNIT_TOLERANCE && rsrt_fog_amount(p->light_irradiance[0]) &&
           rsrt_fog_amount(p->light_irradiance[1]) && rsrt_fog_amount(p->light_irradiance[2]) && rsrt_fog_amount(p->ambient[0]) &&
           rsrt_fog_amount(p->ambient[1]) && rsrt_fog_amount(p->ambient[2]) && p->max_distance > 0.0f && p->max_distance <= RSRT_FOG_LARGEST &&
           (p->density * RSRT_SKY_LOG2E) * p->max_distance <= 0.5f * RSRT_FOG_LARGEST && p->steps >= 1u && p->steps <= RSRT_FOG_MAX_STEPS &&
           (p->flags & ~RSRT_FOG_JITTER) == 0u && rsrt_fog_sample_finite(p);
}

/* p must pass rsrt_fog_params_ok */
RSRT_HD void rsrt_fog_prepare(const rsrt_fog_params *p, rsrt_fog_constants *k)
{
    const float g = p->anisotropy;
    k->sigma2 = p->density * RSRT_SKY_LOG2E;
    for (int c = 0; c < 3; c++) {
        k->sigma_s[c] = p->density * p->albedo[c];
        k->s_amb[c] = k->sigma_s[c] * p->ambient[c];
        k->light_dir[c] = p->light_dir[c];
        k->light_irradiance[c] = p->light_irradiance[c];
    }
    k->phase_norm = (1.0f - g * g) / (4.0f * RSRT_PIF);
    k->one_gg = 1.0f + g * g;
    k->two_g = 2.0f * g;
    k->max_distance = p->max_distance;
    k->steps = p->steps;
    k->flags = p->flags;
}

/* the Henyey-Greenstein phase function at cos_theta = d . light_dir */
RSRT_HD float rsrt_fog_cos_theta(const rsrt_fog_constants *k, const float d[3])
{
    return (d[0] * k->light_dir[0] + d[1] * k->light_dir[1]) + d[2] * k->light_dir[2];
}
RSRT_HD float rsrt_fog_phase(const rsrt_fog_constants *k, float cos_theta)
{
    const float q = k->one_gg - k->two_g * cos_theta;
    return k->phase_norm / (q * rsrt_sqrtf(q));
}
/* what a lit march point scatters towards the camera from the light, per unit length */
RSRT_HD void rsrt_fog_sun(const rsrt_fog_constants *k, float phase, float s_sun[3])
{
    for (int c = 0; c < 3; c++) s_sun[c] = (k->sigma_s[c] * phase) * k->light_irradiance[c];
}

/* the marched segment of a camera ray whose closest hit lies at t_hit (hit == 0: it hits nothing) */
RSRT_HD float rsrt_fog_segment(const rsrt_fog_constants *k, int hit, float t_hit) { return (hit && t_hit < k->max_distance) ? t_hit : k->max_distance; }
RSRT_HD float rsrt_fog_delta(const rsrt_fog_constants *k, float L) { return L / (float)k->steps; }
/* march point i: its distance and its position */
RSRT_HD float rsrt_fog_t(uint32_t i, float xi, float delta) { return ((float)i + xi) * delta; }
RSRT_HD void rsrt_fog_point(const float o[3], const float d[3], float t, float x[3])
{
    for (int c = 0; c < 3; c++) x[c] = o[c] + d[c] * t;
}
/* e^(-sigma_t t) */
RSRT_HD float rsrt_fog_transmittance(const rsrt_fog_constants *k, float t) { return rsrt_sky_exp2(-(k->sigma2 * t)); }

/* one march point joins the running sum */
RSRT_HD void rsrt_fog_step(const rsrt_fog_constants *k, float sum[3], float T, int lit, const float s_sun[3])
{
    for (int c = 0; c < 3; c++) sum[c] = sum[c] + T * (lit ? s_sun[c] + k->s_amb[c] : k->s_amb[c]);
}
/* one sample joins the pixel's record: rec = (inscatter rgb, transmittance) */
RSRT_HD void rsrt_fog_record(const rsrt_fog_constants *k, float rec[4], const float sum[3], float delta, float L)
{
    for (int c = 0; c < 3; c++) rec[c] = rec[c] + sum[c] * delta;
    rec[3] = rec[3] + rsrt_fog_transmittance(k, L);
}

/* One sample's march, visibility given: lit[i] != 0 where march point i sees the light.  What the kernel does with the shadow query in
 * the place of lit[i]; the tests' CPU evaluation. */
RSRT_HD void rsrt_fog_sample(const rsrt_fog_constants *k, const float d[3], int hit, float t_hit, float xi, const unsigned char *lit, float rec[4])
{
    const float L = rsrt_fog_segment(k, hit, t_hit), delta = rsrt_fog_delta(k, L);
    float s_sun[3], sum[3] = {0.0f, 0.0f, 0.0f};
    rsrt_fog_sun(k, rsrt_fog_phase(k, rsrt_fog_cos_theta(k, d)), s_sun);
    for (uint32_t i = 0; i < k->steps; i++) rsrt_fog_step(k, sum, rsrt_fog_transmittance(k, rsrt_fog_t(i, xi, delta)), lit[i] != 0, s_sun);
    rsrt_fog_record(k, rec, sum, delta, L);
}

/* the fogged pixel: colour is the source's (already divided by its sample total), rec the pixel's record, n the fog sample total */
RSRT_HD void rsrt_fog_compose(const float colour[3], const float rec[4], float n, float out[3])
{
    const float Tm = rec[3] / n, i0 = rec[0] / n, i1 = rec[1] / n, i2 = rec[2] / n;
    if (Tm == 1.0f && i0 == 0.0f && i1 == 0.0f && i2 == 0.0f) { /* a clear medium: the source itself */
        out[0] = colour[0]; out[1] = colour[1]; out[2] = colour[2];
        return;
    }
    out[0] = colour[0] * Tm + i0;
    out[1] = colour[1] * Tm + i1;
    out[2] = colour[2] * Tm + i2;
}

/* The sun of a procedural sky as the fog's light: dir is rsrt_sky_prepare's sun_dir, irradiance its disc radiance times the widened
 * disc's solid angle 4 pi sin^2(r_eff / 2) — the expression rsrt_sky_prepare divides by, so the widening cancels.  p must pass
 * rsrt_sky_params_ok, env_height > 0 is the map's.  Host only in use. */
RSRT_HD void rsrt_fog_light_from_sky(const rsrt_sky_params *p, uint32_t env_height, float dir[3], float irradiance[3])
{
    rsrt_sky_constants k;
    rsrt_sky_prepare(p, env_height, &k);
    const float half = rsrt_sinf(0.5f * k.r_eff);
    const float omega = (4.0f * RSRT_PIF) * (half * half);
    for (int c = 0; c < 3; c++) {
        dir[c] = k.sun_dir[c];
        irradiance[c] = rsrt_sky_sat(k.sun_radiance[c] * omega);
    }
}

#endif
