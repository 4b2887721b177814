// The volumetric fog pass's arithmetic (csrc/hip/rt_fog.h) run on the CPU over include/rsrt_fog.h, the header the kernels use — built by
// tests/test_fog.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/fog_ref.py).  With
// -DFOG_HOST_MAIN it is a stand-alone program (for a sanitizer build) that runs every function over a few inputs.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rsrt.h"
#include "rsrt_fog.h"

static rsrt_fog_constants constants(const rsrt_fog_params *p)
{
    rsrt_fog_constants k;
    rsrt_fog_prepare(p, &k);
    return k;
}

// out: rsrt_fog_constants' 17 floats in order; words: steps, flags
extern "C" void fog_prepare(const rsrt_fog_params *p, float *out, uint32_t *words)
{
    const rsrt_fog_constants k = constants(p);
    const float v[17] = {k.sigma2, k.sigma_s[0], k.sigma_s[1], k.sigma_s[2], k.s_amb[0], k.s_amb[1], k.s_amb[2], k.phase_norm, k.one_gg, k.two_g,
                         k.light_dir[0], k.light_dir[1], k.light_dir[2], k.light_irradiance[0], k.light_irradiance[1], k.light_irradiance[2], k.max_distance};
    for (int i = 0; i < 17; i++) out[i] = v[i];
    words[0] = k.steps;
    words[1] = k.flags;
}

// d: n directions; cos_out, phase_out: n; sun_out: n * 3
extern "C" void fog_light_term(const rsrt_fog_params *p, const float *d, size_t n, float *cos_out, float *phase_out, float *sun_out)
{
    const rsrt_fog_constants k = constants(p);
    for (size_t i = 0; i < n; i++) {
        cos_out[i] = rsrt_fog_cos_theta(&k, d + 3 * i);
        phase_out[i] = rsrt_fog_phase(&k, cos_out[i]);
        rsrt_fog_sun(&k, phase_out[i], sun_out + 3 * i);
    }
}

// the phase function at given cosines
extern "C" void fog_phase(const rsrt_fog_params *p, const float *cos_theta, size_t n, float *out)
{
    const rsrt_fog_constants k = constants(p);
    for (size_t i = 0; i < n; i++) out[i] = rsrt_fog_phase(&k, cos_theta[i]);
}

// march point `step` of n rays: seg_out, delta_out, t_out, trans_out (of t), trans_seg_out (of the segment): n; x_out: n * 3
extern "C" void fog_march_point(const rsrt_fog_params *p, const float *o, const float *d, const int *hit, const float *t_hit, const float *xi, uint32_t step,
                                size_t n, float *seg_out, float *delta_out, float *t_out, float *x_out, float *trans_out, float *trans_seg_out)
{
    const rsrt_fog_constants k = constants(p);
    for (size_t i = 0; i < n; i++) {
        seg_out[i] = rsrt_fog_segment(&k, hit[i], t_hit[i]);
        delta_out[i] = rsrt_fog_delta(&k, seg_out[i]);
        t_out[i] = rsrt_fog_t(step, xi[i], delta_out[i]);
        rsrt_fog_point(o + 3 * i, d + 3 * i, t_out[i], x_out + 3 * i);
        trans_out[i] = rsrt_fog_transmittance(&k, t_out[i]);
        trans_seg_out[i] = rsrt_fog_transmittance(&k, seg_out[i]);
    }
}

// one sample of n rays joins rec (n * 4, in and out); lit: n * steps bytes
extern "C" void fog_sample(const rsrt_fog_params *p, const float *d, const int *hit, const float *t_hit, const float *xi, const unsigned char *lit, size_t n,
                           float *rec)
{
    const rsrt_fog_constants k = constants(p);
    for (size_t i = 0; i < n; i++) rsrt_fog_sample(&k, d + 3 * i, hit[i], t_hit[i], xi[i], lit + (size_t)k.steps * i, rec + 4 * i);
}

// colour: n * 3 (already divided by its sample total); rec: n * 4; out: n * 4, alpha 1
extern "C" void fog_compose(const float *colour, const float *rec, float fog_total, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) {
        rsrt_fog_compose(colour + 3 * i, rec + 4 * i, fog_total, out + 4 * i);
        out[4 * i + 3] = 1.0f;
    }
}

extern "C" int fog_light_from_sky(const rsrt_sky_params *p, uint32_t env_height, float *dir, float *irradiance)
{
    if (!rsrt_sky_params_ok(p) || env_height == 0) return 1;
    rsrt_fog_light_from_sky(p, env_height, dir, irradiance);
    return 0;
}

extern "C" int fog_params_ok(const rsrt_fog_params *p) { return rsrt_fog_params_ok(p); }

extern "C" void fog_defaults(rsrt_fog_params *p)
{
    *p = rsrt_fog_params{RSRT_FOG_DENSITY, {RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO}, RSRT_FOG_ANISOTROPY, {0.0f, 1.0f, 0.0f}, {1.0f, 1.0f, 1.0f},
                         {RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT}, RSRT_FOG_MAX_DISTANCE, RSRT_FOG_STEPS, RSRT_FOG_FLAGS};
}

// size of rsrt_fog_params, then the offsets of albedo, anisotropy, light_dir, light_irradiance, ambient, max_distance, steps, flags;
// RSRT_FOG_MAX_STEPS; RSRT_FOG_JITTER; RSRT_EXPOSURE_FOG; size of rsrt_fog_constants
extern "C" void fog_layout(uint32_t *out /* 13 */)
{
    const size_t v[13] = {sizeof(rsrt_fog_params), offsetof(rsrt_fog_params, albedo), offsetof(rsrt_fog_params, anisotropy), offsetof(rsrt_fog_params, light_dir),
                          offsetof(rsrt_fog_params, light_irradiance), offsetof(rsrt_fog_params, ambient), offsetof(rsrt_fog_params, max_distance),
                          offsetof(rsrt_fog_params, steps), offsetof(rsrt_fog_params, flags), RSRT_FOG_MAX_STEPS, RSRT_FOG_JITTER, RSRT_EXPOSURE_FOG,
                          sizeof(rsrt_fog_constants)};
    for (int i = 0; i < 13; i++) out[i] = (uint32_t)v[i];
}

#ifdef FOG_HOST_MAIN
int main()
{
    rsrt_fog_params p;
    fog_defaults(&p);
    p.ambient[1] = 0.25f;
    double sum = 0.0;
    for (uint32_t steps : {1u, 7u, 64u}) {
        p.steps = steps;
        if (!fog_params_ok(&p)) return 1;
        const size_t n = 33;
        std::vector<float> o(3 * n, 0.5f), d(3 * n), t_hit(n), xi(n), rec(4 * n, 0.0f), colour(3 * n, 0.75f), out(4 * n), a(n), b(n), c(n), x(3 * n), e(n), f(n);
        std::vector<int> hit(n);
        std::vector<unsigned char> lit(n * steps);
        for (size_t i = 0; i < n; i++) {
            d[3 * i] = 0.6f; d[3 * i + 1] = (i % 2) ? 0.8f : -0.8f; d[3 * i + 2] = 0.0f;
            hit[i] = (int)(i % 3 != 0);
            t_hit[i] = 0.5f * (float)i;
            xi[i] = (float)i / (float)(n - 1);
            for (uint32_t j = 0; j < steps; j++) lit[i * steps + j] = (unsigned char)((i + j) % 2);
        }
        fog_march_point(&p, o.data(), d.data(), hit.data(), t_hit.data(), xi.data(), steps - 1u, n, a.data(), b.data(), c.data(), x.data(), e.data(), f.data());
        fog_sample(&p, d.data(), hit.data(), t_hit.data(), xi.data(), lit.data(), n, rec.data());
        fog_compose(colour.data(), rec.data(), 1.0f, n, out.data());
        for (float v : out) sum += v;
        for (float v : x) sum += v;
    }
    const rsrt_sky_params sky = {RSRT_SKY_SUN_AZIMUTH, RSRT_SKY_SUN_ELEVATION, RSRT_SKY_TURBIDITY, {0.2f, 0.2f, 0.2f}, RSRT_SKY_SCALE, RSRT_SKY_SUN_ILLUMINANCE,
                                 RSRT_SKY_SUN_RADIUS, RSRT_SKY_FLAGS};
    float dir[3], irr[3];
    if (fog_light_from_sky(&sky, 512u, dir, irr)) return 1;
    std::printf("%.9g %.9g %.9g\n", sum, (double)dir[1], (double)irr[0]);
    return 0;
}
#endif
