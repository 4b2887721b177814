/*
 * rsrt_variance.h — per-pixel arithmetic of the variance-guided filter and the firefly clamp (rsrt_denoise with RSRT_DENOISE_VARIANCE
 * and RSRT_DENOISE_CLAMP, include/rsrt.h), as shared inline code.
 *
 * The variance guidance follows SVGF (Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017): the a-trous filter's colour
 * term compares luminance against a per-pixel estimate of its noise instead of a fixed sigma, so a pixel with much history is filtered
 * little and a fresh one much.  Like rsrt_denoise.h this is part of the published numeric contract: plain f32 + - * / (-ffp-contract=off,
 * nothing fused), every sum in a fixed order, so that a numpy float32 restatement reproduces the GPU output bit for bit
 * (tests/variance_ref.py, tests/test_variance.py).
 *
 * lum(x) = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b.  r_p is the filter's input of rsrt_denoise.h (demodulated: r = c / max(a, eps)).
 *
 * Clamp (CLAMP).  Lmax = max(0, lum(r_q)) over the 8 neighbours q of p inside the image, of the unclamped input.  If lum(r_p) > Lmax,
 *   r_p <- r_p (Lmax / lum(r_p)): an isolated firefly becomes as bright as its brightest neighbour; anything that is not a strict local
 *   maximum is untouched, and so is the pixel of a 1 x 1 image (no neighbour).
 * Variance (VARIANCE).  Moment records m = (mu1, mu2, frames, scale): the temporal pass's (RSRT_TEMPORAL_MOMENTS, rsrt_temporal.h), or
 *   (l, l l, 1, 1) with l = lum of the unclamped r_p.
 *   frames >= RSRT_SV_MIN_FRAMES: v = scale max(mu2 - mu1 mu1, 0).
 *   otherwise the spatial estimate over the 7 x 7 window (dy outer, dx inner, taps outside the image skipped):
 *     w_q = 1 / (dn dz) with the filter's normal and depth terms (rsrt_denoise.h, from the packed features, kz of p's depth),
 *     mu_k = (sum w_q mu_k(q)) / (sum w_q), v = scale_p max(mu_2 - mu_1 mu_1, 0).
 * Level i (VARIANCE), step 2^i, the 5 x 5 B3 spline of rsrt_denoise.h, on (r, v):
 *   g_p   = (sum k v_q) / (sum k) over the 3 x 3 neighbourhood inside the image, k = [1, 2, 1] x [1, 2, 1] (dy outer, dx inner)
 *   kl    = 1 / ((sigma_l sigma_l) g_p + RSRT_SV_EPS)         sigma_l = rsrt_denoise_params.sigma_color under VARIANCE
 *   dl    = 1 + ((lum(r_q) - lum(r_p))^2) kl
 *   w_q   = h_dx h_dy / ((dl dn) dz)
 *   r'_p  = (sum w r_q) / (sum w),  v'_p = (sum (w w) v_q) / ((sum w) (sum w))
 * After the last level r' is remodulated as in rsrt_denoise.h.
 */
#ifndef RSRT_VARIANCE_H
#define RSRT_VARIANCE_H

#include "rsrt_denoise.h"

#define RSRT_SV_MIN_FRAMES 4.0f /* below this many frames of history the variance is estimated spatially */
#define RSRT_SV_EPS 1.0e-6f     /* keeps the luminance term finite where the variance is 0 */
#define RSRT_SV_SIGMA_L 4.0f    /* default sigma_color under VARIANCE (SVGF's sigma_l) */
#define RSRT_SV_RADIUS 3        /* the spatial estimate's window: 7 x 7 */

RSRT_HD float rsrt_sv_lum(const float x[3]) { return (0.2126f * x[0] + 0.7152f * x[1]) + 0.0722f * x[2]; }

/* the luminance of one frame's demodulated mean colour (rsrt_dn_prepare with demodulation) */
RSRT_HD float rsrt_sv_frame_lum(const float sum[3], float sample_total, const float aov[8], float aov_total)
{
    float r[3];
    rsrt_dn_prepare(sum, sample_total, aov, aov_total, 1, r);
    return rsrt_sv_lum(r);
}

/* the clamp of r (in place); lmax: max(0, the neighbours' luminance), have: p has a neighbour inside the image */
RSRT_HD void rsrt_sv_clamp(float r[3], float lmax, int have)
{
    const float l = rsrt_sv_lum(r);
    if (have && l > lmax) {
        const float s = lmax / l;
        for (int i = 0; i < 3; i++) r[i] = r[i] * s;
    }
}

/* one tap q of the spatial estimate at p: adds w mu1_q, w mu2_q and w into acc */
RSRT_HD void rsrt_sv_spatial_tap(const float fp[4], float kn, float kz, const float fq[4], float mu1, float mu2, float acc[3])
{
    const float n0 = fq[0] - fp[0], n1 = fq[1] - fp[1], n2 = fq[2] - fp[2];
    const float z0 = fq[3] - fp[3];
    const float dn = 1.0f + ((n0 * n0 + n1 * n1) + n2 * n2) * kn;
    const float dz = 1.0f + (z0 * z0) * kz;
    const float w = 1.0f / (dn * dz);
    acc[0] = acc[0] + w * mu1;
    acc[1] = acc[1] + w * mu2;
    acc[2] = acc[2] + w;
}

RSRT_HD int rsrt_sv_temporal_enough(const float m[4]) { return m[2] >= RSRT_SV_MIN_FRAMES; }

/* p's variance from its record m and, when !rsrt_sv_temporal_enough(m), the spatial sums */
RSRT_HD float rsrt_sv_variance(const float m[4], const float spatial[3])
{
    float mu1 = m[0], mu2 = m[1];
    if (!rsrt_sv_temporal_enough(m)) {
        mu1 = spatial[0] / spatial[2];
        mu2 = spatial[1] / spatial[2];
    }
    const float d = mu2 - mu1 * mu1;
    return m[3] * (d > 0.0f ? d : 0.0f);
}

/* taps of the 3 x 3 binomial blur of v: [1, 2, 1] */
RSRT_HD float rsrt_sv_binomial(int k) { return k == 0 ? 2.0f : 1.0f; }

/* the level's luminance constant from the blurred variance g_p */
RSRT_HD float rsrt_sv_kl(float sigma_l, float g) { return 1.0f / ((sigma_l * sigma_l) * g + RSRT_SV_EPS); }

/* one tap q of pixel p: adds w r_q, w and (w w) v_q into acc (rgb, weight, variance) */
RSRT_HD void rsrt_sv_tap(float h, float lp, const float fp[4], float kl, float kn, float kz, const float rq[3], float vq,
                         const float fq[4], float acc[5])
{
    const float dlum = rsrt_sv_lum(rq) - lp;
    const float n0 = fq[0] - fp[0], n1 = fq[1] - fp[1], n2 = fq[2] - fp[2];
    const float z0 = fq[3] - fp[3];
    const float dl = 1.0f + (dlum * dlum) * kl;
    const float dn = 1.0f + ((n0 * n0 + n1 * n1) + n2 * n2) * kn;
    const float dz = 1.0f + (z0 * z0) * kz;
    const float w = h / ((dl * dn) * dz);
    acc[0] = acc[0] + w * rq[0];
    acc[1] = acc[1] + w * rq[1];
    acc[2] = acc[2] + w * rq[2];
    acc[3] = acc[3] + w;
    acc[4] = acc[4] + (w * w) * vq;
}

/* end of a level: the weighted mean (remodulated after the last level) and the filtered variance */
RSRT_HD void rsrt_sv_finish(const float acc[5], const float a[3], int remodulate, float out[4])
{
    rsrt_dn_finish(acc, a, remodulate, out);
    out[3] = acc[4] / (acc[3] * acc[3]);
}

#endif
