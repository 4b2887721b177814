/*
 * rsrt_denoise.h — per-pixel arithmetic of the denoiser (rsrt_denoise, include/rsrt.h), as shared inline code.
 *
 * An edge-aware a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, "Edge-Avoiding A-Trous Wavelet Transform for
 * fast Global Illumination Filtering", HPG 2010) guided by the first-hit buffers of rsrt_aov_render.  Like
 * rsrt_tonemap.h this is part of the published numeric contract: plain f32 + - * / (-ffp-contract=off, nothing fused,
 * no exp, no hardware approximation), every sum in a fixed order, so that a numpy float32 restatement reproduces the
 * GPU output bit for bit (tests/test_denoise.py holds it).
 *
 * Per pixel p, with S = sample_total and T = aov_sample_total:
 *   c_p   = sum_p / S                                      the noisy mean (rsrt_display_srgb8's input)
 *   a_p   = (albedo_sum_p + (T - hits_p)) / T              mean first-hit albedo; a sample that hit nothing counts as 1
 *   n_p   = normal_sum_p / T,  z_p = distance_sum_p / T    mean first-hit normal and distance (a miss counts as 0),
 *                                                          both stored as binary16 (the packed features one tap reads);
 *                                                          z_p saturates at RSRT_DN_DEPTH_MAX first, so that a far pixel
 *                                                          packs to a finite depth instead of inf (inf - inf = NaN in dz)
 *   r_p   = c_p / max(a_p, RSRT_DN_ALBEDO_EPS)             demodulated (RSRT_DENOISE_DEMODULATE; otherwise r_p = c_p)
 * Level i = 0 .. L-1, step 2^i, taps q = p + 2^i (dx, dy), dx, dy in -2..2, dy outer, dx inner; taps outside the image
 * are skipped:
 *   w_q   = h_dx h_dy / ((dc * dn) * dz)                   h = [1, 4, 6, 4, 1] / 16
 *   dc    = 1 + |r_q - r_p|^2 * 4^i / sigma_c^2            (the rational edge-stopping functions 1 / (1 + x) of the
 *   dn    = 1 + |n_q - n_p|^2 / sigma_n^2                   colour, normal and relative depth, multiplied before the
 *   dz    = 1 + (z_q - z_p)^2 / (sigma_z^2 (z_p^2 + 1e-4))  one division)
 *   r'_p  = (sum_q w_q r_q) / (sum_q w_q)                  the centre tap has w = 36 / 256 > 0
 * After the last level the result is remodulated, out_p = r'_p * a_p.  L = 0 returns c_p exactly.
 */
#ifndef RSRT_DENOISE_H
#define RSRT_DENOISE_H

#include "rsrt_detmath.h"

#define RSRT_DN_ALBEDO_EPS 1.0e-3f /* demodulation divides by max(albedo, this) */
#define RSRT_DN_DEPTH_EPS 1.0e-4f  /* keeps the relative-depth scale finite where nothing was hit (z = 0) */
#define RSRT_DN_DEPTH_MAX 65504.0f /* the largest finite binary16: the packed mean distance saturates here */

/* taps of the B3 spline: [1, 4, 6, 4, 1] / 16, exact in f32 */
RSRT_HD float rsrt_dn_b3(int k) { return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f); }

/* mean albedo of the first hits, a miss counting as 1 */
RSRT_HD void rsrt_dn_albedo(const float aov[8], float aov_total, float a[3])
{
    const float miss = aov_total - aov[3];
    for (int i = 0; i < 3; i++) a[i] = (aov[i] + miss) / aov_total;
}

/* the guide features before their binary16 packing: mean normal xyz, mean distance (saturated at RSRT_DN_DEPTH_MAX) */
RSRT_HD void rsrt_dn_features(const float aov[8], float aov_total, float f[4])
{
    for (int i = 0; i < 4; i++) f[i] = aov[4 + i] / aov_total;
    f[3] = f[3] > RSRT_DN_DEPTH_MAX ? RSRT_DN_DEPTH_MAX : f[3];
}

/* the filtered quantity of one pixel */
RSRT_HD void rsrt_dn_prepare(const float sum[3], float sample_total, const float aov[8], float aov_total, int demodulate, float r[3])
{
    float a[3];
    rsrt_dn_albedo(aov, aov_total, a);
    for (int i = 0; i < 3; i++) {
        const float c = sum[i] / sample_total;
        const float d = a[i] < RSRT_DN_ALBEDO_EPS ? RSRT_DN_ALBEDO_EPS : a[i];
        r[i] = demodulate ? c / d : c;
    }
}

/* per-level colour constant 4^i / sigma_c^2, and the normal constant 1 / sigma_n^2 */
RSRT_HD float rsrt_dn_kc(float sigma_c, unsigned level)
{
    float s = 1.0f;
    for (unsigned i = 0; i < level; i++) s = s * 4.0f;
    return s / (sigma_c * sigma_c);
}
RSRT_HD float rsrt_dn_kn(float sigma_n) { return 1.0f / (sigma_n * sigma_n); }
/* the centre pixel's depth constant */
RSRT_HD float rsrt_dn_kz(float sigma_z, float zp) { return 1.0f / ((sigma_z * sigma_z) * (zp * zp + RSRT_DN_DEPTH_EPS)); }

/* one tap q of pixel p: adds w * r_q and w into acc (rgb, weight) */
RSRT_HD void rsrt_dn_tap(float h, const float rp[3], const float fp[4], float kc, float kn, float kz, const float rq[3], const float fq[4],
                         float acc[4])
{
    const float c0 = rq[0] - rp[0], c1 = rq[1] - rp[1], c2 = rq[2] - rp[2];
    const float n0 = fq[0] - fp[0], n1 = fq[1] - fp[1], n2 = fq[2] - fp[2];
    const float z0 = fq[3] - fp[3];
    const float dc = 1.0f + ((c0 * c0 + c1 * c1) + c2 * c2) * kc;
    const float dn = 1.0f + ((n0 * n0 + n1 * n1) + n2 * n2) * kn;
    const float dz = 1.0f + (z0 * z0) * kz;
    const float w = h / ((dc * dn) * dz);
    acc[0] = acc[0] + w * rq[0];
    acc[1] = acc[1] + w * rq[1];
    acc[2] = acc[2] + w * rq[2];
    acc[3] = acc[3] + w;
}

/* end of a level: the weighted mean; after the last one (remodulate != 0) times the albedo */
RSRT_HD void rsrt_dn_finish(const float acc[4], const float a[3], int remodulate, float out[3])
{
    for (int i = 0; i < 3; i++) {
        const float m = acc[i] / acc[3];
        out[i] = remodulate ? m * a[i] : m;
    }
}

#endif
