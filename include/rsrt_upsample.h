/*
 * rsrt_upsample.h — per-pixel arithmetic of the guided upsampling (rsrt_upsample, include/rsrt.h), as shared inline code.
 *
 * The path samples are traced at a low size w x h; the picture of the output size W x H (W >= w, H >= h) is rebuilt from them with
 * a joint-bilateral upsample guided by first-hit records of the OUTPUT size (rsrt_guide_render): the demodulated colour is smooth,
 * the edges and the albedo's detail live in the guide.  Like rsrt_denoise.h this is part of the published numeric contract: plain
 * f32 + - * / (-ffp-contract=off, nothing fused), every sum in a fixed order, so that a numpy float32 restatement reproduces the
 * GPU output bit for bit (tests/upsample_ref.py holds it).  The demodulation, the features and the edge constants are the
 * denoiser's (rsrt_dn_*).
 *
 * A render's pixel p is centred at p / res (the jitter is a disc around the integer coordinate, no + 0.5), so output pixel X sits
 * at the low coordinate X * w / W.
 *
 * Low pass, per low pixel q, with S = sample_total and T = aov_sample_total (what the denoiser's prepare pass writes):
 *   r_q = rsrt_dn_prepare(colour_q, S, aov_q, T, demodulate)        the demodulated mean (or the mean)
 *   f_q = binary16(rsrt_dn_features(aov_q, T))                       mean normal, mean distance
 * High pass, per output pixel P = (X, Y), with Tg = guide_sample_total:
 *   u   = (X * w) / W,  v = (Y * h) / H                              rsrt_up_coord
 *   xn  = floor(u + 0.5), yn = floor(v + 0.5)                        rsrt_up_nearest
 *   f_P = binary16(rsrt_dn_features(guide_P, Tg)),  a_P = rsrt_dn_albedo(guide_P, Tg)
 *   taps q = (xn + dx, yn + dy), dy = -1..1 outer, dx = -1..1 inner; taps outside the low frame are skipped:
 *     hx = 1 - |qx - u| / 2,  hy = 1 - |qy - v| / 2                  a tent of radius 2: all nine taps weigh >= 1 / 16, so the
 *                                                                    edge terms always have a choice
 *     w_q = hx hy / (dn * dz)                                        dn, dz: the denoiser's normal and relative-depth terms
 *   r   = (sum_q w_q r_q) / (sum_q w_q)    when the weight sum is > 0,
 *         r of the nearest low pixel (min(xn, w - 1), min(yn, h - 1)) otherwise: a zero or NaN weight sum, e.g. from features
 *         that pack to inf
 *   out = demodulate ? r * a_P : r
 * There is no colour term: no colour of the output size exists.
 */
#ifndef RSRT_UPSAMPLE_H
#define RSRT_UPSAMPLE_H

#include "rsrt_denoise.h"

#define RSRT_UP_SIGMA_NORMAL 0.5f /* rsrt_upsample_params defaults */
#define RSRT_UP_SIGMA_DEPTH 0.3f
#define RSRT_UP_MAX_SIZE 16384u   /* largest guide / output width and height */

/* the low coordinate of output pixel X of `out_size`, for a low frame of `low_size` pixels */
RSRT_HD float rsrt_up_coord(uint32_t X, uint32_t low_size, uint32_t out_size) { return ((float)X * (float)low_size) / (float)out_size; }
/* the nearest low pixel of a low coordinate (may be low_size: its taps at and beyond it are skipped) */
RSRT_HD int rsrt_up_nearest(float u) { return (int)floorf(u + 0.5f); }
/* the tent of radius 2 */
RSRT_HD float rsrt_up_tent(int q, float u)
{
    const float d = (float)q - u;
    return 1.0f - (d < 0.0f ? -d : d) * 0.5f;
}

/* one tap q of output pixel P: adds w * r_q and w into acc (rgb, weight) */
RSRT_HD void rsrt_up_tap(float hs, const float fp[4], float kn, float kz, const float rq[3], const float fq[4], float acc[4])
{
    const float n0 = fq[0] - fp[0], n1 = fq[1] - fp[1], n2 = fq[2] - fp[2];
    const float z0 = fq[3] - fp[3];
    const float dn = 1.0f + ((n0 * n0 + n1 * n1) + n2 * n2) * kn;
    const float dz = 1.0f + (z0 * z0) * kz;
    const float w = hs / (dn * dz);
    acc[0] = acc[0] + w * rq[0];
    acc[1] = acc[1] + w * rq[1];
    acc[2] = acc[2] + w * rq[2];
    acc[3] = acc[3] + w;
}

/* the weighted mean, or the nearest low pixel's value when the weights sum to nothing; times the guide's albedo (remodulate != 0) */
RSRT_HD void rsrt_up_finish(const float acc[4], const float nearest[3], const float a[3], int remodulate, float out[3])
{
    const int ok = acc[3] > 0.0f;
    for (int i = 0; i < 3; i++) {
        const float r = ok ? acc[i] / acc[3] : nearest[i];
        out[i] = remodulate ? r * a[i] : r;
    }
}

#endif
