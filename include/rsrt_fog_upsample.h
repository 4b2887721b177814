/*
 * rsrt_fog_upsample.h — arithmetic of the fog rebuild (rsrt_fog_apply_upsampled in include/rsrt.h), as shared inline code.
 *
 * The fog records are marched at a low size w x h (rsrt_fog_render with a size of its own) and the fog image of the output size W x H
 * (W >= w, H >= h) is rebuilt from them and from first-hit records of the OUTPUT size: the AOV buffer, or the guide for the upsampled
 * image.  The pattern is rsrt_upsample.h's: the smooth quantity comes from the low frame, the edges from the full-size records.  Like
 * rsrt_fog.h this is part of the published numeric contract: plain f32 + - * /, compares and rsrt_sky_exp2 (-ffp-contract=off, nothing
 * fused) in exactly the order written here, so a numpy restatement reproduces every bit (tests/fog_upsample_ref.py holds it).
 *
 * Inscatter is not smooth across a depth edge: it grows with the marched length.  Divided by 1 - transmittance it is the mean source
 * term along the ray, which for lit fog is almost the same on both sides of the edge.  So that quotient is what is upsampled, and the
 * output pixel's own transmittance, which its first-hit record gives exactly, multiplies it back.
 *
 * Per low pixel q, with n the fog sample total (rsrt_fogup_source):
 *   m[c]   = rec_q[c] / n                                   c = 0 .. 3: mean inscatter rgb, mean transmittance
 *   one    = 1 - m[3]
 *   s_q[c] = one > 0 ? min(m[c] / one, RSRT_FOGUP_SOURCE_MAX) : 0
 * The clamp, 2^120, keeps the nine-tap sum finite for every record the fog pass can write (an inscatter sum may be inf, one as small as
 * 2^-24), so that s * 0 below is never inf * 0.  A clear medium (one == 0) has no source term.
 * Per output pixel P = (X, Y), with g its first-hit record of T samples, g[3] the hit count and g[7] the sum of the hit distances, and
 * k the rsrt_fog_constants of the parameters the records were rendered with, of which sigma2 and max_distance are read (rsrt_fogup_tau):
 *   e_far = rsrt_fog_transmittance(k, k.max_distance)
 *   hits  = g[3];  when hits > 0:  d = g[7] / hits,  e_hit = rsrt_fog_transmittance(k, rsrt_fog_segment(k, 1, d))
 *   tau   = e_hit                                           when hits >= T
 *           e_far                                           when hits is not > 0
 *           (hits * e_hit + (T - hits) * e_far) / T         otherwise
 * At T = 1 tau is bit for bit the transmittance rsrt_fog_record adds for the sample the record holds.
 *   u, v, xn, yn                                            rsrt_up_coord, rsrt_up_nearest of (X, w, W) and (Y, h, H)
 *   taps q = (xn + dx, yn + dy), dy = -1..1 outer, dx = -1..1 inner; taps outside the low frame are skipped (rsrt_fogup_tap):
 *     hs = rsrt_up_tent(qx, u) * rsrt_up_tent(qy, v);   acc[c] = acc[c] + hs * s_q[c];   acc[3] = acc[3] + hs
 *   S[c] = acc[c] / acc[3];   I[c] = S[c] * (1 - tau);   out = rsrt_fog_compose(colour, {I, tau}, 1)              (rsrt_fogup_finish)
 * There is no fallback for an empty weight sum because there is none: |xn - u| <= 1/2, so the three taps of an axis lie within 3/2 of
 * u and each tent is 1/4 or more, each weight 1/16 or more; and xn lies in 0 .. w (u < w), so xn - 1, xn or both are inside the frame.
 * Nor is there an edge-stopping weight: on top of the demodulation it made a prototype's error larger at every strength tried.
 *
 * With density 0 every s_q is 0 and tau is exactly 1 (rsrt_sky_exp2(-0) == 1, and (hits + (T - hits)) / T == 1), so I == 0 and
 * rsrt_fog_compose returns the source's colour itself, a negative zero included.
 * Equal sizes are allowed and are NOT the identity: u = X, the taps X - 1, X, X + 1 weigh 1/2, 1, 1/2 an axis — a 3 x 3 tent over
 * the demodulated records.  rsrt_fog_apply is the call that composes records of the source's size as they are.
 */
#ifndef RSRT_FOG_UPSAMPLE_H
#define RSRT_FOG_UPSAMPLE_H

#include "rsrt_fog.h"
#include "rsrt_upsample.h" /* rsrt_up_coord, rsrt_up_nearest, rsrt_up_tent */

#define RSRT_FOGUP_SOURCE_MAX 1.329227995784915872903807060280344576e36f /* 2^120 */

/* the demodulated record of a low pixel: mean inscatter / (1 - mean transmittance) */
RSRT_HD void rsrt_fogup_source(const float rec[4], float n, float s[3])
{
    const float m3 = rec[3] / n;
    const float one = 1.0f - m3;
    for (int c = 0; c < 3; c++) {
        const float m = rec[c] / n;
        if (one > 0.0f) {
            const float q = m / one;
            s[c] = q < RSRT_FOGUP_SOURCE_MAX ? q : RSRT_FOGUP_SOURCE_MAX;
        } else {
            s[c] = 0.0f;
        }
    }
}

/* the transmittance of an output pixel from its first-hit record g (8 floats) of T samples */
RSRT_HD float rsrt_fogup_tau(const rsrt_fog_constants *k, const float g[8], float T)
{
    const float e_far = rsrt_fog_transmittance(k, k->max_distance);
    const float hits = g[3];
    if (!(hits > 0.0f)) return e_far;
    const float d = g[7] / hits;
    const float e_hit = rsrt_fog_transmittance(k, rsrt_fog_segment(k, 1, d));
    if (hits >= T) return e_hit;
    return (hits * e_hit + (T - hits) * e_far) / T;
}

/* one tap q of output pixel P: adds hs * s_q and hs into acc (rgb, weight) */
RSRT_HD void rsrt_fogup_tap(float hs, const float sq[3], float acc[4])
{
    acc[0] = acc[0] + hs * sq[0];
    acc[1] = acc[1] + hs * sq[1];
    acc[2] = acc[2] + hs * sq[2];
    acc[3] = acc[3] + hs;
}

/* the fogged pixel: colour is the source's (already divided by its sample total), acc the taps' sums, tau the pixel's transmittance */
RSRT_HD void rsrt_fogup_finish(const float colour[3], const float acc[4], float tau, float out[3])
{
    const float rest = 1.0f - tau;
    float r[4];
    for (int c = 0; c < 3; c++) r[c] = (acc[c] / acc[3]) * rest;
    r[3] = tau;
    rsrt_fog_compose(colour, r, 1.0f, out);
}

/* One output pixel from low-frame source terms, as the kernel computes it: src is the w x h frame of rsrt_fogup_source's results, 4
 * floats a pixel (the fourth is not read).  The tests' CPU evaluation. */
RSRT_HD void rsrt_fogup_pixel(const rsrt_fog_constants *k, const float *src, uint32_t w, uint32_t h, uint32_t X, uint32_t Y, uint32_t W, uint32_t H,
                              const float g[8], float T, const float colour[3], float out[3])
{
    const float u = rsrt_up_coord(X, w, W), v = rsrt_up_coord(Y, h, H);
    const int xn = rsrt_up_nearest(u), yn = rsrt_up_nearest(v);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = yn + dy;
        if (qy < 0 || qy >= (int)h) continue;
        const float hy = rsrt_up_tent(qy, v);
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = xn + dx;
            if (qx < 0 || qx >= (int)w) continue;
            const float hx = rsrt_up_tent(qx, u);
            rsrt_fogup_tap(hx * hy, src + 4u * ((size_t)qy * w + (size_t)qx), acc);
        }
    }
    rsrt_fogup_finish(colour, acc, rsrt_fogup_tau(k, g, T), out);
}

#endif
