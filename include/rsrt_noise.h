/*
 * rsrt_noise.h — arithmetic of the noise estimate (rsrt_noise_estimate, include/rsrt.h), as shared inline code.
 *
 * The accumulator sums a pixel's samples in increasing order, so a copy of it taken at n1 samples (rsrt_noise_snapshot) and the
 * accumulator itself at n2 > n1 samples hold two estimates of every pixel: the first n1 samples and all n2.  This is the half
 * buffer of Dammertz, Hanika, Keller, Lensch, "A Hierarchical Automatic Stopping Condition for Monte Carlo Global Illumination"
 * (WSCG 2010); it costs one device copy and no extra ray.  Like rsrt_denoise.h this is part of the published numeric contract:
 * plain f32 + - * /, rsrt_sqrtf (-ffp-contract=off, nothing fused), every sum in a fixed order, so that a numpy float32
 * restatement reproduces the GPU output bit for bit (tests/noise_ref.py holds it).
 *
 * Per pixel, with the snapshot's sum S1 of n1 samples and the accumulator's sum S2 of n2 samples:
 *   a   = S1.rgb / n1,  m = S2.rgb / n2
 *   num = (|m.r - a.r| + |m.g - a.g|) + |m.b - a.b|
 *   s   = (m.r + m.g) + m.b
 *   e   = num / rsrt_sqrtf(max(s, 0) + RSRT_NOISE_EPS)         a NaN e becomes +inf: a pixel with non-finite radiance never
 *                                                              counts as converged
 * With n1 = n2 / 2, m - a is half the difference of the two halves, so e estimates the error of m itself.
 *
 * Per tile of tile_w x tile_h pixels (T = tile_w * tile_h a multiple of 64, at most 4096: the partition's rule), a pixel's index
 * inside its tile being i = y * tile_w + x:
 *   v_l = ((0 + e_l) + e_(l+64)) + ...                         lane l of 64, increasing i; pixels outside the frame add nothing
 *   v   = v + v[l xor k]  for k = 32, 16, 8, 4, 2, 1            six butterfly steps; f32 addition commutes, so all lanes agree
 *   tile_error = v / (float)count                              count: the tile's pixels inside the frame (edge tiles are partial)
 * Over the tile map in row-major order (rsrt_noise_download, on the host): the maximum, the mean as a sequential f32 sum divided
 * by the tile count, and the number of tiles with error > threshold, an infinite error always counting.
 */
#ifndef RSRT_NOISE_H
#define RSRT_NOISE_H

#include "rsrt_detmath.h"

#define RSRT_NOISE_EPS 1.0e-3f  /* keeps the relative error finite on black */
#define RSRT_NOISE_TILE_W 16u   /* rsrt_noise_params defaults */
#define RSRT_NOISE_TILE_H 16u
#define RSRT_NOISE_TILE_MAX 4096u /* most pixels a tile may hold; the count is a multiple of 64 */

RSRT_HD float rsrt_noise_abs(float x) { return __builtin_fabsf(x); }
RSRT_HD float rsrt_noise_inf() { return __builtin_inff(); }

/* the error estimate of one pixel from the snapshot's sum of n1 samples and the accumulator's sum of n2 */
RSRT_HD float rsrt_noise_pixel(const float s1[3], float n1, const float s2[3], float n2)
{
    const float a0 = s1[0] / n1, a1 = s1[1] / n1, a2 = s1[2] / n1;
    const float m0 = s2[0] / n2, m1 = s2[1] / n2, m2 = s2[2] / n2;
    const float num = (rsrt_noise_abs(m0 - a0) + rsrt_noise_abs(m1 - a1)) + rsrt_noise_abs(m2 - a2);
    const float s = (m0 + m1) + m2;
    const float e = num / rsrt_sqrtf((s > 0.0f ? s : 0.0f) + RSRT_NOISE_EPS);
    return e == e ? e : rsrt_noise_inf();
}

/* is w x h a tile the estimate takes? */
RSRT_HD int rsrt_noise_tile_ok(uint32_t w, uint32_t h)
{
    return w != 0 && h != 0 && w <= RSRT_NOISE_TILE_MAX && h <= RSRT_NOISE_TILE_MAX && w * h <= RSRT_NOISE_TILE_MAX && (w * h) % 64u == 0;
}

/* pixels of tile (tx, ty) that lie inside a width x height frame */
RSRT_HD uint32_t rsrt_noise_tile_count(uint32_t tx, uint32_t ty, uint32_t tile_w, uint32_t tile_h, uint32_t width, uint32_t height)
{
    const uint32_t x0 = tx * tile_w, y0 = ty * tile_h;
    const uint32_t cw = width - x0 < tile_w ? width - x0 : tile_w, ch = height - y0 < tile_h ? height - y0 : tile_h;
    return cw * ch;
}

/* what is a tile error above the threshold?  An infinite one always is (a threshold of +inf included). */
RSRT_HD int rsrt_noise_above(float error, float threshold) { return error > threshold || error == rsrt_noise_inf(); }

#endif
