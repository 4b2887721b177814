/*
 * rsrt_local.h — arithmetic of the local exposure pass and the graded display (rsrt_local_exposure, rsrt_local_exposure_download,
 * rsrt_local_gain_download, rsrt_display_local_srgb8; include/rsrt.h "local exposure"), as shared inline code.
 *
 * The pass splits log-luminance into a base and a detail layer (Durand, Dorsey, "Fast Bilateral Filtering for the Display of
 * High-Dynamic-Range Images", SIGGRAPH 2002) and compresses the base alone.  The base is the slice of a bilateral grid (Chen, Paris,
 * Durand, "Real-time Edge-Aware Image Processing with the Bilateral Grid", SIGGRAPH 2007): pixels are counted in a coarse grid over
 * (x, y, log-luminance), the grid is blurred, and a pixel reads the blurred grid at its own position AND its own log-luminance — so
 * the base follows edges and draws no halos.  Like rsrt_exposure.h this is part of the published numeric contract: floats are plain
 * f32 + - * / (-ffp-contract=off, nothing fused) in exactly the order written here, and everything up to the slice is in integers, so
 * the grid does not depend on the order anything is counted in and a numpy restatement reproduces every word and every bit
 * (tests/local_ref.py holds it).
 *
 * Luminance of a pixel of sums:  L = rsrt_exposure_luminance(sum, total), the meter's.  A pixel with !(L > 0) — zero, negative, NaN —
 * is SKIPPED: it is not counted, and its gain is 1.
 * Log-luminance, Q8:  q = min(max(bits(L) >> 15, 111 << 8), (111 << 8) + 8191) - (111 << 8)
 *   the meter's piecewise-linear log2 (Mitchell), 256 steps an octave over the 32 octaves from 2^-16; q >> 5 is rsrt_exposure_word(L).
 *   Denormals land on 0, +inf and anything from 2^16 up on 8191.
 * Grid of a w x h image, cell in {8, 16, 32, 64}:  gx = ceil(w / cell), gy = ceil(h / cell), gz = 32; pixel (x, y) counts in the
 *   cell (x / cell, y / cell, q >> 8).  A cell holds two uint32 — the count and the sum of q — at the words 2 * ((z * gy + y) * gx + x)
 *   and the next.  The grid is of the UNEXPOSED image: exposure and strengths enter at the slice only.
 * Blur: a separable 1-2-1 tent along x, then y, then z, zero outside the grid, in uint32: out[i] = in[i - 1] + 2 * in[i] + in[i + 1]
 *   per word.  The weights sum to 64 and sum <= 64 * 64^2 * 8191 < 2^31: no overflow.
 * Slice at pixel (x, y) with its q.  Per axis (g cells):
 *   x:  u = clamp((x + 0.5f) / (float)cell - 0.5f, 0, g - 1);   y likewise;   z:  u = clamp((float)q / 256 - 0.5f, 0, 31)
 *   i0 = (int)u,  i1 = min(i0 + 1, g - 1),  t = u - (float)i0,  weights w0 = 1.0f - t at i0 and w1 = t at i1
 *   the eight corners in the order z0y0x0, z0y0x1, z0y1x0, z0y1x1, z1y0x0, z1y0x1, z1y1x0, z1y1x1, each w = (wz * wy) * wx:
 *   num += w * (float)sum,  den += w * (float)count  one after the other from 0;  base = num / den, in Q8 units.
 *   A counted pixel finds den > 0: its own cell is one of the corners with a weight of at least 1/8, and the blur kept its count.
 * Gain:  mid = (float)q(key / exposure);  d = (base - mid) * (1.0f / 256) (octaves);  s = d > 0 ? highlights : shadows;
 *   e = -(s * d) clamped to [-max_stops, max_stops];  gain = rsrt_local_exp2(e).  With both strengths 0, e is +-0 and the gain exactly 1.
 * rsrt_local_exp2(e), |e| <= 16:  n = floor(e) by integer conversion, f = e - (float)n,
 *   p = 1 + f * (C1 + f * (C2 + f * (C3 + f * C4))) in Horner form, result p * as_float((n + 127) << 23).
 *   Exact at integers (p(0) = 1 and, in f32, p(1) = 2), monotone non-decreasing, and within 3.4e-6 (2^-18.2) of 2^e relatively —
 *   measured over every e = k * 2^-12 in [-16, 16] and the float neighbours of the integers against float64 (tests/test_local.py
 *   asserts 2^-12: a sixteenth of what a display byte is worth near white).
 *
 * Graded display pixel:  hdr = rsrt_display_hdr_bloomed (rsrt_bloom.h; up(B) = 0 where no bloom is asked for);  hdr = hdr * gain
 * (rsrt_display_hdr_local);  then rsrt_aces_tone_map and rsrt_display_encode.  The gain comes after the bloom: the glow is light in the lens, the local exposure is the print.  With both
 * strengths 0 the bytes are rsrt_display_exposed_srgb8's (intensity 0) or rsrt_display_bloomed_srgb8's.
 */
#ifndef RSRT_LOCAL_H
#define RSRT_LOCAL_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_local_params */
#include "rsrt_bloom.h"
#include "rsrt_exposure.h"

#define RSRT_LOCAL_GZ 32u                 /* octave planes */
#define RSRT_LOCAL_Q_LO (111u << 8)       /* bits(2^-16) >> 15 */
#define RSRT_LOCAL_Q_MAX 8191u
#define RSRT_LOCAL_SKIPPED 0xffffffffu    /* rsrt_local_q_of of a pixel that is not counted */
#define RSRT_LOCAL_CELL 32u               /* defaults: the API's choices, not measurements */
#define RSRT_LOCAL_SHADOWS 0.5f
#define RSRT_LOCAL_HIGHLIGHTS 0.5f
#define RSRT_LOCAL_KEY 0.18f
#define RSRT_LOCAL_MAX_STOPS 4.0f
#define RSRT_LOCAL_EXP2_C1 0.6930321455f
#define RSRT_LOCAL_EXP2_C2 0.2413797677f
#define RSRT_LOCAL_EXP2_C3 0.05203237012f
#define RSRT_LOCAL_EXP2_C4 0.01355574746f

RSRT_HD int rsrt_local_cell_ok(uint32_t cell) { return cell == 8u || cell == 16u || cell == 32u || cell == 64u; }

RSRT_HD int rsrt_local_params_ok(const rsrt_local_params *p)
{
    return p->shadows >= 0.0f && p->shadows <= 1.0f && p->highlights >= 0.0f && p->highlights <= 1.0f && rsrt_exposure_finite_positive(p->key) &&
           p->max_stops >= 0.0f && p->max_stops <= 16.0f && p->flags == 0u;
}

/* cells along an axis of n pixels */
RSRT_HD uint32_t rsrt_local_cells(uint32_t n, uint32_t cell) { return (n + cell - 1u) / cell; }

/* q of a luminance > 0 (of anything else: of its bits) */
RSRT_HD uint32_t rsrt_local_q(float L)
{
    const uint32_t b = rsrt_exposure_bits(L) >> 15;
    const uint32_t lo = b < RSRT_LOCAL_Q_LO ? RSRT_LOCAL_Q_LO : b;
    return (lo > RSRT_LOCAL_Q_LO + RSRT_LOCAL_Q_MAX ? RSRT_LOCAL_Q_LO + RSRT_LOCAL_Q_MAX : lo) - RSRT_LOCAL_Q_LO;
}

/* q of a pixel of sums, or RSRT_LOCAL_SKIPPED */
RSRT_HD uint32_t rsrt_local_q_of(const float sum[3], float total)
{
    const float L = rsrt_exposure_luminance(sum, total);
    return L > 0.0f ? rsrt_local_q(L) : RSRT_LOCAL_SKIPPED;
}

/* the word of the count of cell (x, y, z); the sum of q is the next */
RSRT_HD size_t rsrt_local_word(uint32_t gx, uint32_t gy, uint32_t x, uint32_t y, uint32_t z) { return 2u * (((size_t)z * gy + y) * gx + x); }

/* one word of the tent: the neighbours are 0 outside the grid */
RSRT_HD uint32_t rsrt_local_tent(uint32_t before, uint32_t at, uint32_t after) { return before + 2u * at + after; }

/* u -> i0, i1 and t along an axis of g cells; u is already clamped to [0, g - 1] */
RSRT_HD void rsrt_local_axis(float u, int g, int *i0, int *i1, float *t)
{
    *i0 = (int)u;
    *i1 = *i0 + 1 < g - 1 ? *i0 + 1 : g - 1;
    *t = u - (float)*i0;
}

RSRT_HD float rsrt_local_clampf(float u, float lo, float hi) { return u < lo ? lo : (u > hi ? hi : u); }

/* the grid coordinate of pixel i along an axis of g cells */
RSRT_HD float rsrt_local_u(int i, uint32_t cell, int g) { return rsrt_local_clampf(((float)i + 0.5f) / (float)cell - 0.5f, 0.0f, (float)(g - 1)); }
RSRT_HD float rsrt_local_uz(uint32_t q) { return rsrt_local_clampf((float)q / 256.0f - 0.5f, 0.0f, (float)(RSRT_LOCAL_GZ - 1u)); }

/* base of the eight corners c[k] = {count, sum}, k in the documented order, with the three t */
RSRT_HD float rsrt_local_base8(const uint32_t c[8][2], float tx, float ty, float tz)
{
    const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty}, wz[2] = {1.0f - tz, tz};
    float num = 0.0f, den = 0.0f;
    for (int k = 0; k < 8; k++) {
        const float w = (wz[k >> 2] * wy[(k >> 1) & 1]) * wx[k & 1];
        num = num + w * (float)c[k][1];
        den = den + w * (float)c[k][0];
    }
    return num / den;
}

/* the slice of a blurred grid (gx x gy x 32 cells) at pixel (x, y) with log-luminance q: base, in Q8 units */
RSRT_HD float rsrt_local_slice(const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, int x, int y, uint32_t q)
{
    int x0, x1, y0, y1, z0, z1;
    float tx, ty, tz;
    rsrt_local_axis(rsrt_local_u(x, cell, (int)gx), (int)gx, &x0, &x1, &tx);
    rsrt_local_axis(rsrt_local_u(y, cell, (int)gy), (int)gy, &y0, &y1, &ty);
    rsrt_local_axis(rsrt_local_uz(q), (int)RSRT_LOCAL_GZ, &z0, &z1, &tz);
    const int xs[2] = {x0, x1}, ys[2] = {y0, y1}, zs[2] = {z0, z1};
    uint32_t c[8][2];
    for (int k = 0; k < 8; k++) {
        const size_t at = rsrt_local_word(gx, gy, (uint32_t)xs[k & 1], (uint32_t)ys[(k >> 1) & 1], (uint32_t)zs[k >> 2]);
        c[k][0] = grid[at];
        c[k][1] = grid[at + 1];
    }
    return rsrt_local_base8(c, tx, ty, tz);
}

/* 2^e for |e| <= 16 */
RSRT_HD float rsrt_local_exp2(float e)
{
    int n = (int)e;
    if ((float)n > e) n = n - 1;
    const float f = e - (float)n;
    float p = RSRT_LOCAL_EXP2_C4;
    p = p * f + RSRT_LOCAL_EXP2_C3;
    p = p * f + RSRT_LOCAL_EXP2_C2;
    p = p * f + RSRT_LOCAL_EXP2_C1;
    p = p * f + 1.0f;
    return p * rsrt_exposure_as_float((uint32_t)(n + 127) << 23);
}

/* what the gain compares the base with: the log-luminance that the exposure puts on the key; exposure finite and > 0 */
RSRT_HD float rsrt_local_mid(float key, float exposure) { return (float)rsrt_local_q(key / exposure); }

/* the gain of a counted pixel from its base; p must pass rsrt_local_params_ok */
RSRT_HD float rsrt_local_gain(float base, float mid, const rsrt_local_params *p)
{
    const float d = (base - mid) * (1.0f / 256.0f);
    const float s = d > 0.0f ? p->highlights : p->shadows;
    const float e = rsrt_local_clampf(-(s * d), -p->max_stops, p->max_stops);
    return rsrt_local_exp2(e);
}

/* the gain of a pixel with rsrt_local_q_of q */
RSRT_HD float rsrt_local_gain_at(const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, int x, int y, uint32_t q, float mid, const rsrt_local_params *p)
{
    if (q == RSRT_LOCAL_SKIPPED) return 1.0f;
    return rsrt_local_gain(rsrt_local_slice(grid, gx, gy, cell, x, y, q), mid, p);
}

/* the display chain's fourth step: the bloomed colour times the pixel's gain */
RSRT_HD void rsrt_display_hdr_local(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain, float hdr[3])
{
    rsrt_display_hdr_bloomed(sum_rgb, total, exposure, intensity, up_b, hdr);
    for (int i = 0; i < 3; i++) hdr[i] = hdr[i] * gain;
}

/* one pixel: sums (f32), up(B) at it (0 where no bloom is asked for) and its gain -> display bytes at an exposure */
RSRT_HD void rsrt_display_pixel_local(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                                      unsigned char out_rgb[3])
{
    float hdr[3], sdr[3];
    rsrt_display_hdr_local(sum_rgb, total, exposure, intensity, up_b, gain, hdr);
    rsrt_aces_tone_map(hdr, sdr);
    rsrt_display_encode(sdr, out_rgb);
}

#endif
