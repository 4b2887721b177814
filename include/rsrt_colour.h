/*
 * rsrt_colour.h — arithmetic of the white-balance meter, the colour LUT and the colour display (rsrt_white_meter,
 * rsrt_white_download, rsrt_colour_lut_build, rsrt_display_colour_srgb8; include/rsrt.h "white balance and colour grading"), as
 * shared inline code.
 *
 * The meter is a grey-world estimate made robust by a mean shift: a 2-D histogram of log-chromaticity (Finlayson, Hordley, "Color
 * constancy at a pixel", JOSA A 2001: in log(G/R), log(G/B) an illuminant change is a translation), whose mode is followed with a
 * gated mean so that saturated surfaces drop out.  The grade is the ASC CDL (slope, offset, power, saturation) baked into a 3-D LUT
 * that the display reads by tetrahedral interpolation.  The gains are per channel in the working RGB: no chromatic adaptation in a
 * cone space (Bradford) is made.  Like rsrt_exposure.h and rsrt_local.h this is part of the published numeric contract: floats are
 * plain f32 + - * / and rsrt_sqrtf (-ffp-contract=off, nothing fused) in exactly the order written here, and the meter is in integers
 * up to its last step, so the histogram does not depend on the order pixels are counted in and a numpy restatement reproduces every
 * word and every bit (tests/colour_ref.py holds it).
 *
 * Pixel colour:  c = sum.rgb / total, one f32 division a channel (the exposure meter's `total` rule).  A pixel is SKIPPED unless
 *   c.r > 0 && c.g > 0 && c.b > 0: NaN, zero and negative channels are skipped, +inf is not.
 * Integer log2, Q16 (rsrt_colour_ilog2), of x > 0 with b = bits(x):  e = (b >> 23) - 127,  m = (b & 0x7fffff) >> 7,
 *   ilog2 = e * 65536 + m + ((m * (65536 - m) * 22700) >> 32)  in 64-bit: Mitchell's piecewise-linear log2 with a parabola on top,
 *   within 0.0077 octave of log2 over all 2^23 mantissas (Mitchell's plain form, which the exposure meter uses, is 0.086 off and does
 *   not cancel between two channels).  Denormals read as e = -127, +inf as 128 * 65536.
 * Chroma:  u = (ilog2(c.g) - ilog2(c.r)) >> 12,  v = (ilog2(c.g) - ilog2(c.b)) >> 12  (arithmetic shifts: floors), in 1/16 octave.
 * Bins:  ub = clamp(u + 32, 0, 63), vb likewise, word = vb * 64 + ub: -2 .. +2 octaves, bins 0 and 63 of either axis the clamped edges.
 * Histogram: 4097 uint32 words — 4096 bins, then [4096] the skipped pixels; the words sum to the pixel count.
 *
 * White point from a histogram (rsrt_white_from_histogram; pure, integers up to step 4):
 *   1. window = bins 1 .. 62 on both axes.  Over a window:  N = sum of count,  Su = sum of count * (2 * (ub - 32) + 1),  Sv likewise
 *      (a bin's centre in 1/32 octave), in int64.
 *   2. `iterations` times: take N, Su, Sv over the window; if N == 0 stop; centre = floor(S / (2 N)) + 32 per axis (a signed floor);
 *      window = [centre - gate, centre + gate] per axis, clipped to 1 .. 62.
 *   3. N, Su, Sv over the final window.  all = the sum of the 4097 words.  If N == 0 or N * 1000 < min_permille * all there is no
 *      estimate: white = target = (previous given ? previous : {1, 1, 1}), illuminant {1, 1, 1}, eu = ev = 0, estimated = 0.
 *   4. eu = (float)Su / (float)(32 * N),  ev likewise: one f32 division of two correctly rounded integer -> f32 conversions; octaves.
 *      illuminant = (exp2(-eu), 1, exp2(-ev))                                    exp2 is rsrt_local_exp2
 *      xu = clamp(strength * eu, -max_stops, max_stops),  xv likewise;  gr = exp2(xu),  gb = exp2(xv)
 *      norm = (0.2126f * gr + 0.7152f) + 0.0722f * gb;  target = (gr / norm, 1.0f / norm, gb / norm)      a grey keeps its luminance
 *      white = previous given ? previous + (target - previous) * blend : target,  per channel
 *   `previous` is given when it is not all zero.  The library keeps no white point.
 *
 * LUT: n^3 nodes, n in {2, 3, 17, 33, 65}, red fastest, a node the ENCODED output rgb in [0, 1].  The domain is square-root encoded on
 *   both sides: the coordinate of a tone-mapped channel s in [0, 1] is rsrt_sqrtf(s) * (float)(n - 1), the decoded output is enc * enc.
 * Bake (rsrt_colour_lut_node):  enc = (float)i / (float)(n - 1) per axis,  lin = enc * enc;  per channel x = lin * slope + offset
 *   (two roundings), clamped to [0, 1], then x = rsrt_colour_pow(x, power) unless power == 1;  Y = (0.2126f * x.r + 0.7152f * x.g) +
 *   0.0722f * x.b;  unless saturation == 1:  x = Y + saturation * (x - Y);  clamp to [0, 1];  node = rsrt_sqrtf(x).  With identity
 *   parameters the nodes are exactly i / (n - 1): sqrt(fl(x * x)) == x in binary floating point.
 * rsrt_colour_log2(x), x a normal float > 0:  e = exponent, f = mantissa in [1, 2); if f > 1.41421354f: f = f * 0.5f, e = e + 1;
 *   t = (f - 1.0f) / (f + 1.0f),  t2 = t * t,  p = ((((L9 * t2 + L7) * t2 + L5) * t2 + L3) * t2 + L1) * t  (L_k = 2 / (k ln 2)),
 *   result (float)e + p.  Exact at powers of two.
 * rsrt_colour_pow(x, p), x in [0, 1], p in [0.25, 4]:  0 for x < 2^-126 (zero, denormals);  e = p * rsrt_colour_log2(x);  0 for
 *   e < -64;  else rsrt_local_exp2(e).  pow(1, p) == 1.  No powf anywhere.
 * Tetrahedral interpolation (rsrt_colour_lut_at) at enc rgb in [0, 1]:  per axis  p = enc * (float)(n - 1),  i = min((int)p, n - 2),
 *   t = p - (float)i  (an input of exactly 1 lands on the last cell with t = 1).  The three (t, stride) pairs — (t_r, 1), (t_g, n),
 *   (t_b, n * n) — are sorted to a >= b >= c by three compare-and-swaps in this order: if (a.t < b.t) swap(a, b); if (b.t < c.t)
 *   swap(b, c); if (a.t < b.t) swap(a, b).  That picks one of the six tetrahedra; with base = (i_b * n + i_g) * n + i_r the nodes are
 *   n0 = base, n1 = n0 + a.stride, n2 = n1 + b.stride, n3 = n2 + c.stride, the weights w0 = 1 - a.t, w1 = a.t - b.t, w2 = b.t - c.t,
 *   w3 = c.t, and per channel  g = ((w0 * n0 + w1 * n1) + w2 * n2) + w3 * n3.  Exact at the nodes: every weight is then 0 or 1.
 *
 * Colour display pixel (rsrt_display_pixel_colour):  hdr = rsrt_display_hdr_local (rsrt_local.h: the f16-rounded mean times exposure, plus
 *   intensity * up(B), times the local gain);  hdr[i] = hdr[i] * white[i];  rsrt_aces_tone_map;  with lut_strength > 0, per channel:
 *   s = sdr (NaN -> 0),  enc = rsrt_sqrtf(s),  g = the interpolation above at the three enc,  o = enc + lut_strength * (g - enc)
 *   clamped to [0, 1],  sdr = o * o  (up to here: rsrt_display_sdr_colour);  then rsrt_display_encode.  With white {1, 1, 1} and
 *   lut_strength 0 the bytes are rsrt_display_local_srgb8's.
 */
#ifndef RSRT_COLOUR_H
#define RSRT_COLOUR_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_white_params, rsrt_white_result, rsrt_cdl_params, rsrt_colour_params */
#include "rsrt_local.h"

#define RSRT_WHITE_AXIS 64u                /* bins an axis: 16 an octave, -2 .. +2 octaves */
#define RSRT_WHITE_BINS 4096u
#define RSRT_WHITE_WORDS 4097u             /* the bins, then the skipped pixels */
#define RSRT_WHITE_LOG2_K 22700            /* the parabola on Mitchell's log2, Q16 */
#define RSRT_WHITE_GATE 12u                /* rsrt_white_params defaults */
#define RSRT_WHITE_ITERATIONS 3u
#define RSRT_WHITE_MIN_PERMILLE 50u
#define RSRT_WHITE_STRENGTH 1.0f
#define RSRT_WHITE_MAX_STOPS 2.0f
#define RSRT_WHITE_BLEND 1.0f
#define RSRT_CDL_SLOPE 1.0f                /* rsrt_cdl_params defaults: the identity */
#define RSRT_CDL_OFFSET 0.0f
#define RSRT_CDL_POWER 1.0f
#define RSRT_CDL_SATURATION 1.0f
#define RSRT_COLOUR_LUT_SIZE 33u           /* the default n */
#define RSRT_COLOUR_LUT_STRENGTH 1.0f
#define RSRT_COLOUR_LOG2_L1 2.8853900818f  /* 2 / (k ln 2) */
#define RSRT_COLOUR_LOG2_L3 0.9617966939f
#define RSRT_COLOUR_LOG2_L5 0.5770780164f
#define RSRT_COLOUR_LOG2_L7 0.4121985831f
#define RSRT_COLOUR_LOG2_L9 0.3205988980f

RSRT_HD int rsrt_colour_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }

/* Q16 log2 of x > 0 */
RSRT_HD int32_t rsrt_colour_ilog2(float x)
{
    const uint32_t b = rsrt_exposure_bits(x);
    const int64_t e = (int64_t)(b >> 23) - 127, m = (int64_t)((b & 0x7fffffu) >> 7);
    return (int32_t)(e * 65536 + m + ((m * (65536 - m) * RSRT_WHITE_LOG2_K) >> 32));
}

RSRT_HD uint32_t rsrt_white_bin(int32_t d)
{
    const int32_t u = (d >> 12) + 32; /* an arithmetic shift: a floor */
    return (uint32_t)(u < 0 ? 0 : (u > 63 ? 63 : u));
}

/* the histogram word a pixel of sums counts in: its bin, or 4096 (skipped) */
RSRT_HD uint32_t rsrt_white_word(const float sum[3], float total)
{
    const float r = sum[0] / total, g = sum[1] / total, b = sum[2] / total;
    if (!(r > 0.0f && g > 0.0f && b > 0.0f)) return RSRT_WHITE_BINS;
    const int32_t lg = rsrt_colour_ilog2(g);
    return rsrt_white_bin(lg - rsrt_colour_ilog2(b)) * RSRT_WHITE_AXIS + rsrt_white_bin(lg - rsrt_colour_ilog2(r));
}

RSRT_HD int rsrt_white_params_ok(const rsrt_white_params *p)
{
    const float *q = p->previous;
    const int none = q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f;
    const int given = rsrt_exposure_finite_positive(q[0]) && rsrt_exposure_finite_positive(q[1]) && rsrt_exposure_finite_positive(q[2]);
    return p->gate >= 1u && p->gate <= 31u && p->iterations <= 8u && p->min_permille <= 1000u && p->strength >= 0.0f && p->strength <= 1.0f &&
           p->max_stops >= 0.0f && p->max_stops <= 4.0f && p->blend >= 0.0f && p->blend <= 1.0f && (none || given) && p->flags == 0u;
}

/* N, Su, Sv of the window [lo[0], hi[0]] x [lo[1], hi[1]] (u, v) */
RSRT_HD void rsrt_white_window(const uint32_t *hist, const int lo[2], const int hi[2], int64_t *N, int64_t *Su, int64_t *Sv)
{
    *N = *Su = *Sv = 0;
    for (int vb = lo[1]; vb <= hi[1]; vb++)
        for (int ub = lo[0]; ub <= hi[0]; ub++) {
            const int64_t c = (int64_t)hist[(uint32_t)vb * RSRT_WHITE_AXIS + (uint32_t)ub];
            *N += c;
            *Su += c * (2 * (ub - 32) + 1);
            *Sv += c * (2 * (vb - 32) + 1);
        }
}

RSRT_HD int64_t rsrt_colour_floor_div(int64_t a, int64_t b /* > 0 */) { return a / b - (a % b < 0 ? 1 : 0); }

/* the white point of a histogram of RSRT_WHITE_WORDS words; p must pass rsrt_white_params_ok */
RSRT_HD void rsrt_white_from_histogram(const uint32_t *hist, const rsrt_white_params *p, rsrt_white_result *out)
{
    uint64_t all = 0;
    for (uint32_t i = 0; i < RSRT_WHITE_WORDS; i++) all += hist[i];
    int lo[2] = {1, 1}, hi[2] = {62, 62};
    int64_t N, S[2];
    for (uint32_t it = 0; it < p->iterations; it++) {
        rsrt_white_window(hist, lo, hi, &N, &S[0], &S[1]);
        if (N == 0) break;
        for (int a = 0; a < 2; a++) {
            const int centre = (int)rsrt_colour_floor_div(S[a], 2 * N) + 32;
            lo[a] = centre - (int)p->gate < 1 ? 1 : centre - (int)p->gate;
            hi[a] = centre + (int)p->gate > 62 ? 62 : centre + (int)p->gate;
        }
    }
    rsrt_white_window(hist, lo, hi, &N, &S[0], &S[1]);
    const int given = !(p->previous[0] == 0.0f && p->previous[1] == 0.0f && p->previous[2] == 0.0f);
    out->gated = (uint32_t)N;
    out->counted = (uint32_t)(all - hist[RSRT_WHITE_BINS]);
    out->skipped = hist[RSRT_WHITE_BINS];
    out->_pad = 0;
    if (N == 0 || (uint64_t)N * 1000u < (uint64_t)p->min_permille * all) {
        for (int i = 0; i < 3; i++) {
            out->white[i] = out->target[i] = given ? p->previous[i] : 1.0f;
            out->illuminant[i] = 1.0f;
        }
        out->eu = out->ev = 0.0f;
        out->estimated = 0;
        return;
    }
    const float den = (float)(32 * N);
    const float eu = (float)S[0] / den, ev = (float)S[1] / den;
    out->eu = eu;
    out->ev = ev;
    out->estimated = 1;
    out->illuminant[0] = rsrt_local_exp2(-eu);
    out->illuminant[1] = 1.0f;
    out->illuminant[2] = rsrt_local_exp2(-ev);
    const float gr = rsrt_local_exp2(rsrt_local_clampf(p->strength * eu, -p->max_stops, p->max_stops));
    const float gb = rsrt_local_exp2(rsrt_local_clampf(p->strength * ev, -p->max_stops, p->max_stops));
    const float norm = (0.2126f * gr + 0.7152f) + 0.0722f * gb;
    out->target[0] = gr / norm;
    out->target[1] = 1.0f / norm;
    out->target[2] = gb / norm;
    for (int i = 0; i < 3; i++) out->white[i] = given ? p->previous[i] + (out->target[i] - p->previous[i]) * p->blend : out->target[i];
}

/* ---- the colour LUT ---- */

RSRT_HD int rsrt_colour_lut_size_ok(uint32_t n) { return n == 2u || n == 3u || n == 17u || n == 33u || n == 65u; }

RSRT_HD int rsrt_colour_in(float x, float lo, float hi) { return x >= lo && x <= hi; } /* (NaN: no) */

RSRT_HD int rsrt_cdl_params_ok(const rsrt_cdl_params *p)
{
    for (int i = 0; i < 3; i++)
        if (!(rsrt_colour_in(p->slope[i], 0.0f, 16.0f) && rsrt_colour_in(p->offset[i], -1.0f, 1.0f) && rsrt_colour_in(p->power[i], 0.25f, 4.0f))) return 0;
    return rsrt_colour_in(p->saturation, 0.0f, 4.0f) && p->flags == 0u;
}

RSRT_HD int rsrt_colour_params_ok(const rsrt_colour_params *p)
{
    return rsrt_exposure_finite_positive(p->white[0]) && rsrt_exposure_finite_positive(p->white[1]) && rsrt_exposure_finite_positive(p->white[2]) &&
           rsrt_colour_in(p->lut_strength, 0.0f, 1.0f) && p->flags == 0u;
}

/* log2 of a normal float > 0 */
RSRT_HD float rsrt_colour_log2(float x)
{
    const uint32_t b = rsrt_exposure_bits(x);
    int e = (int)(b >> 23) - 127;
    float f = rsrt_exposure_as_float((b & 0x7fffffu) | 0x3f800000u);
    if (f > 1.41421354f) {
        f = f * 0.5f;
        e = e + 1;
    }
    const float t = (f - 1.0f) / (f + 1.0f), t2 = t * t;
    float p = RSRT_COLOUR_LOG2_L9;
    p = p * t2 + RSRT_COLOUR_LOG2_L7;
    p = p * t2 + RSRT_COLOUR_LOG2_L5;
    p = p * t2 + RSRT_COLOUR_LOG2_L3;
    p = p * t2 + RSRT_COLOUR_LOG2_L1;
    return (float)e + p * t;
}

/* x^p for x in [0, 1], p in [0.25, 4] */
RSRT_HD float rsrt_colour_pow(float x, float p)
{
    if (x < 1.17549435e-38f) return 0.0f;
    const float e = p * rsrt_colour_log2(x);
    if (e < -64.0f) return 0.0f;
    return rsrt_local_exp2(e);
}

RSRT_HD float rsrt_colour_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

/* the node (ir, ig, ib) of the n^3 LUT of a CDL: encoded rgb; p must pass rsrt_cdl_params_ok */
RSRT_HD void rsrt_colour_lut_node(uint32_t n, uint32_t ir, uint32_t ig, uint32_t ib, const rsrt_cdl_params *p, float out[3])
{
    const uint32_t idx[3] = {ir, ig, ib};
    float x[3];
    for (int i = 0; i < 3; i++) {
        const float enc = (float)idx[i] / (float)(n - 1u);
        const float lin = enc * enc;
        x[i] = rsrt_colour_clamp01(lin * p->slope[i] + p->offset[i]);
        if (p->power[i] != 1.0f) x[i] = rsrt_colour_pow(x[i], p->power[i]);
    }
    if (p->saturation != 1.0f) {
        const float Y = (0.2126f * x[0] + 0.7152f * x[1]) + 0.0722f * x[2];
        for (int i = 0; i < 3; i++) x[i] = Y + p->saturation * (x[i] - Y);
    }
    for (int i = 0; i < 3; i++) out[i] = rsrt_sqrtf(rsrt_colour_clamp01(x[i]));
}

/* cell and fraction of an encoded channel in [0, 1] along n nodes */
RSRT_HD void rsrt_colour_lut_axis(float enc, uint32_t n, uint32_t *i, float *t)
{
    const float p = enc * (float)(n - 1u);
    const uint32_t c = (uint32_t)(int)p;
    *i = c > n - 2u ? n - 2u : c;
    *t = p - (float)*i;
}

/* the LUT (n^3 nodes of 4 floats: rgb and a fourth that is not read) at encoded rgb, every channel in [0, 1] */
RSRT_HD void rsrt_colour_lut_at(const float *lut, uint32_t n, const float enc[3], float out[3])
{
    uint32_t ir, ig, ib;
    float ta, tb, tc;
    rsrt_colour_lut_axis(enc[0], n, &ir, &ta);
    rsrt_colour_lut_axis(enc[1], n, &ig, &tb);
    rsrt_colour_lut_axis(enc[2], n, &ib, &tc);
    uint32_t sa = 1u, sb = n, sc = n * n;
    if (ta < tb) { const float t = ta; ta = tb; tb = t; const uint32_t s = sa; sa = sb; sb = s; }
    if (tb < tc) { const float t = tb; tb = tc; tc = t; const uint32_t s = sb; sb = sc; sc = s; }
    if (ta < tb) { const float t = ta; ta = tb; tb = t; const uint32_t s = sa; sa = sb; sb = s; }
    const float w0 = 1.0f - ta, w1 = ta - tb, w2 = tb - tc, w3 = tc;
    const float *n0 = lut + 4u * (size_t)((ib * n + ig) * n + ir), *n1 = n0 + 4u * (size_t)sa, *n2 = n1 + 4u * (size_t)sb, *n3 = n2 + 4u * (size_t)sc;
    for (int i = 0; i < 3; i++) out[i] = ((w0 * n0[i] + w1 * n1[i]) + w2 * n2[i]) + w3 * n3[i];
}

/* step 4 of the colour display: tone-mapped sdr through the LUT at a strength > 0, in place */
RSRT_HD void rsrt_colour_grade(const float *lut, uint32_t n, float strength, float sdr[3])
{
    float enc[3], g[3];
    for (int i = 0; i < 3; i++) enc[i] = rsrt_sqrtf(sdr[i] == sdr[i] ? sdr[i] : 0.0f);
    rsrt_colour_lut_at(lut, n, enc, g);
    for (int i = 0; i < 3; i++) {
        const float o = rsrt_colour_clamp01(enc[i] + strength * (g[i] - enc[i]));
        sdr[i] = o * o;
    }
}

/* the display chain's fifth to seventh step: one pixel's sums (f32), up(B) at it (0 where no bloom is asked for), its local gain (1 where
 * none is asked for), the white point and the LUT (looked at only with lut_strength > 0) -> the tone-mapped, graded colour */
RSRT_HD void rsrt_display_sdr_colour(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                                     const rsrt_colour_params *colour, const float *lut, uint32_t n, float sdr[3])
{
    float hdr[3];
    rsrt_display_hdr_local(sum_rgb, total, exposure, intensity, up_b, gain, hdr);
    for (int i = 0; i < 3; i++) hdr[i] = hdr[i] * colour->white[i];
    rsrt_aces_tone_map(hdr, sdr);
    if (colour->lut_strength > 0.0f) rsrt_colour_grade(lut, n, colour->lut_strength, sdr);
}

/* ... -> display bytes at an exposure */
RSRT_HD void rsrt_display_pixel_colour(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                                       const rsrt_colour_params *colour, const float *lut, uint32_t n, unsigned char out_rgb[3])
{
    float sdr[3];
    rsrt_display_sdr_colour(sum_rgb, total, exposure, intensity, up_b, gain, colour, lut, n, sdr);
    rsrt_display_encode(sdr, out_rgb);
}

#endif
