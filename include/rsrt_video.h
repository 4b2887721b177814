/*
 * rsrt_video.h — arithmetic of the video pass (rsrt_display_video; include/rsrt.h "video output"), as shared inline code: what happens to
 * a pixel's display colour when the output is a Y'CbCr 4:2:0 frame for an encoder instead of an RGB word — a continuous transfer code,
 * the luma / colour-difference matrix, the 2 x 2 chroma reduction at a named siting, the quantiser and the frame's layout.
 *
 * Like rsrt_hdr.h this is part of the published numeric contract: floats are plain f32 + - * / and floorf (-ffp-contract=off, nothing
 * fused) in exactly the order written here, both transfer curves are the threshold tables the RGB displays quantise with (no pow at run
 * time), the dither's noise is rsrt_finish.h's integer hash, and a numpy restatement reproduces every code (tests/video_ref.py holds it).
 *
 * 1. input, three channels x:
 *    RSRT_VIDEO_BT709:  rsrt_finish_sdr (rsrt_finish.h step 1): the tone-mapped, graded colour rsrt_display_colour_srgb8 quantises, LUT
 *      included; table T = RSRT_SRGB8_THRESHOLDS, N = 255, end = 1.
 *    RSRT_VIDEO_HDR10:  rsrt_hdr_pixel_nits (rsrt_hdr.h steps 1 to 5) with the caller's rsrt_hdr_params, encoding RSRT_HDR_PQ10 (its
 *      dither and seed are not looked at): Rec.2020 nits behind the shoulder; T = RSRT_PQ10_THRESHOLDS, N = 1023, end = 10000.
 * 2. continuous code (rsrt_video_code), the value rsrt_finish.h step 7 names, b + p - 0.5 at position p inside code b.  b = the number of
 *    thresholds <= x (NaN: 0), the displays' own binary search.
 *      0 < b < N:  e = ((float)b - 0.5f) + (x - T[b - 1]) / (T[b] - T[b - 1])
 *      b == 0:     e = x > 0 ? 0.5f * (x / T[0]) : 0                       (NaN, -0 and negatives give 0)
 *      b == N:     e = x >= end ? (float)N : ((float)N - 0.5f) + 0.5f * ((x - T[N - 1]) / (end - T[N - 1]))
 *    e is finite for every input, non-decreasing in x (a difference, a quotient by a positive constant and a sum with a constant are
 *    each monotone in f32, and a piece ends where the next begins: at b + 0.5) and lies in [b - 0.5, b + 0.5] (in [0, 0.5] and
 *    [N - 0.5, N] at the ends).  The signal is  E' = e / (float)N  per channel, in [0, 1].  Between thresholds the code is linear in x
 *    where the true curve bends: the largest distance, just above the sRGB curve's linear toe, is g'' / (8 g'^2) = 0.007 of an 8-bit code
 *    (tests/test_video.py derives and checks it); the PQ table's is smaller.
 * 3. matrix (rsrt_video_ycc), non-constant luminance:
 *      Y'  = (Kr * R' + Kg * G') + Kb * B',   Cb' = (B' - Y') / Db,   Cr' = (R' - Y') / Dr
 *    RSRT_VIDEO_BT709:  Kr 0.2126f, Kg 0.7152f, Kb 0.0722f, Db 1.8556f, Dr 1.5748f     (BT.709; Db = 2 (1 - Kb), Dr = 2 (1 - Kr))
 *    RSRT_VIDEO_HDR10:  Kr 0.2627f, Kg 0.6780f, Kb 0.0593f, Db 1.8814f, Dr 1.4746f     (BT.2020 / BT.2100 NCL)
 *    With R' = G' = B' the luma is the channel to a few ulp, the differences a few 1e-8 and both chroma codes exactly neutral.
 * 4. chroma reduction, on the float Cb', Cr' of step 3, each alone.  The chroma planes are ceil(W / 2) x ceil(H / 2); sample (cx, cy)
 *    belongs to the luma quad (2 cx .., 2 cy ..); every coordinate is clamped to the picture (edge replicate).  With c(x, y) the pixel's
 *    value and  h(y) = ((c(2 cx - 1, y) + c(2 cx + 1, y)) + 2.0f * c(2 cx, y)) * 0.25f   (rsrt_video_h121):
 *      RSRT_VIDEO_SITING_CENTRE:   ((c(2 cx, 2 cy) + c(2 cx + 1, 2 cy)) + (c(2 cx, 2 cy + 1) + c(2 cx + 1, 2 cy + 1))) * 0.25f
 *      RSRT_VIDEO_SITING_LEFT:     (h(2 cy) + h(2 cy + 1)) * 0.5f
 *      RSRT_VIDEO_SITING_TOPLEFT:  ((h(2 cy - 1) + h(2 cy + 1)) + 2.0f * h(2 cy)) * 0.25f
 *    A constant picture keeps its value bit for bit under all three; a picture constant along x gives LEFT and CENTRE the same bits.
 * 5. codes.  d = depth, m = 2^(d - 8) (1 or 4), peak = 2^d - 1:
 *      RSRT_VIDEO_LIMITED:  Y = m * (16.0f + 219.0f * Y') in [16 m, 235 m],   C = m * (128.0f + 224.0f * C') in [16 m, 240 m]
 *      RSRT_VIDEO_FULL:     Y = peak * Y',   C = 128 m + peak * C',   both in [0, peak]
 *    quantiser (rsrt_video_quantise):  v clamped to its range (v < lo ? lo : v > hi ? hi : v),  q = floorf((v + 0.5f) + t),  clamped to the
 *    range again (the dither may pass it), the code (uint32_t)q.  t = dither * ((u1 + u2) - 1.0f), and 0 with dither 0.  The draws are
 *    rsrt_finish.h's, u = rsrt_finish_uniform(rsrt_finish_pcg(base + k)): the luma of pixel (x, y) takes k = 1, 2 at
 *    base = rsrt_finish_hash_base(x, y, seed); Cb takes k = 3, 4 and Cr k = 5, 6 at rsrt_finish_hash_base(cx, cy, seed).
 * 6. layout (rsrt_video_planes).  Rows are tightly packed, every word little-endian, a sample one byte at 8 bits and a uint16 at 10.
 *      RSRT_VIDEO_SEMIPLANAR:  W x H luma, then ceil(H / 2) rows of ceil(W / 2) pairs Cb, Cr.  NV12; at 10 bits P010, the code << 6.
 *      RSRT_VIDEO_PLANAR:      W x H luma, the Cb plane, the Cr plane.  I420; at 10 bits yuv420p10le, the code in the low bits.
 * 7. content light levels (RSRT_VIDEO_HDR10): rsrt_hdr.h step 7 over the nits of step 1: the integers rsrt_display_hdr gives.
 */
#ifndef RSRT_VIDEO_H
#define RSRT_VIDEO_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rsrt.h" /* rsrt_video_params, RSRT_VIDEO_* */
#include "rsrt_hdr.h"

#define RSRT_VIDEO_DEFAULT_STANDARD RSRT_VIDEO_BT709 /* rsrt_video_params defaults */
#define RSRT_VIDEO_DEFAULT_DEPTH 8u
#define RSRT_VIDEO_DEFAULT_LAYOUT RSRT_VIDEO_SEMIPLANAR
#define RSRT_VIDEO_DEFAULT_RANGE RSRT_VIDEO_LIMITED
#define RSRT_VIDEO_DEFAULT_SITING RSRT_VIDEO_SITING_LEFT
#define RSRT_VIDEO_DEFAULT_DITHER 0.0f
#define RSRT_VIDEO_DEFAULT_SEED 0u
#define RSRT_VIDEO_DEFAULT_FLAGS 0u

RSRT_HD int rsrt_video_params_ok(const rsrt_video_params *p)
{
    return (p->standard == RSRT_VIDEO_BT709 || p->standard == RSRT_VIDEO_HDR10) && (p->depth == 10u || (p->depth == 8u && p->standard == RSRT_VIDEO_BT709)) &&
           (p->layout == RSRT_VIDEO_SEMIPLANAR || p->layout == RSRT_VIDEO_PLANAR) && (p->range == RSRT_VIDEO_LIMITED || p->range == RSRT_VIDEO_FULL) &&
           (p->siting == RSRT_VIDEO_SITING_LEFT || p->siting == RSRT_VIDEO_SITING_CENTRE || p->siting == RSRT_VIDEO_SITING_TOPLEFT) &&
           rsrt_colour_in(p->dither, 0.0f, 1.0f) && p->flags == 0u;
}

/* step 2 over a table of n thresholds that ends at `end`: b is the number of thresholds <= x */
RSRT_HD float rsrt_video_code_at(float x, unsigned b, const float *t, unsigned n, float end)
{
    if (b == 0u) return x > 0.0f ? 0.5f * (x / t[0]) : 0.0f;
    if (b == n) return x >= end ? (float)n : ((float)n - 0.5f) + 0.5f * ((x - t[n - 1u]) / (end - t[n - 1u]));
    return ((float)b - 0.5f) + (x - t[b - 1u]) / (t[b] - t[b - 1u]);
}

/* the continuous 8-bit sRGB code of a linear value, 0 .. 255, and the continuous 10-bit PQ code of nits, 0 .. 1023 */
RSRT_HD float rsrt_video_code_srgb(float x) { return rsrt_video_code_at(x, rsrt_srgb8_encode(x), RSRT_SRGB8_THRESHOLDS, 255u, 1.0f); }
RSRT_HD float rsrt_video_code_pq(float nits) { return rsrt_video_code_at(nits, rsrt_pq10_encode(nits), RSRT_PQ10_THRESHOLDS, 1023u, RSRT_HDR_MAX_NITS); }

/* step 2: the three channels of step 1 -> E' */
RSRT_HD void rsrt_video_signal(uint32_t standard, const float x[3], float e[3])
{
    for (int i = 0; i < 3; i++) e[i] = standard == RSRT_VIDEO_HDR10 ? rsrt_video_code_pq(x[i]) / 1023.0f : rsrt_video_code_srgb(x[i]) / 255.0f;
}

/* step 3: E' -> Y', Cb', Cr' */
RSRT_HD void rsrt_video_ycc(uint32_t standard, const float e[3], float ycc[3])
{
    const int hdr = standard == RSRT_VIDEO_HDR10;
    const float kr = hdr ? 0.2627f : 0.2126f, kg = hdr ? 0.6780f : 0.7152f, kb = hdr ? 0.0593f : 0.0722f;
    const float db = hdr ? 1.8814f : 1.8556f, dr = hdr ? 1.4746f : 1.5748f;
    const float y = (kr * e[0] + kg * e[1]) + kb * e[2];
    ycc[0] = y;
    ycc[1] = (e[2] - y) / db;
    ycc[2] = (e[0] - y) / dr;
}

/* step 4 */
RSRT_HD float rsrt_video_h121(float l, float c, float r) { return ((l + r) + 2.0f * c) * 0.25f; }
RSRT_HD float rsrt_video_centre(float p00, float p01, float p10, float p11) { return ((p00 + p01) + (p10 + p11)) * 0.25f; }
RSRT_HD float rsrt_video_left(float h0, float h1) { return (h0 + h1) * 0.5f; }

/* step 5: the value of a luma or a chroma sample before the quantiser, and its range */
RSRT_HD float rsrt_video_luma_value(float y, uint32_t depth, uint32_t range, float *lo, float *hi)
{
    const float m = depth == 10u ? 4.0f : 1.0f, peak = depth == 10u ? 1023.0f : 255.0f;
    if (range == RSRT_VIDEO_FULL) {
        *lo = 0.0f; *hi = peak;
        return peak * y;
    }
    *lo = 16.0f * m; *hi = 235.0f * m;
    return m * (16.0f + 219.0f * y);
}
RSRT_HD float rsrt_video_chroma_value(float c, uint32_t depth, uint32_t range, float *lo, float *hi)
{
    const float m = depth == 10u ? 4.0f : 1.0f, peak = depth == 10u ? 1023.0f : 255.0f;
    if (range == RSRT_VIDEO_FULL) {
        *lo = 0.0f; *hi = peak;
        return 128.0f * m + peak * c;
    }
    *lo = 16.0f * m; *hi = 240.0f * m;
    return m * (128.0f + 224.0f * c);
}

/* the dither's offset from draws k and k + 1 at a hash base; 0 with dither 0 */
RSRT_HD float rsrt_video_dither(float dither, uint32_t base, uint32_t k)
{
    if (!(dither > 0.0f)) return 0.0f;
    const float u1 = rsrt_finish_uniform(rsrt_finish_pcg(base + k)), u2 = rsrt_finish_uniform(rsrt_finish_pcg(base + k + 1u));
    return dither * ((u1 + u2) - 1.0f);
}

RSRT_HD uint32_t rsrt_video_quantise(float v, float lo, float hi, float t)
{
    v = v < lo ? lo : (v > hi ? hi : v);
    float q = floorf((v + 0.5f) + t);
    q = q < lo ? lo : (q > hi ? hi : q);
    return (uint32_t)q;
}

/* steps 5: the luma code of pixel (x, y) from its Y', and the two chroma codes of sample (cx, cy) from its reduced Cb', Cr' */
RSRT_HD uint32_t rsrt_video_luma_code(float y, uint32_t px, uint32_t py, const rsrt_video_params *p)
{
    float lo, hi;
    const float v = rsrt_video_luma_value(y, p->depth, p->range, &lo, &hi);
    return rsrt_video_quantise(v, lo, hi, rsrt_video_dither(p->dither, p->dither > 0.0f ? rsrt_finish_hash_base(px, py, p->seed) : 0u, 1u));
}
RSRT_HD void rsrt_video_chroma_codes(float cb, float cr, uint32_t cx, uint32_t cy, const rsrt_video_params *p, uint32_t out[2])
{
    float lo, hi;
    const uint32_t base = p->dither > 0.0f ? rsrt_finish_hash_base(cx, cy, p->seed) : 0u;
    const float vb = rsrt_video_chroma_value(cb, p->depth, p->range, &lo, &hi), vr = rsrt_video_chroma_value(cr, p->depth, p->range, &lo, &hi);
    out[0] = rsrt_video_quantise(vb, lo, hi, rsrt_video_dither(p->dither, base, 3u));
    out[1] = rsrt_video_quantise(vr, lo, hi, rsrt_video_dither(p->dither, base, 5u));
}

/* step 6.  Plane 0 is the luma; RSRT_VIDEO_SEMIPLANAR has one more (interleaved Cb, Cr: `width` counts its samples, two a pair),
 * RSRT_VIDEO_PLANAR two (Cb, Cr); what a layout has not got is zero.  pitch = width * bytes a sample. */
typedef struct rsrt_video_planes_out {
    uint64_t offset[3], pitch[3]; /* bytes */
    uint32_t width[3], height[3]; /* samples */
    uint32_t planes, sample_bytes;
} rsrt_video_planes_out;

/* the frame's byte count (0 for a size of 0 or params rsrt_video_params_ok refuses); out may be NULL */
RSRT_HD size_t rsrt_video_planes(uint32_t width, uint32_t height, const rsrt_video_params *p, rsrt_video_planes_out *out)
{
    rsrt_video_planes_out o;
    for (int i = 0; i < 3; i++) o.offset[i] = o.pitch[i] = o.width[i] = o.height[i] = 0u;
    o.planes = o.sample_bytes = 0u;
    uint64_t at = 0u;
    if (width && height && rsrt_video_params_ok(p)) {
        const uint32_t cw = width / 2u + width % 2u, ch = height / 2u + height % 2u;
        o.sample_bytes = p->depth == 10u ? 2u : 1u;
        o.planes = p->layout == RSRT_VIDEO_PLANAR ? 3u : 2u;
        for (uint32_t i = 0; i < o.planes; i++) {
            o.width[i] = i == 0u ? width : (o.planes == 2u ? 2u * cw : cw);
            o.height[i] = i == 0u ? height : ch;
            o.pitch[i] = (uint64_t)o.width[i] * o.sample_bytes;
            o.offset[i] = at;
            at += o.pitch[i] * o.height[i];
        }
    }
    if (out) *out = o;
    return (size_t)at;
}

/* the word a code is stored as */
RSRT_HD uint32_t rsrt_video_word(uint32_t code, const rsrt_video_params *p) { return p->depth == 10u && p->layout == RSRT_VIDEO_SEMIPLANAR ? code << 6 : code; }

#endif
