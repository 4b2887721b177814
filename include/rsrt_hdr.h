/*
 * rsrt_hdr.h — arithmetic of the HDR display (rsrt_display_hdr; include/rsrt.h "HDR display"), as shared inline code: what happens to a
 * pixel's linear colour when the output is an HDR surface instead of an sRGB byte — a hue-preserving shoulder below the display's peak,
 * the scale to nits, and the SMPTE ST 2084 (PQ) 10-bit or the scRGB binary16 encoding, with the frame's content light levels
 * (CTA-861.3) on the side.
 *
 * Like rsrt_finish.h this is part of the published numeric contract: floats are plain f32 + - * / (-ffp-contract=off, nothing fused) in
 * exactly the order written here, min(a, b) is a < b ? a : b and max(a, b) is a > b ? a : b, the PQ curve is a threshold search (no pow
 * at run time), the dither's noise is rsrt_finish.h's integer hash, the light levels are integer reductions, and a numpy restatement
 * reproduces every bit and word (tests/hdr_ref.py holds it).
 *
 * 1. linear colour (rsrt_hdr_linear):  rsrt_display_hdr_local (rsrt_local.h: the f16-rounded mean times exposure, plus intensity * up(B),
 *    times the local gain), times colour->white per channel — exactly what rsrt_display_sdr_colour hands to rsrt_aces_tone_map.  Linear
 *    Rec.709, 1.0 = paper white.  The colour LUT is display-referred SDR and is not applied (the entry point refuses lut_strength > 0).
 * 2. sanitise (rsrt_hdr_sanitise), per channel:  x = x > 0 ? (x > RSRT_HDR_CAP ? RSRT_HDR_CAP : x) : 0 — NaN, -0 and negatives give +0
 *    (no magenta marker here), +inf gives the cap, 2^64: a power of two, so that c / m and m * (c / m) below are exact at the cap.  No NaN
 *    and no infinity passes this step.
 * 3. range compression (rsrt_hdr_compress), in units of paper white, on m = max(max(r, g), b):
 *      P = peak_nits / paper_white_nits,  k = knee * P,  d = P - k                        (rsrt_hdr_curve_of; d > 0 as knee <= 0.95)
 *      m <= k: the pixel passes, bit for bit (nothing is multiplied by a computed 1);
 *      m >  k: e = m - k,  c = k + d * (e / (d + e)),  s = c / m,  every channel x = x * s.
 *    e / (d + e) lies in (0, 1] and cannot overflow; the curve has slope 1 at the knee and the asymptote P.  One factor for the three
 *    channels: their ratios stay (to the two roundings of the two products).  In f32 c carries four roundings and m * (c / m) two more:
 *    where the curve has flattened to less than that between two inputs (seen from some seventy d above the knee on) a brighter input
 *    may come out an ulp or two darker; over the sweeps of tests/test_hdr.py no code and no half of step 5 steps back.
 * 4. nits (rsrt_hdr_to_nits), per channel:  n = paper_white_nits * x,  n = n > peak_nits ? peak_nits : n.
 * 5. encoding.
 *    RSRT_HDR_PQ10:  Rec.709 -> Rec.2020 by BT.2087's matrix, rows (0.6274, 0.3293, 0.0433), (0.0691, 0.9195, 0.0114), (0.0164, 0.0880,
 *      0.8956), as rsrt_mat3_mul associates: (row.r * n.r + row.g * n.g) + row.b * n.b; clamped to peak_nits again (the rows sum to 1, a
 *      rounding may pass it).  code = rsrt_pq10_encode(n) = the number of RSRT_PQ10_THRESHOLDS <= n (rsrt_pq_table.h), a binary search.
 *      The word is R | G << 10 | B << 20 | 3u << 30.
 *    RSRT_HDR_SCRGB16F:  stays Rec.709;  v = n / 80.0f,  the half is v rounded to binary16, ties to even (rsrt_hdr_f16_bits: the bits of
 *      rsrt_round_to_f16; a device may use its own round-to-nearest-even conversion);  the pixel is (r, g, b, 0x3C00), four uint16.
 * 6. dither (rsrt_hdr_quantise; RSRT_HDR_PQ10 with dither > 0): rsrt_finish_quantise over the PQ thresholds.  b = rsrt_pq10_encode(n);
 *    the code is b with b == 0 or b == 1023;  otherwise with lo = T[b - 1], hi = T[b]:  p = (n - lo) / (hi - lo),
 *    t = dither * ((u1 + u2) - 1.0f),  v = p + t,  code = b + (v >= 1) - (v < 0)  (a value inside the peak's own code may so land one
 *    code above it; without dither no code passes the peak's).  The draws are rsrt_finish.h's:
 *    base = rsrt_finish_hash_base(x, y, seed),  channel c takes u1, u2 = rsrt_finish_uniform(rsrt_finish_pcg(base + 1 + 2 c)), (... + 2 + 2 c).
 * 7. content light levels.  Per pixel  L = max(max(R, G), B)  of the nits of step 5 (before the dither, in the encoding's primaries),
 *    q = (uint32_t)(L * 64.0f)  (at most 640000).  The frame's max_q (uint32) and sum_q (uint64) are integer reductions: no order of
 *    anything changes them.  rsrt_hdr_levels_from:  max_cll = max_q / 64,  max_fall = sum_q / (64 * pixels),  in double, then to float.
 */
#ifndef RSRT_HDR_H
#define RSRT_HDR_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_hdr_params, rsrt_hdr_levels, RSRT_HDR_PQ10, RSRT_HDR_SCRGB16F */
#include "rsrt_finish.h"
#include "rsrt_pq_table.h"

#define RSRT_HDR_PAPER_WHITE 203.0f /* rsrt_hdr_params defaults; BT.2408's HDR reference white */
#define RSRT_HDR_PEAK 1000.0f
#define RSRT_HDR_KNEE 0.5f
#define RSRT_HDR_DITHER 0.0f
#define RSRT_HDR_SEED 0u
#define RSRT_HDR_ENCODING RSRT_HDR_PQ10
#define RSRT_HDR_FLAGS 0u
#define RSRT_HDR_CAP 18446744073709551616.0f /* 2^64: what a channel is capped at, in paper whites */
#define RSRT_HDR_MAX_NITS 10000.0f           /* ST 2084's range */
#define RSRT_HDR_SCRGB_NITS 80.0f            /* scRGB's 1.0 */
#define RSRT_HDR_LEVEL_SCALE 64.0f           /* the light levels count 1 / 64 cd/m^2 */

RSRT_HD int rsrt_hdr_params_ok(const rsrt_hdr_params *p)
{
    return rsrt_colour_in(p->paper_white_nits, 1.0f, RSRT_HDR_MAX_NITS) && rsrt_colour_in(p->peak_nits, p->paper_white_nits, RSRT_HDR_MAX_NITS) &&
           rsrt_colour_in(p->knee, 0.0f, 0.95f) && rsrt_colour_in(p->dither, 0.0f, 1.0f) &&
           (p->encoding == RSRT_HDR_PQ10 || (p->encoding == RSRT_HDR_SCRGB16F && !(p->dither > 0.0f))) && p->flags == 0u;
}

/* step 1: one pixel's sums, up(B) at it (0 where no bloom is asked for), its local gain (1 where none is asked for) and the white point
 * -> linear Rec.709 in paper whites */
RSRT_HD void rsrt_hdr_linear(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                             const rsrt_colour_params *colour, float lin[3])
{
    rsrt_display_hdr_local(sum_rgb, total, exposure, intensity, up_b, gain, lin);
    for (int i = 0; i < 3; i++) lin[i] = lin[i] * colour->white[i];
}

/* step 2, in place */
RSRT_HD void rsrt_hdr_sanitise(float x[3])
{
    for (int i = 0; i < 3; i++) x[i] = x[i] > 0.0f ? (x[i] > RSRT_HDR_CAP ? RSRT_HDR_CAP : x[i]) : 0.0f;
}

typedef struct rsrt_hdr_curve {
    float P, k, d; /* the peak, the knee and their distance, in paper whites */
} rsrt_hdr_curve;

RSRT_HD rsrt_hdr_curve rsrt_hdr_curve_of(const rsrt_hdr_params *p)
{
    rsrt_hdr_curve c;
    c.P = p->peak_nits / p->paper_white_nits;
    c.k = p->knee * c.P;
    c.d = c.P - c.k;
    return c;
}

/* step 3, in place: x sanitised */
RSRT_HD void rsrt_hdr_compress(const rsrt_hdr_curve *cv, float x[3])
{
    const float m = rsrt_finish_max(rsrt_finish_max(x[0], x[1]), x[2]);
    if (m <= cv->k) return;
    const float e = m - cv->k;
    const float c = cv->k + cv->d * (e / (cv->d + e));
    const float s = c / m;
    for (int i = 0; i < 3; i++) x[i] = x[i] * s;
}

/* step 4 */
RSRT_HD void rsrt_hdr_to_nits(const float x[3], float paper_white_nits, float peak_nits, float nits[3])
{
    for (int i = 0; i < 3; i++) {
        const float n = paper_white_nits * x[i];
        nits[i] = n > peak_nits ? peak_nits : n;
    }
}

/* step 5, RSRT_HDR_PQ10: Rec.709 nits -> Rec.2020 nits */
RSRT_HD void rsrt_hdr_to_rec2020(const float nits[3], float peak_nits, float out[3])
{
    const float c0[3] = {0.6274f, 0.0691f, 0.0164f}, c1[3] = {0.3293f, 0.9195f, 0.0880f}, c2[3] = {0.0433f, 0.0114f, 0.8956f}; /* the columns */
    rsrt_mat3_mul(c0, c1, c2, nits, out);
    for (int i = 0; i < 3; i++) out[i] = out[i] > peak_nits ? peak_nits : out[i];
}

/* number of PQ thresholds <= nits (NaN -> 0) */
RSRT_HD unsigned rsrt_pq10_encode(float nits)
{
    unsigned lo = 0, hi = 1023; /* invariant: T[lo-1] <= nits < T[hi] with T[-1] = -inf, T[1023] = +inf */
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if (nits >= RSRT_PQ10_THRESHOLDS[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* step 6: nits and two uniforms -> the 10-bit code; rsrt_finish_quantise over the PQ thresholds */
RSRT_HD unsigned rsrt_hdr_quantise(float nits, float dither, float u1, float u2)
{
    const unsigned b = rsrt_pq10_encode(nits);
    if (!(dither > 0.0f) || b == 0u || b == 1023u) return b;
    const float lo = RSRT_PQ10_THRESHOLDS[b - 1u], hi = RSRT_PQ10_THRESHOLDS[b];
    const float p = (nits - lo) / (hi - lo);
    const float t = dither * ((u1 + u2) - 1.0f);
    const float v = p + t;
    return b + (v >= 1.0f ? 1u : 0u) - (v < 0.0f ? 1u : 0u);
}

/* the bits of the binary16 nearest to f, ties to even: rsrt_round_to_f16's value as the half that holds it */
RSRT_HD uint16_t rsrt_hdr_f16_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    union { _Float16 h; uint16_t u; } dev; /* the device's own conversion: round to nearest even, half denormals kept */
    dev.h = (_Float16)f;
    return dev.u;
#else
    union { float f; uint32_t u; } r;
    r.f = rsrt_round_to_f16(f);
    const uint16_t sign = (uint16_t)((r.u >> 16) & 0x8000u);
    const uint32_t a = r.u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);  /* NaN */
    if (a == 0x7f800000u) return (uint16_t)(sign | 0x7c00u); /* inf, and what rounds past 65504 */
    if (a >= 0x38800000u) return (uint16_t)(sign | (((a >> 23) - 112u) << 10) | ((a >> 13) & 0x3ffu)); /* a normal half */
    r.u = a;
    return (uint16_t)(sign | (uint32_t)(r.f * 16777216.0f)); /* a multiple of 2^-24 below 2^-14: its count */
#endif
}

/* steps 2 to 5: the linear colour of step 1 -> nits in the encoding's primaries (Rec.2020 for RSRT_HDR_PQ10, Rec.709 for
 * RSRT_HDR_SCRGB16F): what the quantiser and the light levels take; p must pass rsrt_hdr_params_ok */
RSRT_HD void rsrt_hdr_nits_of(const float lin[3], const rsrt_hdr_params *p, float nits[3])
{
    float x[3] = {lin[0], lin[1], lin[2]}, n[3];
    rsrt_hdr_sanitise(x);
    const rsrt_hdr_curve cv = rsrt_hdr_curve_of(p);
    rsrt_hdr_compress(&cv, x);
    rsrt_hdr_to_nits(x, p->paper_white_nits, p->peak_nits, n);
    if (p->encoding == RSRT_HDR_PQ10) {
        rsrt_hdr_to_rec2020(n, p->peak_nits, nits);
    } else {
        for (int i = 0; i < 3; i++) nits[i] = n[i];
    }
}

/* steps 1 to 5 of a pixel */
RSRT_HD void rsrt_hdr_pixel_nits(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                                 const rsrt_colour_params *colour, const rsrt_hdr_params *p, float nits[3])
{
    float lin[3];
    rsrt_hdr_linear(sum_rgb, total, exposure, intensity, up_b, gain, colour, lin);
    rsrt_hdr_nits_of(lin, p, nits);
}

/* steps 5 and 6, RSRT_HDR_PQ10: the Rec.2020 nits of pixel (x, y) -> its word */
RSRT_HD uint32_t rsrt_hdr_pack_pq10(const float nits[3], uint32_t x, uint32_t y, const rsrt_hdr_params *p)
{
    uint32_t word = 3u << 30;
    const uint32_t base = p->dither > 0.0f ? rsrt_finish_hash_base(x, y, p->seed) : 0u;
    for (int i = 0; i < 3; i++) {
        float u1 = 0.0f, u2 = 0.0f;
        if (p->dither > 0.0f) {
            u1 = rsrt_finish_uniform(rsrt_finish_pcg(base + 1u + 2u * (uint32_t)i));
            u2 = rsrt_finish_uniform(rsrt_finish_pcg(base + 2u + 2u * (uint32_t)i));
        }
        word |= (uint32_t)rsrt_hdr_quantise(nits[i], p->dither, u1, u2) << (10 * i);
    }
    return word;
}

/* step 5, RSRT_HDR_SCRGB16F: the Rec.709 nits of a pixel -> its four halfs */
RSRT_HD void rsrt_hdr_pack_scrgb(const float nits[3], uint16_t out[4])
{
    for (int i = 0; i < 3; i++) out[i] = rsrt_hdr_f16_bits(nits[i] / RSRT_HDR_SCRGB_NITS);
    out[3] = 0x3c00u;
}

/* step 7: a pixel's count */
RSRT_HD uint32_t rsrt_hdr_level_q(const float nits[3])
{
    return (uint32_t)(rsrt_finish_max(rsrt_finish_max(nits[0], nits[1]), nits[2]) * RSRT_HDR_LEVEL_SCALE);
}

/* ... and the frame's levels from the two reductions */
RSRT_HD void rsrt_hdr_levels_from(uint32_t max_q, uint64_t sum_q, uint64_t pixels, rsrt_hdr_levels *out)
{
    out->sum_q = sum_q;
    out->max_q = max_q;
    out->max_cll = (float)((double)max_q / 64.0);
    out->max_fall = (float)((double)sum_q / (64.0 * (double)pixels));
    out->_pad = 0u;
}

#endif
