/*
 * rsrt_finish.h — arithmetic of the finished display (rsrt_display_finished_srgb8; include/rsrt.h "finished display"), as shared inline
 * code: what happens to a pixel AFTER the tone map and the LUT and before it is a byte — a contrast-adaptive sharpener, film grain and a
 * dithered quantiser.
 *
 * The sharpener is FSR 1's RCAS (AMD FidelityFX Super Resolution 1.0, "robust contrast-adaptive sharpening"), the grain its LFGA shaping,
 * the dither a triangular-PDF dither of one code's amplitude (Lipshitz, Wannamaker, Vanderkooy 1992) over the sRGB thresholds.  All three
 * are display-referred: they work on the tone-mapped colour in the square-root domain the colour LUT already uses.  Like rsrt_colour.h
 * this is part of the published numeric contract: floats are plain f32 + - * / and rsrt_sqrtf (-ffp-contract=off, nothing fused) in
 * exactly the order written here, min(a, b) is a < b ? a : b and max(a, b) is a > b ? a : b, the noise is an integer hash, and a numpy
 * restatement reproduces every bit and byte (tests/finish_ref.py holds it).
 *
 * 1. sdr (rsrt_finish_sdr): rsrt_display_sdr_colour (rsrt_colour.h), the tone-mapped, graded colour of a pixel that
 *    rsrt_display_pixel_colour encodes: f16-rounded mean times exposure, plus intensity * up(B), times the local gain, times the white
 *    point, rsrt_aces_tone_map, rsrt_colour_grade with lut_strength > 0.
 * 2. record (rsrt_finish_record), 4 floats a pixel:  s = sdr > 0 ? (sdr > 1 ? 1 : sdr) : 0  (NaN, -0 and negatives give +0; the clamp is
 *    byte-neutral for the quantiser),  enc = rsrt_sqrtf(s)  per channel, and the luma  L = (0.5f * enc.r + enc.g) + 0.5f * enc.b
 *    (RCAS's: green whole, red and blue halved; 0 .. 2).
 * 3. sharpen (rsrt_finish_sharpen; skipped with sharpness 0, o = enc then) over the cross b (x, y - 1), d (x - 1, y), e (x, y),
 *    f (x + 1, y), h (x, y + 1), coordinates clamped to the picture.  Per channel:
 *      mn4 = min(min(b, d), min(f, h)),  mx4 = max(max(b, d), max(f, h))
 *      lobe_c = 0  when mx4 == 0 (the ring is all 0: 0 / 0) or mn4 == 1 (the ring is all 1: 0 / 0), else
 *      hitMin = mn4 / (4.0f * mx4),  hitMax = (1.0f - mx4) / (4.0f * mn4 - 4.0f),  lobe_c = max(-hitMin, hitMax)
 *    (with mx4 > 0 and mn4 < 1 both divisors are non-zero and both quotients lie in [0, 0.25] and [-0.25, 0]).  Then
 *      lobe = max(-0.1875f, min(max(max(lobe_r, lobe_g), lobe_b), 0.0f)) * sharpness
 *    and under RSRT_FINISH_NOISE_AWARE, with the records' lumas,  mx5 / mn5 = max / min over bL, dL, eL, fL, hL (in that order),
 *      range = mx5 - mn5;  a = 0.25f * ((bL + dL) + (fL + hL)) - eL;  a = a < 0 ? -a : a;
 *      lobe = lobe * (range > 0 ? 1.0f - 0.5f * min(a / range, 1.0f) : 1.0f)           RCAS's optional limiter
 *    and per channel
 *      o = e + (lobe * (((b + d) + (f + h)) - 4.0f * e)) / (4.0f * lobe + 1.0f),  clamped to [0, 1].
 *    4 lobe + 1 lies in [0.25, 1].  On a flat cross (b + d) + (f + h) and 4 e are the same exact number, so o is e bit for bit; so it
 *    is with sharpness 0.  Every input in [0, 1] gives a finite result in [0, 1].
 * 4. hash:  pcg(v):  s = v * 747796405u + 2891336453u;  w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;  (w >> 22) ^ w   (PCG-RXS-M-XS 32)
 *      rsrt_finish_hash(x, y, seed, k) = pcg(pcg(pcg(pcg(x) + y) + seed) + k),  all in uint32 (wrapping);
 *      a uniform in [0, 1) is  (float)(word >> 8) * 2^-24.   Draw k = 0 is the grain's, draws 1 + 2 c and 2 + 2 c are channel c's dither.
 * 5. grain (skipped with grain 0), monochrome:  t = grain * (2.0f * u0 - 1.0f);  per channel  o = o + t * min(o, 1.0f - o)   (LFGA's
 *    shaping: nothing at 0 and 1, at most grain * min(o, 1 - o) anywhere, never outside [0, 1]).
 * 6. back to linear, per channel:  sdr = (o == enc) ? sdr : o * o — a channel that the sharpener and the grain left alone reaches the
 *    quantiser with exactly the value rsrt_display_pixel_colour gives it, a NaN included.
 * 7. quantiser (rsrt_finish_quantise):  b = rsrt_srgb8_encode(x);  the byte is b with dither 0 or b == 0 or b == 255;  otherwise with
 *    lo = T[b - 1], hi = T[b] (RSRT_SRGB8_THRESHOLDS):  p = (x - lo) / (hi - lo),  t = dither * ((u1 + u2) - 1.0f),  v = p + t,
 *    byte = b + (v >= 1) - (v < 0).  With dither 1 the mean byte of a value at p is b + p - 0.5: the continuous code.
 * With sharpness, grain and dither all 0 the bytes are rsrt_display_pixel_colour's.
 */
#ifndef RSRT_FINISH_H
#define RSRT_FINISH_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_finish_params, RSRT_FINISH_NOISE_AWARE */
#include "rsrt_colour.h"

#define RSRT_FINISH_SHARPNESS 0.5f /* rsrt_finish_params defaults */
#define RSRT_FINISH_GRAIN 0.0f
#define RSRT_FINISH_DITHER 1.0f
#define RSRT_FINISH_SEED 0u
#define RSRT_FINISH_FLAGS 0u
#define RSRT_FINISH_LOBE_LIMIT 0.1875f /* RCAS's limit, 0.25 - 1 / 16 */

RSRT_HD int rsrt_finish_params_ok(const rsrt_finish_params *p)
{
    return rsrt_colour_in(p->sharpness, 0.0f, 1.0f) && rsrt_colour_in(p->grain, 0.0f, 1.0f) && rsrt_colour_in(p->dither, 0.0f, 1.0f) &&
           (p->flags & ~(uint32_t)RSRT_FINISH_NOISE_AWARE) == 0u;
}

RSRT_HD float rsrt_finish_min(float a, float b) { return a < b ? a : b; }
RSRT_HD float rsrt_finish_max(float a, float b) { return a > b ? a : b; }

/* step 1: one pixel's sums, up(B) at it (0 where no bloom is asked for), its local gain (1 where none is asked for), the white point
 * and the LUT (looked at only with lut_strength > 0) -> the tone-mapped, graded colour */
RSRT_HD void rsrt_finish_sdr(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float gain,
                             const rsrt_colour_params *colour, const float *lut, uint32_t n, float sdr[3])
{
    rsrt_display_sdr_colour(sum_rgb, total, exposure, intensity, up_b, gain, colour, lut, n, sdr);
}

RSRT_HD float rsrt_finish_luma(const float enc[3]) { return (0.5f * enc[0] + enc[1]) + 0.5f * enc[2]; }

/* step 2: the record of a pixel: enc rgb and its luma */
RSRT_HD void rsrt_finish_record(const float sdr[3], float rec[4])
{
    for (int i = 0; i < 3; i++) rec[i] = rsrt_sqrtf(sdr[i] > 0.0f ? (sdr[i] > 1.0f ? 1.0f : sdr[i]) : 0.0f);
    rec[3] = rsrt_finish_luma(rec);
}

/* step 3: records of the cross -> the sharpened enc rgb of e */
RSRT_HD void rsrt_finish_sharpen(const float b[4], const float d[4], const float e[4], const float f[4], const float h[4], float sharpness, uint32_t flags,
                                 float o[3])
{
    float lobe_c[3];
    for (int i = 0; i < 3; i++) {
        const float mn4 = rsrt_finish_min(rsrt_finish_min(b[i], d[i]), rsrt_finish_min(f[i], h[i]));
        const float mx4 = rsrt_finish_max(rsrt_finish_max(b[i], d[i]), rsrt_finish_max(f[i], h[i]));
        if (mx4 == 0.0f || mn4 == 1.0f) {
            lobe_c[i] = 0.0f;
        } else {
            const float hit_min = mn4 / (4.0f * mx4), hit_max = (1.0f - mx4) / (4.0f * mn4 - 4.0f);
            lobe_c[i] = rsrt_finish_max(-hit_min, hit_max);
        }
    }
    float lobe = rsrt_finish_max(-RSRT_FINISH_LOBE_LIMIT, rsrt_finish_min(rsrt_finish_max(rsrt_finish_max(lobe_c[0], lobe_c[1]), lobe_c[2]), 0.0f)) * sharpness;
    if (flags & RSRT_FINISH_NOISE_AWARE) {
        const float mx5 = rsrt_finish_max(rsrt_finish_max(rsrt_finish_max(rsrt_finish_max(b[3], d[3]), e[3]), f[3]), h[3]);
        const float mn5 = rsrt_finish_min(rsrt_finish_min(rsrt_finish_min(rsrt_finish_min(b[3], d[3]), e[3]), f[3]), h[3]);
        const float range = mx5 - mn5;
        float a = 0.25f * ((b[3] + d[3]) + (f[3] + h[3])) - e[3];
        a = a < 0.0f ? -a : a;
        lobe = lobe * (range > 0.0f ? 1.0f - 0.5f * rsrt_finish_min(a / range, 1.0f) : 1.0f);
    }
    const float den = 4.0f * lobe + 1.0f;
    for (int i = 0; i < 3; i++) o[i] = rsrt_colour_clamp01(e[i] + (lobe * (((b[i] + d[i]) + (f[i] + h[i])) - 4.0f * e[i])) / den);
}

/* step 4 */
RSRT_HD uint32_t rsrt_finish_pcg(uint32_t v)
{
    const uint32_t s = v * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (w >> 22) ^ w;
}

/* what the draws of a pixel share; draw k is rsrt_finish_pcg(base + k) */
RSRT_HD uint32_t rsrt_finish_hash_base(uint32_t x, uint32_t y, uint32_t seed) { return rsrt_finish_pcg(rsrt_finish_pcg(rsrt_finish_pcg(x) + y) + seed); }

RSRT_HD uint32_t rsrt_finish_hash(uint32_t x, uint32_t y, uint32_t seed, uint32_t k) { return rsrt_finish_pcg(rsrt_finish_hash_base(x, y, seed) + k); }

RSRT_HD float rsrt_finish_uniform(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-08f; }

/* step 7: a linear value and two uniforms -> the byte */
RSRT_HD unsigned rsrt_finish_quantise(float x, float dither, float u1, float u2)
{
    const unsigned b = rsrt_srgb8_encode(x);
    if (!(dither > 0.0f) || b == 0u || b == 255u) return b;
    const float lo = RSRT_SRGB8_THRESHOLDS[b - 1u], hi = RSRT_SRGB8_THRESHOLDS[b];
    const float p = (x - lo) / (hi - lo);
    const float t = dither * ((u1 + u2) - 1.0f);
    const float v = p + t;
    return b + (v >= 1.0f ? 1u : 0u) - (v < 0.0f ? 1u : 0u);
}

/* steps 3 and 5: the sharpened, grained enc rgb of the pixel whose record is e; base: rsrt_finish_hash_base of it (read only with grain > 0) */
RSRT_HD void rsrt_finish_shape(const float b[4], const float d[4], const float e[4], const float f[4], const float h[4], uint32_t base, const rsrt_finish_params *p,
                               float o[3])
{
    if (p->sharpness > 0.0f) {
        rsrt_finish_sharpen(b, d, e, f, h, p->sharpness, p->flags, o);
    } else {
        for (int i = 0; i < 3; i++) o[i] = e[i];
    }
    if (p->grain > 0.0f) {
        const float t = p->grain * (2.0f * rsrt_finish_uniform(rsrt_finish_pcg(base)) - 1.0f);
        for (int i = 0; i < 3; i++) o[i] = o[i] + t * rsrt_finish_min(o[i], 1.0f - o[i]);
    }
}

/* steps 3 to 7: the pixel (x, y) from its sdr (step 1), its record e and the records of its cross (looked at only with sharpness > 0) */
RSRT_HD void rsrt_finish_pixel(const float sdr[3], const float b[4], const float d[4], const float e[4], const float f[4], const float h[4], uint32_t x, uint32_t y,
                               const rsrt_finish_params *p, unsigned char out_rgb[3])
{
    float o[3];
    const uint32_t base = (p->grain > 0.0f || p->dither > 0.0f) ? rsrt_finish_hash_base(x, y, p->seed) : 0u;
    rsrt_finish_shape(b, d, e, f, h, base, p, o);
    for (int i = 0; i < 3; i++) {
        const float lin = o[i] == e[i] ? sdr[i] : o[i] * o[i];
        float u1 = 0.0f, u2 = 0.0f;
        if (p->dither > 0.0f) {
            u1 = rsrt_finish_uniform(rsrt_finish_pcg(base + 1u + 2u * (uint32_t)i));
            u2 = rsrt_finish_uniform(rsrt_finish_pcg(base + 2u + 2u * (uint32_t)i));
        }
        out_rgb[i] = (unsigned char)rsrt_finish_quantise(lin, p->dither, u1, u2);
    }
}

#endif
