/*
 * rsrt_exposure.h — arithmetic of the auto-exposure meter and the exposed display (rsrt_exposure_meter, rsrt_exposure_download,
 * rsrt_display_exposed_srgb8; include/rsrt.h), as shared inline code.
 *
 * The meter is the log-average ("key") meter of Reinhard, Stark, Shirley, Ferwerda, "Photographic Tone Reproduction for Digital
 * Images" (SIGGRAPH 2002) — exposure = key / exp(mean(log L)) — with the histogram trimming that engines use: the darkest
 * low_permille and the brightest 1000 - high_permille of the metered pixels do not count.  No logarithm is taken: the bit pattern of
 * a positive float, read as an integer, is a piecewise-linear log2 (Mitchell's approximation: exact at powers of two, at most 0.086
 * octave low in between, and partly cancelling in key / average because both ends go through the same map).  Pixels are quantised
 * to 1/8 octave, so a uniform image reads up to half a bin, about 4 %, high or low.  Like rsrt_noise.h this is part of the
 * published numeric contract: plain f32 * + / (-ffp-contract=off, nothing fused) for a pixel's luminance and for the exposure,
 * everything in between in integers — so the histogram does not depend on the order pixels are counted in, and a numpy restatement
 * reproduces every word and every result bit (tests/exposure_ref.py holds it).
 *
 * Luminance of a pixel of an image of sums (the accumulator: total = (float)sample_total; every other source: total = 1):
 *   c = sum.rgb / total                                       one f32 division a channel
 *   L = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b        rsrt_sv_lum's expression
 * Bin of a pixel: a pixel with !(L > 0) — zero, negative, NaN — is skipped; otherwise
 *   b   = bits(L) >> 20                                       8 exponent bits, 3 mantissa bits: eight bins an octave
 *   bin = min(max(b, RSRT_EXPOSURE_LO), RSRT_EXPOSURE_LO + 255) - RSRT_EXPOSURE_LO      RSRT_EXPOSURE_LO = 888: 2^-16
 * so the bins cover 2^-16 .. 2^16; denormals and anything below land in bin 0, +inf and anything above in bin 255.
 * Histogram: 257 uint32 words — 256 bin counts, then [256] the skipped pixels; the words sum to the pixel count.
 *
 * Exposure from a histogram (rsrt_exposure_from_histogram; pure, in uint64):
 *   N = sum of hist[0..255];  a = N * low_permille / 1000 (floor),  b = (N * high_permille + 999) / 1000 (ceil)
 *   pixels are ranked by bin: bin i holds ranks [cum_i, cum_i + hist[i]);  S = sum of i * |[cum_i, cum_i + hist[i]) ^ [a, b)|,  M = b - a
 *   bits_avg = (RSRT_EXPOSURE_LO << 20) + (1 << 19) + (S << 20) / M      the centre of the mean bin position (S << 20 < 2^60 for
 *                                                                        frames up to 16384 x 16384)
 *   average_luminance = as_float(bits_avg)
 *   target   = key / average_luminance, then  target < min_exposure ? min_exposure : (max_exposure < target ? max_exposure : target)
 *   exposure = previous_exposure > 0 ? previous_exposure + (target - previous_exposure) * blend : target
 *   N == 0 (nothing metered): metered = 0, average_luminance = 0, target = exposure = (previous_exposure > 0 ? previous_exposure : 1)
 * The library keeps no exposure: adaptation over time is the caller handing the last exposure back as previous_exposure.
 *
 * Exposed display pixel: mean = rsrt_display_mean (rsrt_tonemap.h), hdr = mean * exposure (rsrt_display_hdr_exposed), then
 * rsrt_aces_tone_map and rsrt_display_encode.  With exposure 1 the multiply is exact and the bytes are rsrt_display_pixel's.
 */
#ifndef RSRT_EXPOSURE_H
#define RSRT_EXPOSURE_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_exposure_params, rsrt_exposure_result */
#include "rsrt_tonemap.h"

#define RSRT_EXPOSURE_BINS 256u
#define RSRT_EXPOSURE_WORDS 257u          /* the bins, then the skipped pixels */
#define RSRT_EXPOSURE_LO 888u             /* bits(2^-16) >> 20 */
#define RSRT_EXPOSURE_LOW_PERMILLE 100u   /* rsrt_exposure_params defaults */
#define RSRT_EXPOSURE_HIGH_PERMILLE 950u
#define RSRT_EXPOSURE_KEY 0.18f
#define RSRT_EXPOSURE_MIN 1.52587890625e-05f /* 2^-16 */
#define RSRT_EXPOSURE_MAX 65536.0f           /* 2^16 */
#define RSRT_EXPOSURE_BLEND 1.0f
#define RSRT_EXPOSURE_PREVIOUS 0.0f

RSRT_HD uint32_t rsrt_exposure_bits(float x)
{
    union { float f; uint32_t u; } v;
    v.f = x;
    return v.u;
}

RSRT_HD float rsrt_exposure_as_float(uint32_t u)
{
    union { float f; uint32_t u; } v;
    v.u = u;
    return v.f;
}

/* the luminance the meter sees of a pixel of sums */
RSRT_HD float rsrt_exposure_luminance(const float sum[3], float total)
{
    const float c0 = sum[0] / total, c1 = sum[1] / total, c2 = sum[2] / total;
    return (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2;
}

/* the histogram word a luminance counts in: its bin, or 256 (skipped) */
RSRT_HD uint32_t rsrt_exposure_word(float L)
{
    if (!(L > 0.0f)) return RSRT_EXPOSURE_BINS;
    const uint32_t b = rsrt_exposure_bits(L) >> 20;
    const uint32_t lo = b < RSRT_EXPOSURE_LO ? RSRT_EXPOSURE_LO : b;
    return (lo > RSRT_EXPOSURE_LO + 255u ? RSRT_EXPOSURE_LO + 255u : lo) - RSRT_EXPOSURE_LO;
}

RSRT_HD int rsrt_exposure_finite_positive(float x) { return x > 0.0f && x < __builtin_inff(); }

RSRT_HD int rsrt_exposure_params_ok(const rsrt_exposure_params *p)
{
    return p->low_permille < p->high_permille && p->high_permille <= 1000u && rsrt_exposure_finite_positive(p->key) &&
           rsrt_exposure_finite_positive(p->min_exposure) && rsrt_exposure_finite_positive(p->max_exposure) &&
           p->min_exposure <= p->max_exposure && p->blend >= 0.0f && p->blend <= 1.0f &&
           (p->previous_exposure == 0.0f || rsrt_exposure_finite_positive(p->previous_exposure));
}

/* the exposure of a histogram of RSRT_EXPOSURE_WORDS words; p must pass rsrt_exposure_params_ok */
RSRT_HD void rsrt_exposure_from_histogram(const uint32_t *hist, const rsrt_exposure_params *p, rsrt_exposure_result *out)
{
    uint64_t N = 0;
    for (uint32_t i = 0; i < RSRT_EXPOSURE_BINS; i++) N += hist[i];
    out->metered = (uint32_t)N;
    out->skipped = hist[RSRT_EXPOSURE_BINS];
    out->_pad = 0;
    if (N == 0) {
        out->average_luminance = 0.0f;
        out->target = out->exposure = p->previous_exposure > 0.0f ? p->previous_exposure : 1.0f;
        return;
    }
    const uint64_t a = N * p->low_permille / 1000u, b = (N * p->high_permille + 999u) / 1000u;
    uint64_t S = 0, cum = 0;
    for (uint32_t i = 0; i < RSRT_EXPOSURE_BINS; i++) {
        const uint64_t lo = cum > a ? cum : a, end = cum + hist[i], hi = end < b ? end : b;
        if (hi > lo) S += (uint64_t)i * (hi - lo);
        cum = end;
    }
    const uint32_t bits_avg = (RSRT_EXPOSURE_LO << 20) + (1u << 19) + (uint32_t)((S << 20) / (b - a));
    out->average_luminance = rsrt_exposure_as_float(bits_avg);
    float target = p->key / out->average_luminance;
    target = target < p->min_exposure ? p->min_exposure : (p->max_exposure < target ? p->max_exposure : target);
    out->target = target;
    out->exposure = p->previous_exposure > 0.0f ? p->previous_exposure + (target - p->previous_exposure) * p->blend : target;
}

/* the display chain's second step: the f16-rounded mean times the exposure */
RSRT_HD void rsrt_display_hdr_exposed(const float sum_rgb[3], float total, float exposure, float hdr[3])
{
    rsrt_display_mean(sum_rgb, total, hdr);
    for (int i = 0; i < 3; i++) hdr[i] = hdr[i] * exposure;
}

/* one pixel: sums (f32) -> display bytes at an exposure */
RSRT_HD void rsrt_display_pixel_exposed(const float sum_rgb[3], float total, float exposure, unsigned char out_rgb[3])
{
    float hdr[3], sdr[3];
    rsrt_display_hdr_exposed(sum_rgb, total, exposure, hdr);
    rsrt_aces_tone_map(hdr, sdr);
    rsrt_display_encode(sdr, out_rgb);
}

#endif
