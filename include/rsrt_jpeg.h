/*
 * rsrt_jpeg.h — arithmetic of the JPEG pass (rsrt_display_jpeg; include/rsrt.h "JPEG output"), as shared inline code: what happens to a
 * pixel's display colour when the output is a baseline JPEG / JFIF file — the continuous sRGB code, JFIF's matrix, the chroma
 * reduction, the 8 x 8 forward DCT, the quantiser, the order of the blocks, the Huffman code and the file around the scan.
 *
 * Like rsrt_video.h this is part of the published numeric contract: floats are plain f32 + - * /, floorf and fabsf (-ffp-contract=off,
 * nothing fused) in exactly the order written here, and a numpy restatement reproduces every byte (tests/jpeg_ref.py holds it).  The
 * tables are include/rsrt_jpeg_table.h's.
 *
 * 1. input, three channels: rsrt_finish_sdr (rsrt_finish.h step 1), the tone-mapped, graded colour rsrt_display_colour_srgb8 quantises,
 *    LUT included.  E' = rsrt_video_signal(RSRT_VIDEO_BT709, ..) of it (rsrt_video.h step 2): the continuous 8-bit sRGB code over 255, in
 *    [0, 1], finite for every input, 0 for NaN, -0 and negatives.  Baseline JPEG is 8-bit SDR: there is no HDR variant.
 * 2. matrix (rsrt_jpeg_samples), JFIF's: BT.601, full range — not the video pass's BT.709.
 *      Y' = (0.299f * R' + 0.587f * G') + 0.114f * B',   Cb' = (B' - Y') / 1.772f,   Cr' = (R' - Y') / 1.402f
 *    samples, level-shifted, floats (the DCT takes the unquantised sample):
 *      sY = 255.0f * Y' - 128.0f in [-128, 127],   sCb = 255.0f * Cb',   sCr = 255.0f * Cr', both in [-127.5, 127.5] (an ulp or two more in f32)
 *    A grey R' = G' = B' does NOT give exactly zero chroma: the three products' sum is the channel to within two ulp, so |sCb| and
 *    |sCr| stay below 1e-4 — and every chroma coefficient of a grey picture is below 1e-3 and quantises to 0 at every quality.
 * 3. subsampling.  RSRT_JPEG_420: MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr; a chroma sample (cx, cy) is rsrt_video_centre of the float
 *    sCb (sCr) of pixels (2 cx .., 2 cy ..): ((p00 + p01) + (p10 + p11)) * 0.25f.  RSRT_JPEG_444: MCU 8 x 8, blocks Y Cb Cr.  Every
 *    pixel coordinate is clamped to the picture (edge replicate): partial MCUs, odd sizes and 1 x 1 are legal.
 * 4. forward DCT (rsrt_jpeg_fdct) with D = RSRT_JPEG_DCT, separable, along x first:
 *      t[y][u] = dot(D[u], s[y][.]),   c[v][u] = dot(D[v], t[.][u]),   dot(d, a):  acc = d[0] * a[0];  acc = acc + d[k] * a[k], k = 1 .. 7
 *    No fast factorisation and no MFMA: the order of the sums is the contract.  With |s| <= 128 a DC is 8 * mean, in [-1024, 1016] for luma and [-1020, 1020] for chroma, and an
 *    AC's magnitude at most 1020 (a row of D sums to at most 2 sqrt 2 in magnitude, squared 8, times the samples' half range 127.5), a
 *    few 1e-4 more in f32.
 * 5. quantiser.  Q = rsrt_jpeg_q(base, quality), Annex K's tables the IJG way, integers:  s = quality < 50 ? 5000 / quality :
 *    200 - 2 * quality,  Q = clamp((base * s + 50) / 100, 1, 255).  q = sign(c) * floorf(fabsf(c) / Q + 0.5f), then clamped to
 *    [-1023, 1023], a DC to [-1024, 1023].  By step 4's bound the clamp never acts on a picture's coefficients; it stays as the guard
 *    that keeps every symbol inside the baseline tables.  Output: int16 in zigzag order, 64 a block.
 * 6. scan order.  MCUs left to right, top to bottom; the blocks of an MCU as in step 3; block i of the picture is i-th in that order.  A
 *    block's DC predictor is the DC of the previous block of its component, 0 for the first: rsrt_jpeg_block_pred gives that block's
 *    index (or -1) by arithmetic, no running state.
 * 7. entropy code (T.81 F.1.2) with the four Annex K typical tables.  A block: the DC difference's size code and its bits; for every
 *    non-zero AC after a run of r zeros, r / 16 times ZRL (0xF0), then the symbol (r % 16) << 4 | size and the value's bits; EOB (0x00)
 *    unless coefficient 63 is non-zero.  A value's bits are v, or v - 1 for a negative, in size = bit length of |v| bits.  At most
 *    20 + 63 * 26 = 1658 bits a block (RSRT_JPEG_BLOCK_BITS = 1664 is the slot a worst case is sized with).  Bits go MSB first.
 * 8. file.  SOI, APP0 JFIF 1.01 (no units, 1:1, no thumbnail), DQT luma, DQT chroma, SOF0, DHT DC luma, AC luma, DC chroma, AC chroma, SOS
 *    (rsrt_jpeg_headers: RSRT_JPEG_HEADER_BYTES), the scan padded with 1-bits to a byte with 0x00 after every 0xFF (rsrt_jpeg_stuff), EOI.
 */
#ifndef RSRT_JPEG_H
#define RSRT_JPEG_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rsrt.h" /* rsrt_jpeg_params, RSRT_JPEG_* */
#include "rsrt_jpeg_table.h"
#include "rsrt_video.h"

#define RSRT_JPEG_DEFAULT_QUALITY 90u /* rsrt_jpeg_params defaults */
#define RSRT_JPEG_DEFAULT_SUBSAMPLING RSRT_JPEG_420
#define RSRT_JPEG_DEFAULT_FLAGS 0u
#define RSRT_JPEG_DEFAULT_RESERVED 0u
#define RSRT_JPEG_BLOCK_BITS 1664u  /* a block's slot: its code is at most 20 + 63 * 26 = 1658 bits */
#define RSRT_JPEG_HEADER_BYTES 623u /* SOI .. SOS */
#define RSRT_JPEG_MAX_SIDE 65535u   /* SOF0 holds a side in 16 bits */

RSRT_HD int rsrt_jpeg_params_ok(const rsrt_jpeg_params *p)
{
    return p->quality >= 1u && p->quality <= 100u && (p->subsampling == RSRT_JPEG_420 || p->subsampling == RSRT_JPEG_444) && p->flags == 0u && p->reserved == 0u;
}

/* step 6: the picture in MCUs and blocks */
RSRT_HD uint32_t rsrt_jpeg_mcu_side(uint32_t subsampling) { return subsampling == RSRT_JPEG_444 ? 8u : 16u; }
RSRT_HD uint32_t rsrt_jpeg_mcu_blocks(uint32_t subsampling) { return subsampling == RSRT_JPEG_444 ? 3u : 6u; }
RSRT_HD uint32_t rsrt_jpeg_mcus(uint32_t side, uint32_t subsampling) { return side / rsrt_jpeg_mcu_side(subsampling) + (side % rsrt_jpeg_mcu_side(subsampling) ? 1u : 0u); }
RSRT_HD uint64_t rsrt_jpeg_blocks(uint32_t width, uint32_t height, uint32_t subsampling)
{
    return (uint64_t)rsrt_jpeg_mcus(width, subsampling) * rsrt_jpeg_mcus(height, subsampling) * rsrt_jpeg_mcu_blocks(subsampling);
}
/* block i's component: 0 Y, 1 Cb, 2 Cr */
RSRT_HD uint32_t rsrt_jpeg_block_component(uint64_t i, uint32_t subsampling)
{
    if (subsampling == RSRT_JPEG_444) return (uint32_t)(i % 3u);
    const uint32_t k = (uint32_t)(i % 6u);
    return k < 4u ? 0u : k - 3u;
}
/* the block whose DC predicts block i's, -1: none (the predictor is 0) */
RSRT_HD int64_t rsrt_jpeg_block_pred(uint64_t i, uint32_t subsampling)
{
    if (subsampling == RSRT_JPEG_444) return i >= 3u ? (int64_t)i - 3 : -1;
    const uint32_t k = (uint32_t)(i % 6u);
    if (k >= 1u && k <= 3u) return (int64_t)i - 1;
    if (i < 6u) return -1;
    return k == 0u ? (int64_t)i - 3 : (int64_t)i - 6; /* Y00: the MCU before's Y11 */
}

/* steps 1 and 2: the display colour of a pixel -> sY, sCb, sCr */
RSRT_HD void rsrt_jpeg_ycc(const float e[3], float ycc[3])
{
    const float y = (0.299f * e[0] + 0.587f * e[1]) + 0.114f * e[2];
    ycc[0] = y;
    ycc[1] = (e[2] - y) / 1.772f;
    ycc[2] = (e[0] - y) / 1.402f;
}
RSRT_HD void rsrt_jpeg_samples(const float sdr[3], float s[3])
{
    float e[3], ycc[3];
    rsrt_video_signal(RSRT_VIDEO_BT709, sdr, e);
    rsrt_jpeg_ycc(e, ycc);
    s[0] = 255.0f * ycc[0] - 128.0f;
    s[1] = 255.0f * ycc[1];
    s[2] = 255.0f * ycc[2];
}

/* step 4 */
RSRT_HD float rsrt_jpeg_dot(const float *d, const float *a, int stride)
{
    float acc = d[0] * a[0];
    for (int k = 1; k < 8; k++) acc = acc + d[k] * a[k * stride];
    return acc;
}
/* s, c: [y * 8 + x], [v * 8 + u] */
RSRT_HD void rsrt_jpeg_fdct(const float s[64], float c[64])
{
    float t[64];
    for (int y = 0; y < 8; y++)
        for (int u = 0; u < 8; u++) t[y * 8 + u] = rsrt_jpeg_dot(RSRT_JPEG_DCT + 8 * u, s + 8 * y, 1);
    for (int v = 0; v < 8; v++)
        for (int u = 0; u < 8; u++) c[v * 8 + u] = rsrt_jpeg_dot(RSRT_JPEG_DCT + 8 * v, t + u, 8);
}

/* step 5 */
RSRT_HD uint32_t rsrt_jpeg_q(uint32_t base, uint32_t quality)
{
    const uint32_t s = quality < 50u ? 5000u / quality : 200u - 2u * quality, q = (base * s + 50u) / 100u;
    return q < 1u ? 1u : (q > 255u ? 255u : q);
}
/* natural index n = v * 8 + u of a luma (chroma 0) or chroma (1) block */
RSRT_HD uint32_t rsrt_jpeg_q_at(uint32_t n, uint32_t chroma, uint32_t quality) { return rsrt_jpeg_q(RSRT_JPEG_BASE_Q[chroma][n], quality); }
RSRT_HD int rsrt_jpeg_quantise(float c, uint32_t q, int dc)
{
    float r = floorf(fabsf(c) / (float)q + 0.5f);
    if (c < 0.0f) r = -r;
    const float lo = dc ? -1024.0f : -1023.0f;
    r = r < lo ? lo : (r > 1023.0f ? 1023.0f : r);
    return (int)r;
}
RSRT_HD void rsrt_jpeg_quantise_block(const float c[64], uint32_t chroma, uint32_t quality, int16_t zz[64])
{
    for (int k = 0; k < 64; k++) {
        const uint32_t n = RSRT_JPEG_ZIGZAG[k];
        zz[k] = (int16_t)rsrt_jpeg_quantise(c[n], rsrt_jpeg_q_at(n, chroma, quality), n == 0u);
    }
}
/* whether a coefficient is one the baseline tables can code */
RSRT_HD int rsrt_jpeg_value_ok(int v, int dc) { return v >= (dc ? -1024 : -1023) && v <= 1023; }

/* step 7.  A code: `*bits` holds its bits in the low end, the first bit the highest; the result is their count */
RSRT_HD uint32_t rsrt_jpeg_size(int v)
{
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
#if defined(__HIP_DEVICE_COMPILE__)
    return 32u - (uint32_t)__clz((int)a);
#else
    uint32_t n = 0u;
    for (; a; a >>= 1) n++;
    return n;
#endif
}
RSRT_HD uint64_t rsrt_jpeg_value_bits(int v, uint32_t size) { return (uint64_t)((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u)); }
/* the DC difference, -2047 .. 2047: at most 9 + 11 bits */
RSRT_HD uint32_t rsrt_jpeg_dc_code(int diff, uint32_t chroma, uint64_t *bits)
{
    const uint32_t size = rsrt_jpeg_size(diff), e = RSRT_JPEG_DC_CODE[chroma][size];
    *bits = (uint64_t)(e & 0xffffu) << size | rsrt_jpeg_value_bits(diff, size);
    return (e >> 16) + size;
}
/* a non-zero AC v after `run` zeros, run 0 .. 62: the ZRLs, the symbol, the value: at most 3 * 11 + 16 + 10 = 59 bits */
RSRT_HD uint32_t rsrt_jpeg_ac_code(uint32_t run, int v, uint32_t chroma, uint64_t *bits)
{
    const uint32_t zrl = RSRT_JPEG_AC_CODE[chroma][0xf0], size = rsrt_jpeg_size(v), e = RSRT_JPEG_AC_CODE[chroma][(run & 15u) << 4 | size];
    uint64_t acc = 0u;
    uint32_t len = 0u;
    for (uint32_t k = 0; k < run >> 4; k++) {
        acc = acc << (zrl >> 16) | (zrl & 0xffffu);
        len += zrl >> 16;
    }
    *bits = (acc << (e >> 16) | (e & 0xffffu)) << size | rsrt_jpeg_value_bits(v, size);
    return len + (e >> 16) + size;
}
RSRT_HD uint32_t rsrt_jpeg_eob_code(uint32_t chroma, uint64_t *bits)
{
    *bits = RSRT_JPEG_AC_CODE[chroma][0] & 0xffffu;
    return RSRT_JPEG_AC_CODE[chroma][0] >> 16;
}

/* a bit writer over a zeroed buffer, MSB first */
typedef struct rsrt_jpeg_writer {
    uint8_t *p;
    uint64_t n_bits;
} rsrt_jpeg_writer;
RSRT_HD void rsrt_jpeg_put(rsrt_jpeg_writer *w, uint64_t bits, uint32_t len)
{
    for (uint32_t k = len; k-- > 0u; w->n_bits++)
        if (bits >> k & 1u) w->p[w->n_bits >> 3] |= (uint8_t)(0x80u >> (w->n_bits & 7u));
}
/* a block's code: its bit count, and (w != NULL) its bits appended.  zz: step 5's; pred: the predictor's DC */
RSRT_HD uint32_t rsrt_jpeg_block_code(rsrt_jpeg_writer *w, const int16_t zz[64], int pred, uint32_t chroma)
{
    uint64_t bits;
    uint32_t len = rsrt_jpeg_dc_code((int)zz[0] - pred, chroma, &bits), total = len, run = 0u;
    if (w) rsrt_jpeg_put(w, bits, len);
    for (int k = 1; k < 64; k++) {
        if (zz[k] == 0) {
            run++;
            continue;
        }
        total += len = rsrt_jpeg_ac_code(run, zz[k], chroma, &bits);
        if (w) rsrt_jpeg_put(w, bits, len);
        run = 0u;
    }
    if (zz[63] == 0) {
        total += len = rsrt_jpeg_eob_code(chroma, &bits);
        if (w) rsrt_jpeg_put(w, bits, len);
    }
    return total;
}
RSRT_HD uint32_t rsrt_jpeg_block_bits(const int16_t zz[64], int pred, uint32_t chroma) { return rsrt_jpeg_block_code(NULL, zz, pred, chroma); }

static const uint8_t RSRT_JPEG_APP0[20] = {0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00}; /* with SOI */
static const uint8_t RSRT_JPEG_SOS[14] = {0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00};
/* step 8.  Everything up to and with SOS into out (RSRT_JPEG_HEADER_BYTES); the count */
RSRT_HD size_t rsrt_jpeg_headers(uint8_t *out, uint32_t width, uint32_t height, const rsrt_jpeg_params *p)
{
    size_t n = 0;
    for (size_t i = 0; i < sizeof RSRT_JPEG_APP0; i++) out[n++] = RSRT_JPEG_APP0[i];
    for (uint32_t t = 0; t < 2u; t++) {
        out[n++] = 0xff; out[n++] = 0xdb; out[n++] = 0x00; out[n++] = 0x43; out[n++] = (uint8_t)t;
        for (int k = 0; k < 64; k++) out[n++] = (uint8_t)rsrt_jpeg_q_at(RSRT_JPEG_ZIGZAG[k], t, p->quality);
    }
    out[n++] = 0xff; out[n++] = 0xc0; out[n++] = 0x00; out[n++] = 0x11; out[n++] = 0x08;
    out[n++] = (uint8_t)(height >> 8); out[n++] = (uint8_t)height; out[n++] = (uint8_t)(width >> 8); out[n++] = (uint8_t)width;
    out[n++] = 0x03;
    out[n++] = 0x01; out[n++] = p->subsampling == RSRT_JPEG_444 ? 0x11 : 0x22; out[n++] = 0x00;
    out[n++] = 0x02; out[n++] = 0x11; out[n++] = 0x01;
    out[n++] = 0x03; out[n++] = 0x11; out[n++] = 0x01;
    for (uint32_t t = 0; t < 4u; t++) { /* DC luma, AC luma, DC chroma, AC chroma */
        const uint32_t ac = t & 1u, chroma = t >> 1, count = ac ? 162u : 12u;
        const uint8_t *const bits = ac ? RSRT_JPEG_AC_BITS[chroma] : RSRT_JPEG_DC_BITS[chroma], *const vals = ac ? RSRT_JPEG_AC_VALS[chroma] : RSRT_JPEG_DC_VALS[chroma];
        out[n++] = 0xff; out[n++] = 0xc4; out[n++] = 0x00; out[n++] = (uint8_t)(19u + count); out[n++] = (uint8_t)(ac << 4 | chroma);
        for (uint32_t k = 0; k < 16u; k++) out[n++] = bits[k];
        for (uint32_t k = 0; k < count; k++) out[n++] = vals[k];
    }
    for (size_t i = 0; i < sizeof RSRT_JPEG_SOS; i++) out[n++] = RSRT_JPEG_SOS[i];
    return n;
}
/* An unstuffed scan of n_bits bits (what is left of its last byte is 0) -> padded with 1-bits, 0x00 after every 0xFF.  out NULL: counts
 * only.  The byte count written */
RSRT_HD size_t rsrt_jpeg_stuff(const uint8_t *scan, uint64_t n_bits, uint8_t *out)
{
    const uint64_t n = (n_bits + 7u) / 8u;
    size_t at = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint8_t b = scan[i];
        if (i == n - 1u && (n_bits & 7u)) b |= (uint8_t)(0xffu >> (n_bits & 7u));
        if (out) out[at] = b;
        at++;
        if (b == 0xffu) {
            if (out) out[at] = 0x00;
            at++;
        }
    }
    return at;
}
/* headers, scan, EOI around an unstuffed scan: the file's size, written when it fits `capacity` (out may be NULL with capacity 0) */
RSRT_HD size_t rsrt_jpeg_file(const uint8_t *scan, uint64_t n_bits, uint32_t width, uint32_t height, const rsrt_jpeg_params *p, uint8_t *out, size_t capacity)
{
    const size_t need = RSRT_JPEG_HEADER_BYTES + rsrt_jpeg_stuff(scan, n_bits, NULL) + 2u;
    if (!out || capacity < need) return need;
    size_t n = rsrt_jpeg_headers(out, width, height, p);
    n += rsrt_jpeg_stuff(scan, n_bits, out + n);
    out[n++] = 0xff; out[n++] = 0xd9;
    return need;
}
/* whether this library codes a width x height picture: sides of 1 .. 65535 and a worst case, RSRT_JPEG_BLOCK_BITS a block, below 2^32
 * bits (bit offsets are uint32): 2 581 110 blocks, 27.5 megapixels at 4:2:0 and 55 at 4:4:4.  The device and the host refuse the rest alike */
RSRT_HD int rsrt_jpeg_size_ok(uint32_t width, uint32_t height, uint32_t subsampling)
{
    return width >= 1u && height >= 1u && width <= RSRT_JPEG_MAX_SIDE && height <= RSRT_JPEG_MAX_SIDE &&
           rsrt_jpeg_blocks(width, height, subsampling) * RSRT_JPEG_BLOCK_BITS < ((uint64_t)1 << 32);
}
/* the worst case of a width x height file: headers + 2 * 208 bytes a block (every byte stuffed) + EOI; 0 for a side of 0 or above 65535 */
RSRT_HD size_t rsrt_jpeg_max_bytes(uint32_t width, uint32_t height, uint32_t subsampling)
{
    if (width == 0u || height == 0u || width > RSRT_JPEG_MAX_SIDE || height > RSRT_JPEG_MAX_SIDE) return 0u;
    return (size_t)(RSRT_JPEG_HEADER_BYTES + 2u * (RSRT_JPEG_BLOCK_BITS / 8u) * rsrt_jpeg_blocks(width, height, subsampling) + 2u);
}

#endif
