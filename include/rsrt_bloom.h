/*
 * rsrt_bloom.h — arithmetic of the bloom pass and the bloomed display (rsrt_bloom, rsrt_bloom_download,
 * rsrt_display_bloomed_srgb8; include/rsrt.h "bloom"), as shared inline code.
 *
 * The pass is the thresholded mip-pyramid bloom of Jimenez, "Next Generation Post Processing in Call of Duty: Advanced Warfare"
 * (SIGGRAPH 2014): a 13-tap (36-texel) downsample per level, a 3x3 tent and a bilinear doubling on the way up, with the firefly
 * weighting of Karis 2013 on the first downsample (the dual-filter idea goes back to Kawase 2003).  Like rsrt_exposure.h this is part
 * of the published numeric contract: plain f32 + * / (-ffp-contract=off, nothing fused) in exactly the order written here, so a
 * numpy restatement reproduces every bit (tests/bloom_ref.py holds it).
 *
 * Images are rgb; a stored texel is four floats, the fourth 0.  All addressing clamps to the edge: cl(i, n) = min(max(i, 0), n - 1).
 *   lum(p) = (0.2126f * p.r + 0.7152f * p.g) + 0.0722f * p.b
 *
 * Prefilter of a pixel of sums (the accumulator: total = (float)sample_total; every other source: total = 1):
 *   c = sum.rgb / total                 one f32 division a channel
 *   p = c * exposure
 *   p = !(p >= 0) ? 0 : p               per channel: negatives and NaN
 *   p = p > 65504 ? 65504 : p           per channel (RSRT_BLOOM_CLAMP): an overflowed mean spreads no inf or NaN
 *   L = lum(p);  s = L > threshold ? (L - threshold) / L : 0;  q = p * s        (threshold 0: s = 1 exactly wherever L > 0)
 *
 * Downsample, D_k (ceil(w / 2) x ceil(h / 2)) from D_{k-1} (w x h); D_0 is the prefiltered source.  At output (x, y):
 *   box(a, b, c, d) = ((a + b) + (c + d)) * 0.25f
 *   tap(ox, oy) = box(s(x0, y0), s(x1, y0), s(x0, y1), s(x1, y1)),  x0 = cl(2x + ox, w), x1 = cl(2x + ox + 1, w), y likewise
 *   grp(ox, oy) = box(tap(ox, oy), tap(ox + 2, oy), tap(ox, oy + 2), tap(ox + 2, oy + 2))
 *   gc = grp(-1, -1);  g0 = grp(-2, -2), g1 = grp(0, -2), g2 = grp(-2, 0), g3 = grp(0, 0)
 *   plain:  D = gc * 0.5f + ((g0 + g1) + (g2 + g3)) * 0.125f
 *   Karis (k == 1 only, under RSRT_BLOOM_KARIS):  kw(g) = 1.0f / (1.0f + lum(g)),  wc = kw(gc) * 0.5f,  wi = kw(gi) * 0.125f,
 *           num = gc * wc + ((g0 * w0 + g1 * w1) + (g2 * w2 + g3 * w3)),  den = wc + ((w0 + w1) + (w2 + w3)),  D = num / den
 *
 * Tent, same size in and out, c(dx, dy) = U(cl(x + dx, w), cl(y + dy, h)):
 *   T = (((c(-1,-1) + c(1,-1)) + (c(-1,1) + c(1,1))) * 0.0625f + ((c(0,-1) + c(0,1)) + (c(-1,0) + c(1,0))) * 0.125f) + c(0,0) * 0.25f
 *
 * Upsample x2 of a coarse image t (w x h) at the fine pixel (x, y):
 *   x0 = (x + 1) / 2 - 1 (signed), wx0 = x odd ? 0.75f : 0.25f, wx1 = 1.0f - wx0; y likewise
 *   up = (t(cl(x0), cl(y0)) * wx0 + t(cl(x0 + 1), cl(y0)) * wx1) * wy0 + (t(cl(x0), cl(y0 + 1)) * wx0 + t(cl(x0 + 1), cl(y0 + 1)) * wx1) * wy1
 *
 * Chain of N levels:  U_N = D_N;  U_k = D_k + up(tent(U_{k+1})), k = N - 1 .. 1;  the bloom image B = tent(U_1) * (1.0f / (float)N),
 * of D_1's size.
 *
 * Bloomed display pixel: hdr = rsrt_display_hdr_exposed (rsrt_exposure.h), hdr = hdr + intensity * up(B) (rsrt_display_hdr_bloomed), then
 * rsrt_aces_tone_map and rsrt_display_encode.
 */
#ifndef RSRT_BLOOM_H
#define RSRT_BLOOM_H

#include <stdint.h>

#include "rsrt.h" /* rsrt_bloom_params, RSRT_BLOOM_KARIS */
#include "rsrt_exposure.h" /* rsrt_display_hdr_exposed */

#define RSRT_BLOOM_MAX_LEVELS 8u
#define RSRT_BLOOM_CLAMP 65504.0f
#define RSRT_BLOOM_LEVELS 6u        /* rsrt_bloom_params defaults */
#define RSRT_BLOOM_THRESHOLD 1.0f   /* in exposed units: what is brighter than display white blooms */
#define RSRT_BLOOM_FLAGS RSRT_BLOOM_KARIS
#define RSRT_BLOOM_INTENSITY 0.1f   /* rsrt_display_bloomed_srgb8's default */

typedef struct rsrt_bloom_rgb { float r, g, b; } rsrt_bloom_rgb;
/* a stored texel: rgb and a word that is 0 */
typedef struct __attribute__((aligned(16))) rsrt_bloom_texel { float r, g, b, a; } rsrt_bloom_texel;

RSRT_HD rsrt_bloom_rgb rsrt_bloom_make(float r, float g, float b)
{
    rsrt_bloom_rgb v;
    v.r = r; v.g = g; v.b = b;
    return v;
}
RSRT_HD rsrt_bloom_rgb rsrt_bloom_add(rsrt_bloom_rgb a, rsrt_bloom_rgb b) { return rsrt_bloom_make(a.r + b.r, a.g + b.g, a.b + b.b); }
RSRT_HD rsrt_bloom_rgb rsrt_bloom_mul(rsrt_bloom_rgb a, float s) { return rsrt_bloom_make(a.r * s, a.g * s, a.b * s); }
RSRT_HD float rsrt_bloom_lum(rsrt_bloom_rgb p) { return (0.2126f * p.r + 0.7152f * p.g) + 0.0722f * p.b; }
RSRT_HD rsrt_bloom_rgb rsrt_bloom_load(const rsrt_bloom_texel *img, size_t i)
{
    const rsrt_bloom_texel t = img[i];
    return rsrt_bloom_make(t.r, t.g, t.b);
}
RSRT_HD void rsrt_bloom_store(rsrt_bloom_texel *img, size_t i, rsrt_bloom_rgb v)
{
    rsrt_bloom_texel t;
    t.r = v.r; t.g = v.g; t.b = v.b; t.a = 0.0f;
    img[i] = t;
}
RSRT_HD int rsrt_bloom_cl(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

/* the size of level k (0: the source) along an axis of n source texels */
RSRT_HD uint32_t rsrt_bloom_level_size(uint32_t n, uint32_t k)
{
    for (uint32_t i = 0; i < k; i++) n = (n + 1u) / 2u;
    return n;
}

RSRT_HD int rsrt_bloom_finite_nonneg(float x) { return x >= 0.0f && x < __builtin_inff(); }

RSRT_HD int rsrt_bloom_params_ok(const rsrt_bloom_params *p)
{
    return p->levels >= 1u && p->levels <= RSRT_BLOOM_MAX_LEVELS && (p->flags & ~(uint32_t)RSRT_BLOOM_KARIS) == 0u &&
           rsrt_bloom_finite_nonneg(p->threshold);
}

RSRT_HD float rsrt_bloom_prefilter_channel(float sum, float total, float exposure)
{
    const float p = (sum / total) * exposure;
    if (!(p >= 0.0f)) return 0.0f;
    return p > RSRT_BLOOM_CLAMP ? RSRT_BLOOM_CLAMP : p;
}

/* D_0 at a pixel of sums */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_prefilter(rsrt_bloom_rgb sum, float total, float exposure, float threshold)
{
    const rsrt_bloom_rgb p = rsrt_bloom_make(rsrt_bloom_prefilter_channel(sum.r, total, exposure), rsrt_bloom_prefilter_channel(sum.g, total, exposure),
                                             rsrt_bloom_prefilter_channel(sum.b, total, exposure));
    const float L = rsrt_bloom_lum(p);
    const float s = L > threshold ? (L - threshold) / L : 0.0f;
    return rsrt_bloom_mul(p, s);
}

/* a 2x2 tap of four texels, and a group of four taps */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_box(rsrt_bloom_rgb a, rsrt_bloom_rgb b, rsrt_bloom_rgb c, rsrt_bloom_rgb d)
{
    return rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_add(a, b), rsrt_bloom_add(c, d)), 0.25f);
}

RSRT_HD rsrt_bloom_rgb rsrt_bloom_down_plain(rsrt_bloom_rgb gc, rsrt_bloom_rgb g0, rsrt_bloom_rgb g1, rsrt_bloom_rgb g2, rsrt_bloom_rgb g3)
{
    return rsrt_bloom_add(rsrt_bloom_mul(gc, 0.5f), rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_add(g0, g1), rsrt_bloom_add(g2, g3)), 0.125f));
}

RSRT_HD float rsrt_bloom_karis_weight(rsrt_bloom_rgb g) { return 1.0f / (1.0f + rsrt_bloom_lum(g)); }

RSRT_HD rsrt_bloom_rgb rsrt_bloom_down_karis(rsrt_bloom_rgb gc, rsrt_bloom_rgb g0, rsrt_bloom_rgb g1, rsrt_bloom_rgb g2, rsrt_bloom_rgb g3)
{
    const float wc = rsrt_bloom_karis_weight(gc) * 0.5f;
    const float w0 = rsrt_bloom_karis_weight(g0) * 0.125f, w1 = rsrt_bloom_karis_weight(g1) * 0.125f;
    const float w2 = rsrt_bloom_karis_weight(g2) * 0.125f, w3 = rsrt_bloom_karis_weight(g3) * 0.125f;
    const rsrt_bloom_rgb num = rsrt_bloom_add(rsrt_bloom_mul(gc, wc), rsrt_bloom_add(rsrt_bloom_add(rsrt_bloom_mul(g0, w0), rsrt_bloom_mul(g1, w1)),
                                                                                     rsrt_bloom_add(rsrt_bloom_mul(g2, w2), rsrt_bloom_mul(g3, w3))));
    const float den = wc + ((w0 + w1) + (w2 + w3));
    return rsrt_bloom_make(num.r / den, num.g / den, num.b / den);
}

RSRT_HD rsrt_bloom_rgb rsrt_bloom_down(rsrt_bloom_rgb gc, rsrt_bloom_rgb g0, rsrt_bloom_rgb g1, rsrt_bloom_rgb g2, rsrt_bloom_rgb g3, int karis)
{
    return karis ? rsrt_bloom_down_karis(gc, g0, g1, g2, g3) : rsrt_bloom_down_plain(gc, g0, g1, g2, g3);
}

/* the tent of nine texels: corners (-1,-1) (1,-1) (-1,1) (1,1), edges (0,-1) (0,1) (-1,0) (1,0), centre */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_tent9(rsrt_bloom_rgb cmm, rsrt_bloom_rgb cpm, rsrt_bloom_rgb cmp, rsrt_bloom_rgb cpp, rsrt_bloom_rgb c0m,
                                        rsrt_bloom_rgb c0p, rsrt_bloom_rgb cm0, rsrt_bloom_rgb cp0, rsrt_bloom_rgb c00)
{
    const rsrt_bloom_rgb corners = rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_add(cmm, cpm), rsrt_bloom_add(cmp, cpp)), 0.0625f);
    const rsrt_bloom_rgb edges = rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_add(c0m, c0p), rsrt_bloom_add(cm0, cp0)), 0.125f);
    return rsrt_bloom_add(rsrt_bloom_add(corners, edges), rsrt_bloom_mul(c00, 0.25f));
}

/* ... of three rows of three texels */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_tent_rows(const rsrt_bloom_rgb top[3], const rsrt_bloom_rgb mid[3], const rsrt_bloom_rgb bottom[3])
{
    return rsrt_bloom_tent9(top[0], top[2], bottom[0], bottom[2], top[1], bottom[1], mid[0], mid[2], mid[1]);
}

/* the coarse coordinate (before the clamp) and the two weights of a fine coordinate */
RSRT_HD void rsrt_bloom_up_coord(int x, int *x0, float *w0, float *w1)
{
    *x0 = (x + 1) / 2 - 1;
    *w0 = (x & 1) ? 0.75f : 0.25f;
    *w1 = 1.0f - *w0;
}

RSRT_HD rsrt_bloom_rgb rsrt_bloom_up4(rsrt_bloom_rgb t00, rsrt_bloom_rgb t10, rsrt_bloom_rgb t01, rsrt_bloom_rgb t11, float wx0, float wx1,
                                      float wy0, float wy1)
{
    const rsrt_bloom_rgb top = rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_mul(t00, wx0), rsrt_bloom_mul(t10, wx1)), wy0);
    const rsrt_bloom_rgb bottom = rsrt_bloom_mul(rsrt_bloom_add(rsrt_bloom_mul(t01, wx0), rsrt_bloom_mul(t11, wx1)), wy1);
    return rsrt_bloom_add(top, bottom);
}

/* -- the same over stored images (w x h texels, rows of w), clamped ---------------------------------------------------------- */

RSRT_HD rsrt_bloom_rgb rsrt_bloom_at(const rsrt_bloom_texel *img, int w, int h, int x, int y)
{
    return rsrt_bloom_load(img, (size_t)rsrt_bloom_cl(y, h) * (size_t)w + (size_t)rsrt_bloom_cl(x, w));
}

/* tap(ox, oy) of output (x, y): the texels 2x + ox, 2x + ox + 1 of the rows 2y + oy, 2y + oy + 1 */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_tap_at(const rsrt_bloom_texel *src, int w, int h, int x, int y, int ox, int oy)
{
    const int sx = 2 * x + ox, sy = 2 * y + oy;
    return rsrt_bloom_box(rsrt_bloom_at(src, w, h, sx, sy), rsrt_bloom_at(src, w, h, sx + 1, sy), rsrt_bloom_at(src, w, h, sx, sy + 1),
                          rsrt_bloom_at(src, w, h, sx + 1, sy + 1));
}

RSRT_HD rsrt_bloom_rgb rsrt_bloom_grp_at(const rsrt_bloom_texel *src, int w, int h, int x, int y, int ox, int oy)
{
    return rsrt_bloom_box(rsrt_bloom_tap_at(src, w, h, x, y, ox, oy), rsrt_bloom_tap_at(src, w, h, x, y, ox + 2, oy),
                          rsrt_bloom_tap_at(src, w, h, x, y, ox, oy + 2), rsrt_bloom_tap_at(src, w, h, x, y, ox + 2, oy + 2));
}

/* D_k(x, y) from D_{k-1} (w x h) */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_down_at(const rsrt_bloom_texel *src, int w, int h, int x, int y, int karis)
{
    return rsrt_bloom_down(rsrt_bloom_grp_at(src, w, h, x, y, -1, -1), rsrt_bloom_grp_at(src, w, h, x, y, -2, -2), rsrt_bloom_grp_at(src, w, h, x, y, 0, -2),
                           rsrt_bloom_grp_at(src, w, h, x, y, -2, 0), rsrt_bloom_grp_at(src, w, h, x, y, 0, 0), karis);
}

RSRT_HD rsrt_bloom_rgb rsrt_bloom_tent_at(const rsrt_bloom_texel *u, int w, int h, int x, int y)
{
    return rsrt_bloom_tent9(rsrt_bloom_at(u, w, h, x - 1, y - 1), rsrt_bloom_at(u, w, h, x + 1, y - 1), rsrt_bloom_at(u, w, h, x - 1, y + 1),
                            rsrt_bloom_at(u, w, h, x + 1, y + 1), rsrt_bloom_at(u, w, h, x, y - 1), rsrt_bloom_at(u, w, h, x, y + 1),
                            rsrt_bloom_at(u, w, h, x - 1, y), rsrt_bloom_at(u, w, h, x + 1, y), rsrt_bloom_at(u, w, h, x, y));
}

/* up(t)(x, y) of a stored coarse image t (w x h) */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_up_at(const rsrt_bloom_texel *t, int w, int h, int x, int y)
{
    int x0, y0;
    float wx0, wx1, wy0, wy1;
    rsrt_bloom_up_coord(x, &x0, &wx0, &wx1);
    rsrt_bloom_up_coord(y, &y0, &wy0, &wy1);
    return rsrt_bloom_up4(rsrt_bloom_at(t, w, h, x0, y0), rsrt_bloom_at(t, w, h, x0 + 1, y0), rsrt_bloom_at(t, w, h, x0, y0 + 1),
                          rsrt_bloom_at(t, w, h, x0 + 1, y0 + 1), wx0, wx1, wy0, wy1);
}

/* up(tent(u))(x, y) of a stored coarse image u (w x h): the step from U_{k+1} towards U_k without the tent in memory */
RSRT_HD rsrt_bloom_rgb rsrt_bloom_up_tent_at(const rsrt_bloom_texel *u, int w, int h, int x, int y)
{
    int x0, y0;
    float wx0, wx1, wy0, wy1;
    rsrt_bloom_up_coord(x, &x0, &wx0, &wx1);
    rsrt_bloom_up_coord(y, &y0, &wy0, &wy1);
    /* The four tents are centred on the columns xa = cl(x0), xb = cl(x0 + 1) and the rows ya, yb.  0 <= x0 + 1 and x0 <= w - 1 for every
     * fine x < 2w, so either xb = xa + 1 — the tents share two columns — or xa = xb at an edge, where cl(xa - 1) and cl(xa + 1) are
     * the outer columns of both.  Sixteen texels serve all four: the columns cl(xa - 1), xa, xb, cl(xb + 1) and the rows likewise. */
    const int xa = rsrt_bloom_cl(x0, w), xb = rsrt_bloom_cl(x0 + 1, w), ya = rsrt_bloom_cl(y0, h), yb = rsrt_bloom_cl(y0 + 1, h);
    const int cx[4] = {rsrt_bloom_cl(xa - 1, w), xa, xb, rsrt_bloom_cl(xb + 1, w)}, cy[4] = {rsrt_bloom_cl(ya - 1, h), ya, yb, rsrt_bloom_cl(yb + 1, h)};
    rsrt_bloom_rgb t[4][4];
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++) t[j][i] = rsrt_bloom_load(u, (size_t)cy[j] * (size_t)w + (size_t)cx[i]);
    /* per row, the three columns of the tent centred on xa (a) and on xb (b); then the three rows of the tents centred on ya and yb */
    const int ex = xa == xb, ey = ya == yb;
    rsrt_bloom_rgb a[4][3], b[4][3];
    for (int j = 0; j < 4; j++) {
        a[j][0] = t[j][0]; a[j][1] = t[j][1]; a[j][2] = ex ? t[j][3] : t[j][2];
        b[j][0] = ex ? t[j][0] : t[j][1]; b[j][1] = t[j][2]; b[j][2] = t[j][3];
    }
    rsrt_bloom_rgb a2[3], b2[3], a0[3], b0[3]; /* the bottom row of the tents on ya, the top row of the tents on yb */
    for (int i = 0; i < 3; i++) {
        a2[i] = ey ? a[3][i] : a[2][i]; b2[i] = ey ? b[3][i] : b[2][i];
        a0[i] = ey ? a[0][i] : a[1][i]; b0[i] = ey ? b[0][i] : b[1][i];
    }
    const rsrt_bloom_rgb taa = rsrt_bloom_tent_rows(a[0], a[1], a2), tba = rsrt_bloom_tent_rows(b[0], b[1], b2);
    const rsrt_bloom_rgb tab = rsrt_bloom_tent_rows(a0, a[2], a[3]), tbb = rsrt_bloom_tent_rows(b0, b[2], b[3]);
    return rsrt_bloom_up4(taa, tba, tab, tbb, wx0, wx1, wy0, wy1);
}

/* the display chain's third step: the exposed mean plus intensity times up(B) at the pixel */
RSRT_HD void rsrt_display_hdr_bloomed(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b, float hdr[3])
{
    const float bloom[3] = {up_b.r, up_b.g, up_b.b};
    rsrt_display_hdr_exposed(sum_rgb, total, exposure, hdr);
    for (int i = 0; i < 3; i++) hdr[i] = hdr[i] + intensity * bloom[i];
}

/* one pixel: sums (f32) and up(B) at it -> display bytes at an exposure */
RSRT_HD void rsrt_display_pixel_bloomed(const float sum_rgb[3], float total, float exposure, float intensity, rsrt_bloom_rgb up_b,
                                        unsigned char out_rgb[3])
{
    float hdr[3], sdr[3];
    rsrt_display_hdr_bloomed(sum_rgb, total, exposure, intensity, up_b, hdr);
    rsrt_aces_tone_map(hdr, sdr);
    rsrt_display_encode(sdr, out_rgb);
}

#endif
