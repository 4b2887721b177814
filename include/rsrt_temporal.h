/*
 * rsrt_temporal.h — per-pixel arithmetic of the temporal pass (rsrt_temporal_accumulate, include/rsrt.h), as shared inline code.
 *
 * The pass reprojects the previous frames' per-pixel history into the current camera, rejects it where the surface changed
 * (disocclusion) and blends the rest with the new frame, weighted by sample count.  Like rsrt_denoise.h this is part of the
 * published numeric contract: plain f32 + - * /, rsrt_sqrtf, floorf and rsrt_sinf (-ffp-contract=off), every sum in a fixed
 * order, so that a numpy float32 restatement reproduces the GPU output bit for bit (tests/temporal_ref.py, tests/test_temporal.py).
 * The one exception is the centre ray, which is start_path's camera ray with zero jitter and fuses exactly what start_path fuses
 * (the column-major mat3 product and the dot product of the normalisation).
 *
 * Per pixel p = (x, y) of a W x H frame, with S = sample_total, T = aov_sample_total, the accumulator sum and the AOV record a:
 *   c     = sum.rgb / S
 *   surface when 2 a[3] >= T: n = a[4..6] / a[3], z = a[7] / a[3] (means over the hits), X = o + z d(p); otherwise sky, and only
 *   the direction d(p) is reprojected.  d(p) is the centre ray of p (pixel x aims at fx = x: pixel centres sit at integer
 *   coordinates in start_path's mapping).
 *   Identity: the previous camera equals the current one (pos, the 3x3 of rot_transform and fov_y as bit patterns) and W, H are
 *   unchanged: h = Hc(p), nh = Hn(p), no tests, no cap, so a camera held still converges like the plain accumulator.
 *   Otherwise v = R'^T (X - o') (sky: R'^T d(p)); no history when -v.z <= 0; sx = v.x / ((-v.z) m' aspect), sy = v.y / ((-v.z) m'),
 *   m' = rsrt_sinf(fov'/2), fx = ((sx + 1) 0.5) W, fy = ((1 - sy) 0.5) H; no history unless -1 < fx < W and -1 < fy < H (this
 *   covers non-finite values: outside that range no tap inside the image has a positive weight).  Bilinear taps (x0, y0),
 *   (x0+1, y0), (x0, y0+1), (x0+1, y0+1), x0 = floor(fx), weights (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax ay.  A tap q is valid when
 *   it lies inside the image, Hn(q) > 0, its class (surface or sky) is p's and, for surfaces, |n . (Xq - X)| <= tau_z z (the
 *   plane-distance test; Xq = o' + zq d'(q) from the stored depth and the previous camera's centre ray of q) and n . nq >= tau_n.
 *   wsum = sum of the valid weights; below RSRT_TP_MIN_WEIGHT there is no history; otherwise h = (sum w Hc(q)) / wsum and
 *   nh = min((sum w Hn(q)) / wsum, max_history).
 *   Blend: out.rgb = (h nh + c S) / (nh + S), out.w = nh + S; without history out = (c, S).
 *   Stored for the next frame: out, and the features (n.xyz, z), or (0, 0, 0, -1) for sky.
 *   With RSRT_TEMPORAL_MOMENTS the same taps also carry the luminance moments (rsrt_tp_moments, below).
 *
 * Defaults (what a zero-initialised caller should fill in; the Python and C++ State use them):
 *   max_history 32 samples (in [1, 2^24]), depth_tolerance tau_z 0.05 (in [1e-6, 1e6]), normal_tolerance tau_n 0.9 (in [-1, 1]).
 * The depth tolerance: at 1 spp a pixel's first hit lies up to about one pixel's angular size alpha off its centre ray, so two
 * frames' points of one surface disagree by up to about 2 z alpha along the normal, about 2 % of z at 160 x 90 (alpha = 2 m / H
 * with m = sin(fov/2)); the plane-distance test, unlike a relative-depth test, stays that small at grazing angles, where a whole
 * floor would otherwise be rejected.  0.05 leaves room for that and for the mean of a few samples straddling an edge.
 */
#ifndef RSRT_TEMPORAL_H
#define RSRT_TEMPORAL_H

#include "rsrt_detmath.h"
#include "rsrt_variance.h" /* rsrt_sv_frame_lum: the moments' luminance */

#define RSRT_TP_MIN_WEIGHT 0.01f       /* below this much valid bilinear weight a pixel has no history */
#define RSRT_TP_MAX_HISTORY 32u        /* defaults of rsrt_temporal_params */
#define RSRT_TP_DEPTH_TOLERANCE 0.05f
#define RSRT_TP_NORMAL_TOLERANCE 0.9f

/* what happened to a pixel (the kernel does not store it; the host tests compare it with the restatement's) */
enum {
    RSRT_TP_FIRST = 0,           /* no previous frame */
    RSRT_TP_IDENTITY = 1,        /* unchanged camera: the pixel's own history */
    RSRT_TP_REPROJECTED = 2,     /* surface, history resampled */
    RSRT_TP_SKY = 3,             /* sky, history resampled */
    RSRT_TP_BEHIND = 4,          /* behind the previous camera */
    RSRT_TP_OUT_OF_VIEW = 5,     /* outside the previous frame (or not finite) */
    RSRT_TP_PLANE_REJECTED = 6,  /* too little weight, and a tap failed the plane-distance test */
    RSRT_TP_NORMAL_REJECTED = 7, /* too little weight, and a tap failed the normal test (none the plane test) */
    RSRT_TP_LOW_WEIGHT = 8       /* too little weight otherwise (taps outside, empty or of the other class) */
};

/* a camera as the pass sees it: rot = rot_transform's 3x3, column-major (rot[3 j + k] = rot_transform[j][k]); m = rsrt_sinf(fov_y / 2) */
typedef struct rsrt_tp_camera {
    float pos[3];
    float rot[9];
    float fov_y;
    float m;
} rsrt_tp_camera;

/* what is constant over one frame */
typedef struct rsrt_tp_frame {
    rsrt_tp_camera cur, prev;
    unsigned width, height;
    float sample_total, aov_sample_total;
    float max_history, depth_tolerance, normal_tolerance;
    float aspect;   /* W / H */
    int has_prev;   /* a previous frame exists (since the last reset) */
    int identity;   /* rsrt_tp_same_camera(cur, prev) */
} rsrt_tp_frame;

RSRT_HD void rsrt_tp_camera_init(rsrt_tp_camera *c, const float pos[3], const float rot[9], float fov_y)
{
    for (int i = 0; i < 3; i++) c->pos[i] = pos[i];
    for (int i = 0; i < 9; i++) c->rot[i] = rot[i];
    c->fov_y = fov_y;
    c->m = rsrt_sinf(fov_y / 2.0f);
}

RSRT_HD unsigned rsrt_tp_bits(float x)
{
    union { float f; unsigned u; } v;
    v.f = x;
    return v.u;
}

/* pos, the 3x3 and fov_y compared as bit patterns */
RSRT_HD int rsrt_tp_same_camera(const rsrt_tp_camera *a, const rsrt_tp_camera *b)
{
    int same = rsrt_tp_bits(a->fov_y) == rsrt_tp_bits(b->fov_y);
    for (int i = 0; i < 3; i++) same = same && rsrt_tp_bits(a->pos[i]) == rsrt_tp_bits(b->pos[i]);
    for (int i = 0; i < 9; i++) same = same && rsrt_tp_bits(a->rot[i]) == rsrt_tp_bits(b->rot[i]);
    return same;
}

/* start_path's camera ray of pixel (x, y) with zero jitter: fx = x, fy = y, then exactly its arithmetic (mat3_mul and the dot of
 * normalize fused; the reciprocal of the length is the correctly rounded 1 / sqrt) */
RSRT_HD void rsrt_tp_center_ray(const rsrt_tp_camera *c, unsigned w, unsigned h, float aspect, int x, int y, float d[3])
{
    const float fx = (float)x, fy = (float)y;
    const float sx = ((fx / (float)w) * 2.0f - 1.0f) * 1.0f;
    const float sy = ((fy / (float)h) * 2.0f - 1.0f) * -1.0f;
    const float v0 = sx * c->m * aspect, v1 = sy * c->m, v2 = -1.0f;
    const float *r = c->rot;
    const float a0 = __builtin_fmaf(r[6], v2, __builtin_fmaf(r[3], v1, r[0] * v0));
    const float a1 = __builtin_fmaf(r[7], v2, __builtin_fmaf(r[4], v1, r[1] * v0));
    const float a2 = __builtin_fmaf(r[8], v2, __builtin_fmaf(r[5], v1, r[2] * v0));
    const float inv = 1.0f / rsrt_sqrtf(__builtin_fmaf(a2, a2, __builtin_fmaf(a1, a1, a0 * a0)));
    d[0] = a0 * inv;
    d[1] = a1 * inv;
    d[2] = a2 * inv;
}

RSRT_HD float rsrt_tp_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* e (a point minus o', or a direction) into camera c: sets fx, fy; 0 when it lies behind the camera */
RSRT_HD int rsrt_tp_project(const rsrt_tp_camera *c, unsigned w, unsigned h, float aspect, const float e[3], float *fx, float *fy)
{
    const float vx = rsrt_tp_dot(c->rot, e), vy = rsrt_tp_dot(c->rot + 3, e), vz = rsrt_tp_dot(c->rot + 6, e);
    const float depth = -vz;
    if (!(depth > 0.0f)) return 0;
    const float sx = vx / ((depth * c->m) * aspect), sy = vy / (depth * c->m);
    *fx = ((sx + 1.0f) * 0.5f) * (float)w;
    *fy = ((1.0f - sy) * 0.5f) * (float)h;
    return 1;
}

/* the current frame at one pixel: c (sum / S) and the features (n.xyz, z) or (0, 0, 0, -1); returns 1 for a surface */
RSRT_HD int rsrt_tp_current(const rsrt_tp_frame *fr, const float sum[3], const float aov[8], float c[3], float f[4])
{
    for (int i = 0; i < 3; i++) c[i] = sum[i] / fr->sample_total;
    const int surface = 2.0f * aov[3] >= fr->aov_sample_total;
    for (int i = 0; i < 4; i++) f[i] = surface ? aov[4 + i] / aov[3] : (i == 3 ? -1.0f : 0.0f);
    return surface;
}

/* What rsrt_tp_pixel_m gathers besides the colour: nothing (the plain pass).  A gatherer sees the history exactly where the colour
 * does: own(q) in the identity case, tap(q, w) for every valid bilinear tap, resolve(wsum) when the taps carry enough weight, and
 * finally blend(used, nh, S), with used != 0 when the pixel has history and nh its (capped) weight. */
struct rsrt_tp_no_moments {
    RSRT_HD void own(unsigned) {}
    RSRT_HD void tap(unsigned, float) {}
    RSRT_HD void resolve(float) {}
    RSRT_HD void blend(int, float, float) {}
};

/* One pixel.  Prev::col(q, float[4]) and Prev::feat(q, float[4]) load the previous history and features of pixel index q.  Writes the
 * new history (out) and features (f); returns an RSRT_TP_* code.  mom gathers along (rsrt_tp_no_moments, rsrt_tp_moments). */
template <class Prev, class Mom>
RSRT_HD int rsrt_tp_pixel_m(const rsrt_tp_frame *fr, const Prev &prev, Mom &mom, int x, int y, const float sum[3], const float aov[8], float out[4],
                            float f[4])
{
    const unsigned w = fr->width, hh = fr->height;
    float c[3];
    const int surface = rsrt_tp_current(fr, sum, aov, c, f);
    const float S = fr->sample_total;
    float h[3] = {0.0f, 0.0f, 0.0f}, nh = 0.0f;
    int code;
    if (!fr->has_prev) {
        code = RSRT_TP_FIRST;
    } else if (fr->identity) {
        float hq[4];
        prev.col((unsigned)y * w + (unsigned)x, hq);
        h[0] = hq[0]; h[1] = hq[1]; h[2] = hq[2]; nh = hq[3];
        mom.own((unsigned)y * w + (unsigned)x);
        code = RSRT_TP_IDENTITY;
    } else {
        float d[3], X[3], e[3], fx = 0.0f, fy = 0.0f;
        rsrt_tp_center_ray(&fr->cur, w, hh, fr->aspect, x, y, d);
        for (int i = 0; i < 3; i++) {
            X[i] = fr->cur.pos[i] + f[3] * d[i];
            e[i] = surface ? X[i] - fr->prev.pos[i] : d[i];
        }
        if (!rsrt_tp_project(&fr->prev, w, hh, fr->aspect, e, &fx, &fy)) {
            code = RSRT_TP_BEHIND;
        } else if (!(fx > -1.0f && fx < (float)w && fy > -1.0f && fy < (float)hh)) {
            code = RSRT_TP_OUT_OF_VIEW;
        } else {
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float ax = fx - flx, ay = fy - fly;
            const float tw[4] = {(1.0f - ax) * (1.0f - ay), ax * (1.0f - ay), (1.0f - ax) * ay, ax * ay};
            const float tol = fr->depth_tolerance * f[3];
            float wsum = 0.0f, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            int plane_rej = 0, normal_rej = 0;
            for (int t = 0; t < 4; t++) {
                const int qx = x0 + (t & 1), qy = y0 + (t >> 1);
                if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)hh) continue;
                const unsigned q = (unsigned)qy * w + (unsigned)qx;
                float hq[4], fq[4];
                prev.col(q, hq);
                if (!(hq[3] > 0.0f)) continue;
                prev.feat(q, fq);
                if ((fq[3] >= 0.0f) != (surface != 0)) continue;
                if (surface) {
                    float dq[3], eq[3];
                    rsrt_tp_center_ray(&fr->prev, w, hh, fr->aspect, qx, qy, dq);
                    for (int i = 0; i < 3; i++) eq[i] = (fr->prev.pos[i] + fq[3] * dq[i]) - X[i];
                    const float pd = rsrt_tp_dot(f, eq);
                    if (!((pd < 0.0f ? -pd : pd) <= tol)) { plane_rej = 1; continue; }
                    if (!(rsrt_tp_dot(f, fq) >= fr->normal_tolerance)) { normal_rej = 1; continue; }
                }
                wsum = wsum + tw[t];
                for (int i = 0; i < 4; i++) acc[i] = acc[i] + tw[t] * hq[i];
                mom.tap(q, tw[t]);
            }
            if (wsum < RSRT_TP_MIN_WEIGHT) {
                code = plane_rej ? RSRT_TP_PLANE_REJECTED : (normal_rej ? RSRT_TP_NORMAL_REJECTED : RSRT_TP_LOW_WEIGHT);
            } else {
                for (int i = 0; i < 3; i++) h[i] = acc[i] / wsum;
                nh = acc[3] / wsum;
                nh = nh > fr->max_history ? fr->max_history : nh;
                mom.resolve(wsum);
                code = surface ? RSRT_TP_REPROJECTED : RSRT_TP_SKY;
            }
        }
    }
    if (code == RSRT_TP_IDENTITY || code == RSRT_TP_REPROJECTED || code == RSRT_TP_SKY) {
        for (int i = 0; i < 3; i++) out[i] = (h[i] * nh + c[i] * S) / (nh + S);
        out[3] = nh + S;
        mom.blend(1, nh, S);
    } else {
        for (int i = 0; i < 3; i++) out[i] = c[i];
        out[3] = S;
        mom.blend(0, nh, S);
    }
    return code;
}

/* the plain pass (rt_temporal_kernel) */
template <class Prev>
RSRT_HD int rsrt_tp_pixel(const rsrt_tp_frame *fr, const Prev &prev, int x, int y, const float sum[3], const float aov[8], float out[4], float f[4])
{
    rsrt_tp_no_moments none;
    return rsrt_tp_pixel_m(fr, prev, none, x, y, sum, aov, out, f);
}

/* The luminance moments (RSRT_TEMPORAL_MOMENTS, rt_temporal_moments_kernel): a float4 record (mu1, mu2, frames, scale) per pixel.
 * l = rsrt_sv_lum of the frame's demodulated colour sum / S / max(a, RSRT_DN_ALBEDO_EPS) (rsrt_sv_frame_lum, with the current AOV
 * record's mean albedo a).  mu1, mu2 and frames are reprojected with the colour's taps, weights and wsum (hm = (sum w m(q)) / wsum;
 * identity: the pixel's own record) and blended with the colour's weights:
 *   mu1' = (hm1 nh + l S) / (nh + S),  mu2' = (hm2 nh + (l l) S) / (nh + S),  frames' = hm3 + 1,  scale = S / (nh + S);
 * without history (l, l l, 1, 1).  scale is the factor by which the spread of the per-frame means shrinks in the blended colour:
 * scale (mu2 - mu1^2) estimates the variance of the output's luminance, and it goes to 0 as a still camera converges.
 * Load::mom(q, float[4]) loads the previous record of pixel index q. */
template <class Load>
struct rsrt_tp_moments {
    const Load *load;
    float l;
    float h[3];   /* the reprojected mu1, mu2, frames */
    float out[4]; /* the new record */
    RSRT_HD void own(unsigned q)
    {
        float m[4];
        load->mom(q, m);
        for (int i = 0; i < 3; i++) h[i] = m[i];
    }
    RSRT_HD void tap(unsigned q, float w)
    {
        float m[4];
        load->mom(q, m);
        for (int i = 0; i < 3; i++) h[i] = h[i] + w * m[i];
    }
    RSRT_HD void resolve(float wsum)
    {
        for (int i = 0; i < 3; i++) h[i] = h[i] / wsum;
    }
    RSRT_HD void blend(int used, float nh, float S)
    {
        const float l2 = l * l;
        if (used) {
            out[0] = (h[0] * nh + l * S) / (nh + S);
            out[1] = (h[1] * nh + l2 * S) / (nh + S);
            out[2] = h[2] + 1.0f;
            out[3] = S / (nh + S);
        } else {
            out[0] = l; out[1] = l2; out[2] = 1.0f; out[3] = 1.0f;
        }
    }
};

/* one pixel of a MOMENTS frame: rsrt_tp_pixel's history and features, bit for bit, and the moment record (mout) */
template <class Prev>
RSRT_HD int rsrt_tp_pixel_moments(const rsrt_tp_frame *fr, const Prev &prev, int x, int y, const float sum[3], const float aov[8], float out[4],
                                  float f[4], float mout[4])
{
    rsrt_tp_moments<Prev> mom = {&prev, rsrt_sv_frame_lum(sum, fr->sample_total, aov, fr->aov_sample_total), {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    const int code = rsrt_tp_pixel_m(fr, prev, mom, x, y, sum, aov, out, f);
    for (int i = 0; i < 4; i++) mout[i] = mom.out[i];
    return code;
}

#endif
