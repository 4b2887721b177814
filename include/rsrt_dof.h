/*
 * rsrt_dof.h — arithmetic of the depth-of-field pass (rsrt_dof, rsrt_dof_coc_download, rsrt_dof_depth_at; include/rsrt.h "depth of
 * field"), as shared inline code.
 *
 * The pass is a post-process lens blur: a signed circle of confusion per pixel from the first-hit distance (Potmesil, Chakravarty
 * 1981, for the thin lens behind it) and a disc gather with the scatter-as-gather occlusion rule of the real-time literature
 * (Jimenez 2014).  Like rsrt_bloom.h this is part of the published numeric contract: plain f32 + - * / and compares
 * (-ffp-contract=off, nothing fused, no transcendental) in exactly the order written here, so a numpy restatement reproduces every
 * bit (tests/dof_ref.py holds it).  The one exception is the centre ray, which is rsrt_temporal.h's and fuses what start_path fuses.
 *
 * Per pixel p = (x, y) of a w x h frame, its 8-float first-hit record rec (rec[3] the hit count, rec[7] the sum of hit distances;
 * no sample total is needed), the camera and the parameters (focus_distance, aperture, max_radius):
 *   depth z:   rec[3] > 0:  d = rec[7] / rec[3],  c = dot(centre ray of p, forward axis),  z = d * c
 *              otherwise (sky) the pixel is infinitely far: z = +inf
 *              (the centre ray is rsrt_tp_center_ray's, the dot rsrt_tp_dot's, the forward axis minus the third column of the
 *              camera's rotation.  Focus is on a PLANE, not a sphere: without the cosine a wall that faces the camera at the focus
 *              distance would blur towards the corners.)
 *   radius r:  A = aperture * (float)h  (the blur radius of a point at infinity, a fraction of the picture's height: the look does
 *              not depend on the resolution),  t = focus_distance / z,  r = A * (1.0f - t);  sky: r = A
 *              r = clamp(r, -R, R), R = (float)max_radius;  a NaN r becomes 0;  z = 0 gives -R through the clamp.
 *              Negative r is the near field (in front of the focus plane), positive r the far field.
 *   prepared texel:  (c.rgb, r), c = sum.rgb / total (the accumulator: total = (float)sample_total; every other source: total = 1).
 *              Not rounded to binary16: the display does that to the output.
 *
 * Lens blur of the output pixel p over the prepared texels:
 *   for dy = -max_radius .. max_radius (outer), dx = -max_radius .. max_radius (inner), q = p + (dx, dy); sequential f32 sums in
 *   that order; a tap outside the frame is skipped, not clamped.  For each tap in the frame:
 *     a = |r_q|;  if r_q > r_p (the tap lies behind p): a = min(a, |r_p|);  a = max(a, 0.5f)
 *         — a defocused background does not leak over a sharper foreground, an in-focus pixel behind a near-field blur keeps to
 *         itself, a near-field blur spreads over what is behind it
 *     k = clamp(a + 0.5f - D[dy][dx], 0, 1),  D the correctly rounded f32 sqrt(dx^2 + dy^2), a table (rsrt_dof_table.h)
 *     wgt = k * (0.25f / (a * a))        normalised by the disc's area; exactly 1 for an in-focus pixel on itself
 *     k == 0: the tap is SKIPPED, nothing is added (not added as zero: a non-finite colour times 0 is NaN)
 *     otherwise acc.rgb += wgt * c_q, acc.w += wgt        (acc.rgb starts at -0, acc.w at 0: the first term is added exactly)
 *   out = acc.rgb / acc.w, alpha 1.  (The pixel's own tap has k = 1, so acc.w > 0.)
 * The code below evaluates a and 0.25f / (a * a) in an equal form that needs no division per tap:
 *   max(min(|r_q|, |r_p|), 0.5f) = min(max(|r_q|, 0.5f), max(|r_p|, 0.5f)), so a is one of a_q = max(|r_q|, 0.5f) and a_p, and
 *   0.25f / (a * a) is the same f32 expression of whichever it is: area(a_q), computed once a texel, or area(a_p), once a pixel.
 *
 * Consequences: with aperture 0, or everything at the focus distance, every r is 0, only the pixel's own tap has k > 0 and the
 * output is (1 * c) / 1: the source's colour bit for bit, inf and NaN included.  A non-finite or negative colour spreads over the
 * disc it covers.  With B = ceil(max |r|) over the texels a pixel can reach, a tap more than B pixels away along an axis has
 * D >= B + 1 and a <= max(B, 0.5f), so k == 0: a loop over |dx|, |dy| <= B adds the same numbers in the same order
 * (rt_dof_gather_kernel's workgroup-uniform bound).
 *
 * A thin lens of focal length f and f-number N focused at distance s images a point at depth z as a disc of diameter
 * (f / N) * f * |z - s| / (z * (s - f)) on the sensor; as a radius in pixels of a sensor `sensor_height` tall that is
 * h * (f * f / (2 N (s - f) sensor_height)) * |1 - s / z|, so aperture = f * f / (2 N (s - f) sensor_height): a 50 mm lens at
 * f/1.8 focused at 2 m on a 24 mm sensor has aperture 0.0148.
 */
#ifndef RSRT_DOF_H
#define RSRT_DOF_H

#include <stddef.h>
#include <stdint.h>

#include "rsrt.h" /* rsrt_dof_params */
#include "rsrt_dof_table.h"
#include "rsrt_temporal.h" /* rsrt_tp_camera, rsrt_tp_center_ray, rsrt_tp_dot */

#define RSRT_DOF_RADIUS 8u             /* rsrt_dof_params defaults */
#define RSRT_DOF_APERTURE 0.01f
#define RSRT_DOF_FOCUS_DISTANCE 1.0f
#define RSRT_DOF_FLAGS 0u

/* a prepared texel: the colour and the signed blur radius */
typedef struct __attribute__((aligned(16))) rsrt_dof_texel { float r, g, b, rad; } rsrt_dof_texel;
/* the running sums of one output pixel.  The colour sums start at -0: (-0) + x is x for every x, -0 included, so a sum of one term is
 * that term bit for bit */
typedef struct rsrt_dof_acc { float r, g, b, w; } rsrt_dof_acc;
#define RSRT_DOF_ACC_INIT {-0.0f, -0.0f, -0.0f, 0.0f}

/* what is constant over one frame */
typedef struct rsrt_dof_frame {
    rsrt_tp_camera cam;
    float forward[3];      /* the optical axis: minus the third column of cam.rot */
    unsigned width, height;
    float aspect;          /* W / H */
    float total;           /* samples in a pixel's sum */
    float focus_distance;
    float A;               /* aperture * (float)height */
    float R;               /* (float)max_radius */
    int max_radius;
} rsrt_dof_frame;

RSRT_HD int rsrt_dof_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }

RSRT_HD int rsrt_dof_params_ok(const rsrt_dof_params *p)
{
    return rsrt_dof_finite(p->focus_distance) && p->focus_distance > 0.0f && rsrt_dof_finite(p->aperture) && p->aperture >= 0.0f &&
           p->max_radius >= 1u && p->max_radius <= (uint32_t)RSRT_DOF_MAX_RADIUS && p->flags == 0u;
}

/* pos, rot (rsrt_tp_camera's column-major 3x3) and fov_y of the camera the source was rendered with; p must be rsrt_dof_params_ok */
RSRT_HD void rsrt_dof_frame_init(rsrt_dof_frame *fr, const float pos[3], const float rot[9], float fov_y, unsigned width, unsigned height,
                                 float total, const rsrt_dof_params *p)
{
    rsrt_tp_camera_init(&fr->cam, pos, rot, fov_y);
    for (int i = 0; i < 3; i++) fr->forward[i] = -rot[6 + i];
    fr->width = width;
    fr->height = height;
    fr->aspect = (float)width / (float)height;
    fr->total = total;
    fr->focus_distance = p->focus_distance;
    fr->A = p->aperture * (float)height;
    fr->R = (float)p->max_radius;
    fr->max_radius = (int)p->max_radius;
}

/* the depth of pixel (x, y) along the optical axis from its first-hit record; +inf on sky */
RSRT_HD float rsrt_dof_depth(const rsrt_dof_frame *fr, int x, int y, const float rec[8])
{
    if (!(rec[3] > 0.0f)) return __builtin_inff();
    float d[3];
    rsrt_tp_center_ray(&fr->cam, fr->width, fr->height, fr->aspect, x, y, d);
    const float c = rsrt_tp_dot(d, fr->forward);
    return (rec[7] / rec[3]) * c;
}

/* the signed blur radius of pixel (x, y), in pixels */
RSRT_HD float rsrt_dof_coc(const rsrt_dof_frame *fr, int x, int y, const float rec[8])
{
    float r = fr->A;
    if (rec[3] > 0.0f) {
        const float t = fr->focus_distance / rsrt_dof_depth(fr, x, y, rec);
        r = fr->A * (1.0f - t);
    }
    r = r < -fr->R ? -fr->R : (r > fr->R ? fr->R : r);
    return r == r ? r : 0.0f;
}

RSRT_HD rsrt_dof_texel rsrt_dof_prepare(const rsrt_dof_frame *fr, int x, int y, const float sum[3], const float rec[8])
{
    rsrt_dof_texel t;
    t.r = sum[0] / fr->total;
    t.g = sum[1] / fr->total;
    t.b = sum[2] / fr->total;
    t.rad = rsrt_dof_coc(fr, x, y, rec);
    return t;
}

/* max(|r|, 0.5f): the radius a texel spreads over where nothing occludes it */
RSRT_HD float rsrt_dof_spread(float r)
{
    const float a = r < 0.0f ? -r : r;
    return a < 0.5f ? 0.5f : a;
}
/* the weight that normalises a disc of radius a by its area */
RSRT_HD float rsrt_dof_area(float a) { return 0.25f / (a * a); }
/* ceil(|r|) for |r| <= RSRT_DOF_MAX_RADIUS */
RSRT_HD int rsrt_dof_ceil_abs(float r)
{
    const float a = r < 0.0f ? -r : r;
    const int c = (int)a;
    return (float)c < a ? c + 1 : c;
}

/* One tap.  The pixel: r_p, a_p = rsrt_dof_spread(r_p), w_p = rsrt_dof_area(a_p).  The tap: its colour, r_q and
 * w_q = rsrt_dof_area(rsrt_dof_spread(r_q)); dist = RSRT_DOF_DIST of the offset. */
RSRT_HD void rsrt_dof_tap(rsrt_dof_acc *acc, float r_p, float a_p, float w_p, float cr, float cg, float cb, float r_q, float w_q, float dist)
{
    float a = rsrt_dof_spread(r_q), w = w_q;
    if (r_q > r_p && a_p < a) { a = a_p; w = w_p; }
    float k = (a + 0.5f) - dist;
    k = k < 0.0f ? 0.0f : (k > 1.0f ? 1.0f : k);
    if (k == 0.0f) return;
    const float wgt = k * w;
    acc->r = acc->r + wgt * cr;
    acc->g = acc->g + wgt * cg;
    acc->b = acc->b + wgt * cb;
    acc->w = acc->w + wgt;
}

RSRT_HD float rsrt_dof_dist(int dx, int dy) { return RSRT_DOF_DIST[(dy + RSRT_DOF_MAX_RADIUS) * RSRT_DOF_TABLE_WIDTH + (dx + RSRT_DOF_MAX_RADIUS)]; }

/* the output pixel (x, y) of a stored prepared image (w x h texels, rows of w): out = (rgb, 1) */
RSRT_HD void rsrt_dof_pixel(const rsrt_dof_texel *img, int w, int h, int max_radius, int x, int y, float out[4])
{
    const rsrt_dof_texel p = img[(size_t)y * (size_t)w + (size_t)x];
    const float a_p = rsrt_dof_spread(p.rad), w_p = rsrt_dof_area(a_p);
    rsrt_dof_acc acc = RSRT_DOF_ACC_INIT;
    for (int dy = -max_radius; dy <= max_radius; dy++)
        for (int dx = -max_radius; dx <= max_radius; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const rsrt_dof_texel q = img[(size_t)qy * (size_t)w + (size_t)qx];
            rsrt_dof_tap(&acc, p.rad, a_p, w_p, q.r, q.g, q.b, q.rad, rsrt_dof_area(rsrt_dof_spread(q.rad)), rsrt_dof_dist(dx, dy));
        }
    out[0] = acc.r / acc.w;
    out[1] = acc.g / acc.w;
    out[2] = acc.b / acc.w;
    out[3] = 1.0f;
}

#endif
