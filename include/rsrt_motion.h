/*
 * rsrt_motion.h — arithmetic of the camera motion blur pass (rsrt_motion_blur, rsrt_motion_velocity_download,
 * rsrt_motion_tiles_download; include/rsrt.h "camera motion blur"), as shared inline code.
 *
 * The scene is static, so the only motion is the camera's, and the shutter is a pass over the picture: a velocity per pixel from the
 * first-hit distance and the camera of one frame earlier, the dominant velocity of every tile and of its neighbourhood, and a gather
 * along that velocity (McGuire et al. 2012, with the tap weight of Jimenez 2014).  Like rsrt_dof.h this is part of the published
 * numeric contract: plain f32 + - * /, compares, floorf and rsrt_sqrtf (-ffp-contract=off, nothing fused) in exactly the order
 * written here, so a numpy restatement reproduces every bit (tests/motion_ref.py holds it).  The centre ray and the projection are
 * rsrt_temporal.h's, taken as they are.
 *
 * Parameters (rsrt_motion_params): shutter, the fraction of the frame interval the shutter is open, finite, in [0, 1]; max_radius,
 * the largest blur half-length in pixels, 1 .. RSRT_MOTION_MAX_RADIUS = RSRT_MOTION_TILE = 16; taps along the line, even, 2 .. 32;
 * flags 0.
 *
 * Velocity of pixel p = (x, y) of a w x h frame, from its 8-float first-hit record rec (rec[3] the hit count, rec[7] the sum of hit
 * distances), the camera the source was rendered with (cur: o, and the centre ray d of p) and the camera one frame earlier (prev: o'):
 *   rsrt_tp_same_camera(cur, prev):  u = (0, 0) exactly (projecting a point back into the same camera does not return x bit for bit)
 *   otherwise  surface (rec[3] > 0): z = rec[7] / rec[3], e = (o + z d) - o';   sky: e = d, z = +inf
 *              rsrt_tp_project(prev, e) -> fx, fy; behind the previous camera: u = 0
 *              hs = 0.5f * shutter,  u = (((float)x - fx) * hs, ((float)y - fy) * hs): while the shutter is open the pixel's image
 *              travels from p - u to p + u, centred on the rendered instant
 *              a component that is not finite: u = 0
 *   l = rsrt_sqrtf(ux ux + uy uy);  l not finite (the squares overflowed): u = 0, l = 0;  l > R = (float)max_radius: s = R / l,
 *   u = u s, l = R exactly
 *   the stored z: a NaN z counts as +inf (the velocity above used the z it was given)
 * Prepared texel: the colour c = sum.rgb / total, not rounded (the accumulator: total = (float)sample_total; every other source 1),
 * l, z and u.
 *
 * Tile maximum: tiles are RSRT_MOTION_TILE = 16 pixels square, clipped at the frame.  A tile's dominant velocity is the (ux, uy, l)
 * of its texel with the greatest l, ties to the first in row-major order; every l 0: (0, 0, 0).
 * Neighbour maximum n = (nx, ny, nl) of a tile: the dominant velocity with the greatest l over the 3 x 3 tiles around it that exist,
 * ties to the first in row-major order of tiles.  With max_radius <= the tile this covers every texel that can reach the tile.
 *
 * Gather for the output pixel p in a tile with neighbour maximum n, N = taps:
 *   nl < 0.5f:  out = (c_p, 1), the source's colour bit for bit, for the whole tile
 *   otherwise for i = 0 .. N - 1:  t_i = (float)(2 i + 1) / (float)N - 1.0f,
 *       o_i = ((int)floorf(t_i nx + 0.5f), (int)floorf(t_i ny + 0.5f)),  d_i = |t_i| nl   (of the tile only, never of p: they are
 *       workgroup-uniform in the kernel; |o_i| <= ceil(nl) along each axis, since |t_i| <= 31/32)
 *     q = p + o_i; a tap outside the frame is skipped.  Inside:
 *       l'_p = max(l_p, 0.5f), l'_q likewise;  cone(d, l') = clamp(1 - d / l', 0, 1)
 *       the foreground share f of q: z_q == z_p (both sky included): 0.5f; otherwise
 *           f = 0.5f + (z_p - z_q) / (RSRT_MOTION_DEPTH_EXTENT min(z_p, z_q)), clamped to [0, 1] with a NaN falling to 0; an
 *           infinite or zero depth falls out of the clamp
 *       b = 1.0f - f,  w = f cone(d_i, l'_q) + b cone(d_i, l'_p)        (Jimenez's form; w <= 1)
 *       w == 0: the tap is SKIPPED, nothing is added (a non-finite colour times 0 is NaN)
 *       otherwise acc.rgb += w c_q, acc.w += w   (sequential, in tap order; acc.rgb starts at -0, acc.w at 0)
 *   out.rgb = acc.rgb / (float)N + (1.0f - acc.w / (float)N) c_p, alpha 1: what the taps do not cover stays the pixel's own.
 *
 * Consequences: the same camera, or shutter 0, makes every u and l 0, every tile takes the copy path and the output is the source's
 * colour bit for bit, inf and NaN included.  A sky pixel moves under a rotation only.
 */
#ifndef RSRT_MOTION_H
#define RSRT_MOTION_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rsrt.h" /* rsrt_motion_params */
#include "rsrt_temporal.h" /* rsrt_tp_camera, rsrt_tp_center_ray, rsrt_tp_project, rsrt_tp_same_camera */

#define RSRT_MOTION_TILE 16
#define RSRT_MOTION_MAX_RADIUS 16 /* = RSRT_MOTION_TILE: a texel reaches no farther than the next tile */
#define RSRT_MOTION_MAX_TAPS 32u
#define RSRT_MOTION_DEPTH_EXTENT 0.05f /* the relative depth difference over which a tap goes from half to wholly in front */
#define RSRT_MOTION_SHUTTER 0.5f       /* rsrt_motion_params defaults: a 180 degree shutter */
#define RSRT_MOTION_RADIUS 16u
#define RSRT_MOTION_TAPS 16u
#define RSRT_MOTION_FLAGS 0u

/* a prepared texel */
typedef struct rsrt_motion_texel { float r, g, b, l, z, ux, uy; } rsrt_motion_texel;
/* a velocity and its length: a tile's maximum, a neighbourhood's maximum */
typedef struct rsrt_motion_vel { float ux, uy, l; } rsrt_motion_vel;
/* the running sums of one output pixel (the colour sums start at -0: a sum of one term is that term bit for bit) */
typedef struct rsrt_motion_acc { float r, g, b, w; } rsrt_motion_acc;
#define RSRT_MOTION_ACC_INIT {-0.0f, -0.0f, -0.0f, 0.0f}

/* what is constant over one frame */
typedef struct rsrt_motion_frame {
    rsrt_tp_camera cur, prev;
    unsigned width, height;
    float aspect; /* W / H */
    float total;  /* samples in a pixel's sum */
    float hs;     /* 0.5f * shutter */
    float R;      /* (float)max_radius */
    int same;     /* rsrt_tp_same_camera(cur, prev) */
    int taps;
} rsrt_motion_frame;

RSRT_HD int rsrt_motion_finite(float x) { return x > -__builtin_inff() && x < __builtin_inff(); }

RSRT_HD int rsrt_motion_params_ok(const rsrt_motion_params *p)
{
    return rsrt_motion_finite(p->shutter) && p->shutter >= 0.0f && p->shutter <= 1.0f && p->max_radius >= 1u &&
           p->max_radius <= (uint32_t)RSRT_MOTION_MAX_RADIUS && p->taps >= 2u && p->taps <= RSRT_MOTION_MAX_TAPS && (p->taps & 1u) == 0u && p->flags == 0u;
}

/* cur, prev: pos 3, rot 9 (rsrt_tp_camera's column-major 3x3), fov_y of the camera the source was rendered with and of the one a
 * frame earlier; p must be rsrt_motion_params_ok */
RSRT_HD void rsrt_motion_frame_init(rsrt_motion_frame *fr, const float cur[13], const float prev[13], unsigned width, unsigned height, float total,
                                    const rsrt_motion_params *p)
{
    rsrt_tp_camera_init(&fr->cur, cur, cur + 3, cur[12]);
    rsrt_tp_camera_init(&fr->prev, prev, prev + 3, prev[12]);
    fr->width = width;
    fr->height = height;
    fr->aspect = (float)width / (float)height;
    fr->total = total;
    fr->hs = 0.5f * p->shutter;
    fr->R = (float)p->max_radius;
    fr->same = rsrt_tp_same_camera(&fr->cur, &fr->prev);
    fr->taps = (int)p->taps;
}

/* the velocity (ux, uy), its length l and the depth z of pixel (x, y) from its first-hit record */
RSRT_HD void rsrt_motion_velocity(const rsrt_motion_frame *fr, int x, int y, const float rec[8], float *ux, float *uy, float *l, float *z)
{
    const int surface = rec[3] > 0.0f;
    const float zz = surface ? rec[7] / rec[3] : __builtin_inff();
    *z = zz == zz ? zz : __builtin_inff();
    *ux = 0.0f;
    *uy = 0.0f;
    *l = 0.0f;
    if (fr->same) return;
    float d[3], e[3], fx = 0.0f, fy = 0.0f;
    rsrt_tp_center_ray(&fr->cur, fr->width, fr->height, fr->aspect, x, y, d);
    for (int i = 0; i < 3; i++) {
        const float X = fr->cur.pos[i] + zz * d[i];
        e[i] = surface ? X - fr->prev.pos[i] : d[i];
    }
    if (!rsrt_tp_project(&fr->prev, fr->width, fr->height, fr->aspect, e, &fx, &fy)) return;
    float vx = ((float)x - fx) * fr->hs, vy = ((float)y - fy) * fr->hs;
    if (!rsrt_motion_finite(vx) || !rsrt_motion_finite(vy)) return;
    float len = rsrt_sqrtf(vx * vx + vy * vy);
    if (!rsrt_motion_finite(len)) return;
    if (len > fr->R) {
        const float s = fr->R / len;
        vx = vx * s;
        vy = vy * s;
        len = fr->R;
    }
    *ux = vx;
    *uy = vy;
    *l = len;
}

RSRT_HD rsrt_motion_texel rsrt_motion_prepare(const rsrt_motion_frame *fr, int x, int y, const float sum[3], const float rec[8])
{
    rsrt_motion_texel t;
    t.r = sum[0] / fr->total;
    t.g = sum[1] / fr->total;
    t.b = sum[2] / fr->total;
    rsrt_motion_velocity(fr, x, y, rec, &t.ux, &t.uy, &t.l, &t.z);
    return t;
}

/* tiles along an axis of n pixels */
RSRT_HD int rsrt_motion_tiles(int n) { return (n + RSRT_MOTION_TILE - 1) / RSRT_MOTION_TILE; }

/* the dominant velocity of tile (tx, ty) of a stored prepared image (w x h texels, rows of w) */
RSRT_HD rsrt_motion_vel rsrt_motion_tile_max(const rsrt_motion_texel *img, int w, int h, int tx, int ty)
{
    rsrt_motion_vel m = {0.0f, 0.0f, 0.0f};
    for (int y = ty * RSRT_MOTION_TILE; y < (ty + 1) * RSRT_MOTION_TILE && y < h; y++)
        for (int x = tx * RSRT_MOTION_TILE; x < (tx + 1) * RSRT_MOTION_TILE && x < w; x++) {
            const rsrt_motion_texel *t = img + (size_t)y * (size_t)w + (size_t)x;
            if (t->l > m.l) { m.ux = t->ux; m.uy = t->uy; m.l = t->l; }
        }
    return m;
}

/* the neighbour maximum of tile (tx, ty) over the tiles' own maxima (tiles_x x tiles_y records, rows of tiles_x) */
RSRT_HD rsrt_motion_vel rsrt_motion_neighbour_max(const rsrt_motion_vel *tiles, int tiles_x, int tiles_y, int tx, int ty)
{
    rsrt_motion_vel m = {0.0f, 0.0f, 0.0f};
    int first = 1;
    for (int y = ty - 1; y <= ty + 1; y++)
        for (int x = tx - 1; x <= tx + 1; x++) {
            if (x < 0 || x >= tiles_x || y < 0 || y >= tiles_y) continue;
            const rsrt_motion_vel t = tiles[(size_t)y * (size_t)tiles_x + (size_t)x];
            if (first || t.l > m.l) m = t;
            first = 0;
        }
    return m;
}

/* ceil(l) for 0 <= l <= RSRT_MOTION_MAX_RADIUS: the halo a tile with neighbour maximum l reads */
RSRT_HD int rsrt_motion_ceil(float l)
{
    const int c = (int)l;
    return (float)c < l ? c + 1 : c;
}

/* tap i of N along n: its integer offset and its distance */
RSRT_HD void rsrt_motion_tap_at(const rsrt_motion_vel *n, int i, int N, int *ox, int *oy, float *dist)
{
    const float t = (float)(2 * i + 1) / (float)N - 1.0f;
    *ox = (int)floorf(t * n->ux + 0.5f);
    *oy = (int)floorf(t * n->uy + 0.5f);
    *dist = (t < 0.0f ? -t : t) * n->l;
}

RSRT_HD float rsrt_motion_spread(float l) { return l < 0.5f ? 0.5f : l; }
RSRT_HD float rsrt_motion_cone(float d, float spread)
{
    const float c = 1.0f - d / spread;
    return c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
}
/* the share of tap q that lies in front of the pixel p */
RSRT_HD float rsrt_motion_foreground(float z_p, float z_q)
{
    if (z_q == z_p) return 0.5f;
    const float f = 0.5f + (z_p - z_q) / (RSRT_MOTION_DEPTH_EXTENT * (z_p < z_q ? z_p : z_q));
    return !(f > 0.0f) ? 0.0f : (f > 1.0f ? 1.0f : f);
}

/* One tap in the frame.  The pixel: s_p = rsrt_motion_spread(l_p), z_p.  The tap: its colour, l_q, z_q, and its distance. */
RSRT_HD void rsrt_motion_tap(rsrt_motion_acc *acc, float s_p, float z_p, float dist, float cr, float cg, float cb, float l_q, float z_q)
{
    const float f = rsrt_motion_foreground(z_p, z_q);
    const float b = 1.0f - f;
    const float w = f * rsrt_motion_cone(dist, rsrt_motion_spread(l_q)) + b * rsrt_motion_cone(dist, s_p);
    if (w == 0.0f) return;
    acc->r = acc->r + w * cr;
    acc->g = acc->g + w * cg;
    acc->b = acc->b + w * cb;
    acc->w = acc->w + w;
}

/* the output of a pixel of colour c_p whose N taps gave acc */
RSRT_HD void rsrt_motion_resolve(const rsrt_motion_acc *acc, int N, float cr, float cg, float cb, float out[4])
{
    const float fn = (float)N;
    const float rest = 1.0f - acc->w / fn;
    out[0] = acc->r / fn + rest * cr;
    out[1] = acc->g / fn + rest * cg;
    out[2] = acc->b / fn + rest * cb;
    out[3] = 1.0f;
}

/* the output pixel (x, y) of a stored prepared image (w x h texels, rows of w) and its tiles' own maxima: out = (rgb, 1) */
RSRT_HD void rsrt_motion_pixel(const rsrt_motion_texel *img, const rsrt_motion_vel *tiles, int w, int h, int taps, int x, int y, float out[4])
{
    const rsrt_motion_texel p = img[(size_t)y * (size_t)w + (size_t)x];
    const rsrt_motion_vel n = rsrt_motion_neighbour_max(tiles, rsrt_motion_tiles(w), rsrt_motion_tiles(h), x / RSRT_MOTION_TILE, y / RSRT_MOTION_TILE);
    if (n.l < 0.5f) {
        out[0] = p.r; out[1] = p.g; out[2] = p.b; out[3] = 1.0f;
        return;
    }
    const float s_p = rsrt_motion_spread(p.l);
    rsrt_motion_acc acc = RSRT_MOTION_ACC_INIT;
    for (int i = 0; i < taps; i++) {
        int ox, oy;
        float dist;
        rsrt_motion_tap_at(&n, i, taps, &ox, &oy, &dist);
        const int qx = x + ox, qy = y + oy;
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
        const rsrt_motion_texel q = img[(size_t)qy * (size_t)w + (size_t)qx];
        rsrt_motion_tap(&acc, s_p, p.z, dist, q.r, q.g, q.b, q.l, q.z);
    }
    rsrt_motion_resolve(&acc, taps, p.r, p.g, p.b, out);
}

#endif
