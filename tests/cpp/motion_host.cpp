// The camera motion blur pass (csrc/hip/rt_motion.h) run on the CPU over include/rsrt_motion.h, the header the kernels use — built by
// tests/test_motion.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/motion_ref.py).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rsrt_motion.h"

// out: h*w prepared texels of 7 floats (rgb, l, z, ux, uy); sums h*w*4, rec h*w*8; cur, prev: pos 3, rot 9 (column-major), fov_y
extern "C" void motion_prepare(const float *sums, const float *rec, int h, int w, float total, const float *cur, const float *prev,
                               const rsrt_motion_params *p, float *out)
{
    rsrt_motion_frame fr;
    rsrt_motion_frame_init(&fr, cur, prev, (unsigned)w, (unsigned)h, total, p);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_motion_texel t = rsrt_motion_prepare(&fr, x, y, sums + 4 * i, rec + 8 * i);
            const float v[7] = {t.r, t.g, t.b, t.l, t.z, t.ux, t.uy};
            for (int k = 0; k < 7; k++) out[7 * i + k] = v[k];
        }
}

static std::vector<rsrt_motion_texel> texels(const float *prep, size_t n)
{
    std::vector<rsrt_motion_texel> img(n);
    for (size_t i = 0; i < n; i++) img[i] = rsrt_motion_texel{prep[7 * i], prep[7 * i + 1], prep[7 * i + 2], prep[7 * i + 3], prep[7 * i + 4], prep[7 * i + 5], prep[7 * i + 6]};
    return img;
}

// out: tiles_y * tiles_x * 3 (ux, uy, l): every tile's own maximum
extern "C" void motion_tile_max(const float *prep, int h, int w, float *out)
{
    const std::vector<rsrt_motion_texel> img = texels(prep, (size_t)w * h);
    const int nx = rsrt_motion_tiles(w), ny = rsrt_motion_tiles(h);
    for (int ty = 0; ty < ny; ty++)
        for (int tx = 0; tx < nx; tx++) {
            const rsrt_motion_vel m = rsrt_motion_tile_max(img.data(), w, h, tx, ty);
            float *o = out + 3 * ((size_t)ty * nx + tx);
            o[0] = m.ux; o[1] = m.uy; o[2] = m.l;
        }
}

// out: tiles_y * tiles_x * 3: every tile's neighbour maximum over the tiles' own maxima
extern "C" void motion_neighbour_max(const float *tiles, int tiles_y, int tiles_x, float *out)
{
    std::vector<rsrt_motion_vel> t((size_t)tiles_x * tiles_y);
    for (size_t i = 0; i < t.size(); i++) t[i] = rsrt_motion_vel{tiles[3 * i], tiles[3 * i + 1], tiles[3 * i + 2]};
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x; tx++) {
            const rsrt_motion_vel m = rsrt_motion_neighbour_max(t.data(), tiles_x, tiles_y, tx, ty);
            float *o = out + 3 * ((size_t)ty * tiles_x + tx);
            o[0] = m.ux; o[1] = m.uy; o[2] = m.l;
        }
}

// out: h*w RGBA texels, alpha 1, as rsrt_motion_download returns the motion image; tiles: the tiles' own maxima
extern "C" void motion_gather(const float *prep, const float *tiles, int h, int w, int taps, float *out)
{
    const std::vector<rsrt_motion_texel> img = texels(prep, (size_t)w * h);
    std::vector<rsrt_motion_vel> t((size_t)rsrt_motion_tiles(w) * rsrt_motion_tiles(h));
    for (size_t i = 0; i < t.size(); i++) t[i] = rsrt_motion_vel{tiles[3 * i], tiles[3 * i + 1], tiles[3 * i + 2]};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) rsrt_motion_pixel(img.data(), t.data(), w, h, taps, x, y, out + 4 * ((size_t)y * w + x));
}

extern "C" int motion_params_ok(const rsrt_motion_params *p) { return rsrt_motion_params_ok(p); }

extern "C" void motion_defaults(rsrt_motion_params *p) { *p = rsrt_motion_params{RSRT_MOTION_SHUTTER, RSRT_MOTION_RADIUS, RSRT_MOTION_TAPS, RSRT_MOTION_FLAGS}; }

// size of rsrt_motion_params, then the offsets of max_radius, taps, flags; RSRT_MOTION_MAX_RADIUS; RSRT_MOTION_TILE; RSRT_EXPOSURE_MOTION;
// RSRT_MOTION_MAX_TAPS
extern "C" void motion_layout(uint32_t *out /* 8 */)
{
    const size_t v[8] = {sizeof(rsrt_motion_params), offsetof(rsrt_motion_params, max_radius), offsetof(rsrt_motion_params, taps), offsetof(rsrt_motion_params, flags),
                         RSRT_MOTION_MAX_RADIUS, RSRT_MOTION_TILE, RSRT_EXPOSURE_MOTION, RSRT_MOTION_MAX_TAPS};
    for (int i = 0; i < 8; i++) out[i] = (uint32_t)v[i];
}
