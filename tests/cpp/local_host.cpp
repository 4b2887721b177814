// The local exposure pass and the graded display (csrc/hip/rt_local.h) run on the CPU over include/rsrt_local.h, the header the
// kernels use — built by tests/test_local.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement
// (tests/local_ref.py).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rsrt_local.h"

// out: h*w words: q of every pixel, or RSRT_LOCAL_SKIPPED
extern "C" void local_q_map(const float *sums /* h*w*4 */, size_t n, float total, uint32_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_local_q_of(sums + 4 * i, total);
}

extern "C" uint32_t local_q(float L) { return rsrt_local_q(L); }
extern "C" uint32_t local_meter_word(float L) { return rsrt_exposure_word(L); }
extern "C" float local_luminance(const float *sum, float total) { return rsrt_exposure_luminance(sum, total); }

// out: 2 * gx * gy * 32 words: the raw grid, pixels counted one by one
extern "C" void local_raw_grid(const float *sums, int h, int w, float total, uint32_t cell, uint32_t *out)
{
    const uint32_t gx = rsrt_local_cells((uint32_t)w, cell), gy = rsrt_local_cells((uint32_t)h, cell);
    for (size_t i = 0; i < 2u * gx * gy * RSRT_LOCAL_GZ; i++) out[i] = 0u;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t q = rsrt_local_q_of(sums + 4 * ((size_t)y * w + x), total);
            if (q == RSRT_LOCAL_SKIPPED) continue;
            const size_t at = rsrt_local_word(gx, gy, (uint32_t)x / cell, (uint32_t)y / cell, q >> 8);
            out[at] += 1u;
            out[at + 1] += q;
        }
}

// grid (gx x gy x 32 cells) -> its tent along x, then y, then z, in place
extern "C" void local_blur(uint32_t *grid, uint32_t gx, uint32_t gy)
{
    const uint32_t len[3] = {gx, gy, RSRT_LOCAL_GZ};
    std::vector<uint32_t> tmp(2u * (size_t)gx * gy * RSRT_LOCAL_GZ);
    for (int axis = 0; axis < 3; axis++) {
        for (uint32_t z = 0; z < RSRT_LOCAL_GZ; z++)
            for (uint32_t y = 0; y < gy; y++)
                for (uint32_t x = 0; x < gx; x++) {
                    const uint32_t at[3] = {x, y, z};
                    uint32_t lo[3] = {x, y, z}, hi[3] = {x, y, z};
                    lo[axis] -= 1u;
                    hi[axis] += 1u;
                    for (uint32_t k = 0; k < 2; k++) {
                        const uint32_t before = at[axis] > 0u ? grid[rsrt_local_word(gx, gy, lo[0], lo[1], lo[2]) + k] : 0u;
                        const uint32_t after = at[axis] + 1u < len[axis] ? grid[rsrt_local_word(gx, gy, hi[0], hi[1], hi[2]) + k] : 0u;
                        tmp[rsrt_local_word(gx, gy, x, y, z) + k] = rsrt_local_tent(before, grid[rsrt_local_word(gx, gy, x, y, z) + k], after);
                    }
                }
        for (size_t i = 0; i < tmp.size(); i++) grid[i] = tmp[i];
    }
}

// per pixel, from a blurred grid: base (NaN-free only where the pixel is counted; 0 is written for a skipped one), den > 0 (0 / 1) and the gain
extern "C" void local_gains(const float *sums, int h, int w, float total, float exposure, const rsrt_local_params *p, const uint32_t *grid, uint32_t cell,
                            float *base_out, unsigned char *den_positive, float *gain_out)
{
    const uint32_t gx = rsrt_local_cells((uint32_t)w, cell), gy = rsrt_local_cells((uint32_t)h, cell);
    const float mid = rsrt_local_mid(p->key, exposure);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint32_t q = rsrt_local_q_of(sums + 4 * i, total);
            gain_out[i] = rsrt_local_gain_at(grid, gx, gy, cell, x, y, q, mid, p);
            base_out[i] = 0.0f;
            den_positive[i] = 0;
            if (q == RSRT_LOCAL_SKIPPED) continue;
            base_out[i] = rsrt_local_slice(grid, gx, gy, cell, x, y, q);
            // den alone, with the slice's weights: the eight counts against a sum that is 1 everywhere give num = den
            int x0, x1, y0, y1, z0, z1;
            float tx, ty, tz;
            rsrt_local_axis(rsrt_local_u(x, cell, (int)gx), (int)gx, &x0, &x1, &tx);
            rsrt_local_axis(rsrt_local_u(y, cell, (int)gy), (int)gy, &y0, &y1, &ty);
            rsrt_local_axis(rsrt_local_uz(q), (int)RSRT_LOCAL_GZ, &z0, &z1, &tz);
            const int xs[2] = {x0, x1}, ys[2] = {y0, y1}, zs[2] = {z0, z1};
            const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty}, wz[2] = {1.0f - tz, tz};
            float den = 0.0f;
            for (int k = 0; k < 8; k++)
                den = den + ((wz[k >> 2] * wy[(k >> 1) & 1]) * wx[k & 1]) *
                                (float)grid[rsrt_local_word(gx, gy, (uint32_t)xs[k & 1], (uint32_t)ys[(k >> 1) & 1], (uint32_t)zs[k >> 2])];
            den_positive[i] = den > 0.0f;
        }
}

// out: h*w RGBA8 pixels; gain: h*w; b: ceil(h / 2) x ceil(w / 2) RGBA texels, looked at only with intensity > 0
extern "C" void local_display(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b, unsigned char *out)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    std::vector<rsrt_bloom_texel> B((size_t)bw * bh);
    if (intensity > 0.0f)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_bloom_rgb up = intensity > 0.0f ? rsrt_bloom_up_at(B.data(), bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
            rsrt_display_pixel_local(sums + 4 * i, total, exposure, intensity, up, gain[i], out + 4 * i);
            out[4 * i + 3] = 255;
        }
}

extern "C" void local_exp2(const float *e, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_local_exp2(e[i]);
}

extern "C" int local_params_ok(const rsrt_local_params *p) { return rsrt_local_params_ok(p); }
extern "C" int local_cell_ok(uint32_t cell) { return rsrt_local_cell_ok(cell); }

extern "C" void local_defaults(rsrt_local_params *p, uint32_t *cell)
{
    *p = rsrt_local_params{RSRT_LOCAL_SHADOWS, RSRT_LOCAL_HIGHLIGHTS, RSRT_LOCAL_KEY, RSRT_LOCAL_MAX_STOPS, 0u, 0u};
    *cell = RSRT_LOCAL_CELL;
}

// size of rsrt_local_params, then the offsets of highlights, key, max_stops, flags, _pad; RSRT_LOCAL_GZ
extern "C" void local_layout(uint32_t *out /* 7 */)
{
    const size_t v[7] = {sizeof(rsrt_local_params), offsetof(rsrt_local_params, highlights), offsetof(rsrt_local_params, key), offsetof(rsrt_local_params, max_stops),
                         offsetof(rsrt_local_params, flags), offsetof(rsrt_local_params, _pad), RSRT_LOCAL_GZ};
    for (int i = 0; i < 7; i++) out[i] = (uint32_t)v[i];
}
