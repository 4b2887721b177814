// The noise estimate (csrc/hip/rt_noise.h: rt_noise_tile_kernel, rsrt_noise_download's summary) run on the CPU over
// include/rsrt_noise.h, the header the kernel uses — built by tests/test_noise.py with g++ -ffp-contract=off and compared bit for bit
// with the numpy restatement (tests/noise_ref.py).
#include <cstddef>
#include <cstdint>

#include "rsrt_noise.h"

// tiles: ceil(W / tile_w) * ceil(H / tile_h) floats, row-major; summary: max, mean; returns the tiles above the threshold, or
// 0xffffffff for a tile the estimate does not take
extern "C" uint32_t noise_tiles(const float *snap /* W*H*4 */, const float *acc /* W*H*4 */, uint32_t W, uint32_t H, uint32_t n1, uint32_t n2,
                                uint32_t tile_w, uint32_t tile_h, float threshold, float *tiles, float *summary /* 2 */)
{
    if (!rsrt_noise_tile_ok(tile_w, tile_h)) return 0xffffffffu;
    const uint32_t tiles_x = (W - 1) / tile_w + 1, tiles_y = (H - 1) / tile_h + 1, T = tile_w * tile_h;
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        for (uint32_t tx = 0; tx < tiles_x; tx++) {
            float v[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
                v[lane] = 0.0f;
                for (uint32_t i = lane; i < T; i += 64) {
                    const uint32_t x = tx * tile_w + i % tile_w, y = ty * tile_h + i / tile_w;
                    if (x >= W || y >= H) continue;
                    const size_t p = (size_t)y * W + x;
                    v[lane] = v[lane] + rsrt_noise_pixel(snap + 4 * p, (float)n1, acc + 4 * p, (float)n2);
                }
            }
            for (uint32_t k = 32; k >= 1; k >>= 1) {
                float w[64];
                for (uint32_t lane = 0; lane < 64; lane++) w[lane] = v[lane] + v[lane ^ k];
                for (uint32_t lane = 0; lane < 64; lane++) v[lane] = w[lane];
            }
            tiles[(size_t)ty * tiles_x + tx] = v[0] / (float)rsrt_noise_tile_count(tx, ty, tile_w, tile_h, W, H);
        }
    const size_t n = (size_t)tiles_x * tiles_y;
    float mx = tiles[0], sum = 0.0f;
    uint32_t above = 0;
    for (size_t i = 0; i < n; i++) {
        if (tiles[i] > mx) mx = tiles[i];
        sum = sum + tiles[i];
        above += rsrt_noise_above(tiles[i], threshold) ? 1u : 0u;
    }
    summary[0] = mx;
    summary[1] = sum / (float)n;
    return above;
}
