// The bloom pass and the bloomed display (csrc/hip/rt_bloom.h) run on the CPU over include/rsrt_bloom.h, the header the kernels
// use — built by tests/test_bloom.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement
// (tests/bloom_ref.py).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rsrt_bloom.h"
#include "rsrt_exposure.h"

typedef std::vector<rsrt_bloom_texel> Image;

// out: n texels (rgb, 0): the prefiltered source
extern "C" void bloom_prefilter(const float *sums /* n*4 */, size_t n, float total, float exposure, float threshold, float *out /* n*4 */)
{
    for (size_t i = 0; i < n; i++)
        rsrt_bloom_store(reinterpret_cast<rsrt_bloom_texel *>(out), i,
                         rsrt_bloom_prefilter(rsrt_bloom_make(sums[4 * i], sums[4 * i + 1], sums[4 * i + 2]), total, exposure, threshold));
}

// out: ceil(h / 2) x ceil(w / 2) RGBA texels, alpha 1, as rsrt_bloom_download returns B; sums and out need not be aligned
extern "C" void bloom_image(const float *sums /* h*w*4 */, int h, int w, float total, float exposure, uint32_t levels, uint32_t flags, float threshold, float *out)
{
    std::vector<Image> d(levels + 1);
    std::vector<int> lw(levels + 1), lh(levels + 1);
    lw[0] = w;
    lh[0] = h;
    d[0].resize((size_t)w * h);
    for (size_t i = 0; i < (size_t)w * h; i++)
        rsrt_bloom_store(d[0].data(), i, rsrt_bloom_prefilter(rsrt_bloom_make(sums[4 * i], sums[4 * i + 1], sums[4 * i + 2]), total, exposure, threshold));
    for (uint32_t k = 1; k <= levels; k++) {
        lw[k] = (int)rsrt_bloom_level_size((uint32_t)w, k);
        lh[k] = (int)rsrt_bloom_level_size((uint32_t)h, k);
        d[k].resize((size_t)lw[k] * lh[k]);
        for (int y = 0; y < lh[k]; y++)
            for (int x = 0; x < lw[k]; x++)
                rsrt_bloom_store(d[k].data(), (size_t)y * lw[k] + x,
                                 rsrt_bloom_down_at(d[k - 1].data(), lw[k - 1], lh[k - 1], x, y, k == 1 && (flags & RSRT_BLOOM_KARIS)));
    }
    for (uint32_t k = levels - 1; k >= 1; k--) { // U_k over D_k, by way of the stored tent of U_{k+1}
        Image t(d[k + 1].size());
        for (int y = 0; y < lh[k + 1]; y++)
            for (int x = 0; x < lw[k + 1]; x++) rsrt_bloom_store(t.data(), (size_t)y * lw[k + 1] + x, rsrt_bloom_tent_at(d[k + 1].data(), lw[k + 1], lh[k + 1], x, y));
        for (int y = 0; y < lh[k]; y++)
            for (int x = 0; x < lw[k]; x++) {
                const size_t i = (size_t)y * lw[k] + x;
                rsrt_bloom_store(d[k].data(), i, rsrt_bloom_add(rsrt_bloom_load(d[k].data(), i), rsrt_bloom_up_at(t.data(), lw[k + 1], lh[k + 1], x, y)));
            }
    }
    const float scale = 1.0f / (float)levels;
    for (int y = 0; y < lh[1]; y++)
        for (int x = 0; x < lw[1]; x++) {
            const rsrt_bloom_rgb b = rsrt_bloom_mul(rsrt_bloom_tent_at(d[1].data(), lw[1], lh[1], x, y), scale);
            float *o = out + 4 * ((size_t)y * lw[1] + x);
            o[0] = b.r; o[1] = b.g; o[2] = b.b; o[3] = 1.0f;
        }
}

// the same chain's U_1 step as the kernels take it: up(tent(u)) without the tent in memory; out: H x W texels
extern "C" void bloom_up_tent(const float *u /* h*w*4 */, int h, int w, int H, int W, float *out)
{
    Image t((size_t)w * h);
    for (size_t i = 0; i < t.size(); i++) rsrt_bloom_store(t.data(), i, rsrt_bloom_make(u[4 * i], u[4 * i + 1], u[4 * i + 2]));
    Image o((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) rsrt_bloom_store(o.data(), (size_t)y * W + x, rsrt_bloom_up_tent_at(t.data(), w, h, x, y));
    for (size_t i = 0; i < o.size(); i++) { out[4 * i] = o[i].r; out[4 * i + 1] = o[i].g; out[4 * i + 2] = o[i].b; out[4 * i + 3] = o[i].a; }
}

// out: h*w RGBA8 pixels; b: ceil(h / 2) x ceil(w / 2) RGBA texels; bloomed = 0: rsrt_display_pixel_exposed (b and intensity not looked at)
extern "C" void bloom_display(const float *sums, int h, int w, float total, float exposure, float intensity, const float *b, int bloomed, unsigned char *out)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    Image B((size_t)bw * bh);
    if (bloomed)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            if (bloomed) rsrt_display_pixel_bloomed(sums + 4 * p, total, exposure, intensity, rsrt_bloom_up_at(B.data(), bw, bh, x, y), out + 4 * p);
            else rsrt_display_pixel_exposed(sums + 4 * p, total, exposure, out + 4 * p);
            out[4 * p + 3] = 255;
        }
}

extern "C" int bloom_params_ok(const rsrt_bloom_params *p) { return rsrt_bloom_params_ok(p); }

extern "C" void bloom_defaults(rsrt_bloom_params *p, float *intensity)
{
    *p = rsrt_bloom_params{RSRT_BLOOM_LEVELS, RSRT_BLOOM_FLAGS, RSRT_BLOOM_THRESHOLD, 0.0f};
    *intensity = RSRT_BLOOM_INTENSITY;
}

extern "C" uint32_t bloom_level_size(uint32_t n, uint32_t k) { return rsrt_bloom_level_size(n, k); }

// size of rsrt_bloom_params, then the offsets of flags, threshold, _pad; RSRT_BLOOM_MAX_LEVELS; RSRT_BLOOM_KARIS
extern "C" void bloom_layout(uint32_t *out /* 6 */)
{
    const size_t v[6] = {sizeof(rsrt_bloom_params), offsetof(rsrt_bloom_params, flags), offsetof(rsrt_bloom_params, threshold), offsetof(rsrt_bloom_params, _pad),
                         RSRT_BLOOM_MAX_LEVELS, RSRT_BLOOM_KARIS};
    for (int i = 0; i < 6; i++) out[i] = (uint32_t)v[i];
}
