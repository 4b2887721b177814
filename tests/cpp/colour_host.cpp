// The white-balance meter, the colour LUT and the colour display (csrc/hip/rt_colour.h) run on the CPU over include/rsrt_colour.h, the
// header the kernels use — built by tests/test_colour.py with g++ -ffp-contract=off and compared bit for bit with the numpy
// restatement (tests/colour_ref.py).  With its own main, built as a program with -fsanitize=address,undefined, it walks the special
// pixels and the smallest LUTs, so that the NaN and the edge index paths of the gather are clean on the host.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rsrt_colour.h"

// out: 4097 words, pixels counted one by one
extern "C" void colour_hist(const float *sums /* n*4 */, size_t n, float total, uint32_t *out)
{
    for (uint32_t i = 0; i < RSRT_WHITE_WORDS; i++) out[i] = 0u;
    for (size_t i = 0; i < n; i++) out[rsrt_white_word(sums + 4 * i, total)] += 1u;
}

extern "C" void colour_ilog2(const float *x, size_t n, int32_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_colour_ilog2(x[i]);
}

extern "C" void colour_white(const uint32_t *hist, const rsrt_white_params *p, rsrt_white_result *out) { rsrt_white_from_histogram(hist, p, out); }

extern "C" void colour_log2(const float *x, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_colour_log2(x[i]);
}

extern "C" void colour_pow(const float *x, size_t n, float p, float *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_colour_pow(x[i], p);
}

// out: n^3 nodes of 4 floats (rgb, 1), red fastest: what the device holds
extern "C" void colour_bake(uint32_t n, const rsrt_cdl_params *p, float *out)
{
    for (uint32_t i = 0; i < n * n * n; i++) {
        rsrt_colour_lut_node(n, i % n, (i / n) % n, i / (n * n), p, out + 4 * (size_t)i);
        out[4 * (size_t)i + 3] = 1.0f;
    }
}

extern "C" void colour_lut_at(const float *lut4, uint32_t n, const float *enc /* count*3 */, size_t count, float *out)
{
    for (size_t i = 0; i < count; i++) rsrt_colour_lut_at(lut4, n, enc + 3 * i, out + 3 * i);
}

// out: h*w RGBA8 pixels; gain: h*w or NULL (1); b: ceil(h / 2) x ceil(w / 2) RGBA texels, looked at only with intensity > 0; lut4: n^3
// nodes of 4 floats, looked at only with colour->lut_strength > 0
extern "C" void colour_display(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                               const rsrt_colour_params *colour, const float *lut4, uint32_t n, unsigned char *out)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    std::vector<rsrt_bloom_texel> B((size_t)bw * bh);
    if (intensity > 0.0f)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_bloom_rgb up = intensity > 0.0f ? rsrt_bloom_up_at(B.data(), bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
            rsrt_display_pixel_colour(sums + 4 * i, total, exposure, intensity, up, gain ? gain[i] : 1.0f, colour, lut4, n, out + 4 * i);
            out[4 * i + 3] = 255;
        }
}

extern "C" int colour_white_params_ok(const rsrt_white_params *p) { return rsrt_white_params_ok(p); }
extern "C" int colour_cdl_params_ok(const rsrt_cdl_params *p) { return rsrt_cdl_params_ok(p); }
extern "C" int colour_params_ok(const rsrt_colour_params *p) { return rsrt_colour_params_ok(p); }
extern "C" int colour_lut_size_ok(uint32_t n) { return rsrt_colour_lut_size_ok(n); }

extern "C" void colour_defaults(rsrt_white_params *w, rsrt_cdl_params *c, uint32_t *size, float *strength)
{
    *w = rsrt_white_params{RSRT_WHITE_GATE, RSRT_WHITE_ITERATIONS, RSRT_WHITE_MIN_PERMILLE, RSRT_WHITE_STRENGTH, RSRT_WHITE_MAX_STOPS, RSRT_WHITE_BLEND, {0.0f, 0.0f, 0.0f}, 0u};
    *c = rsrt_cdl_params{{RSRT_CDL_SLOPE, RSRT_CDL_SLOPE, RSRT_CDL_SLOPE}, {RSRT_CDL_OFFSET, RSRT_CDL_OFFSET, RSRT_CDL_OFFSET},
                         {RSRT_CDL_POWER, RSRT_CDL_POWER, RSRT_CDL_POWER}, RSRT_CDL_SATURATION, 0u, 0u};
    *size = RSRT_COLOUR_LUT_SIZE;
    *strength = RSRT_COLOUR_LUT_STRENGTH;
}

// sizes of the four structs, then offsets: white_params strength, previous, flags; white_result target, illuminant, eu, gated, estimated;
// cdl_params offset, power, saturation, flags; colour_params lut_strength, flags, _pad; then RSRT_WHITE_WORDS
extern "C" void colour_layout(uint32_t *out /* 20 */)
{
    const size_t v[20] = {sizeof(rsrt_white_params), sizeof(rsrt_white_result), sizeof(rsrt_cdl_params), sizeof(rsrt_colour_params),
                          offsetof(rsrt_white_params, strength), offsetof(rsrt_white_params, previous), offsetof(rsrt_white_params, flags),
                          offsetof(rsrt_white_result, target), offsetof(rsrt_white_result, illuminant), offsetof(rsrt_white_result, eu),
                          offsetof(rsrt_white_result, gated), offsetof(rsrt_white_result, estimated),
                          offsetof(rsrt_cdl_params, offset), offsetof(rsrt_cdl_params, power), offsetof(rsrt_cdl_params, saturation), offsetof(rsrt_cdl_params, flags),
                          offsetof(rsrt_colour_params, lut_strength), offsetof(rsrt_colour_params, flags), offsetof(rsrt_colour_params, _pad), RSRT_WHITE_WORDS};
    for (int i = 0; i < 20; i++) out[i] = (uint32_t)v[i];
}

// The sanitizer walk: special pixels through the meter and the display, the smallest LUTs at their corners, edges and past a NaN.
int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-41f, 1e-30f, 3e38f, 65519.0f, 1.0f, 0.18f, 2.5f};
    const int ns = (int)(sizeof special / sizeof special[0]);
    std::vector<float> sums;
    for (int a = 0; a < ns; a++)
        for (int b = 0; b < ns; b++)
            for (int c = 0; c < ns; c++) {
                const float px[4] = {special[a], special[b], special[c], 1.0f};
                sums.insert(sums.end(), px, px + 4);
            }
    const size_t n = sums.size() / 4;
    int bad = 0;
    for (float total : {1.0f, 3.0f}) {
        std::vector<uint32_t> hist(RSRT_WHITE_WORDS);
        colour_hist(sums.data(), n, total, hist.data());
        uint64_t all = 0;
        for (uint32_t w : hist) all += w;
        bad += all != n;
        for (uint32_t gate : {1u, 12u, 31u})
            for (uint32_t iterations : {0u, 3u, 8u}) {
                rsrt_white_params p{gate, iterations, 0u, 1.0f, 2.0f, 0.5f, {1.0f, 1.0f, 1.0f}, 0u};
                rsrt_white_result r;
                bad += !rsrt_white_params_ok(&p);
                colour_white(hist.data(), &p, &r);
                for (int i = 0; i < 3; i++) bad += !(r.white[i] > 0.0f && r.white[i] < inf);
            }
        std::vector<uint32_t> zero(RSRT_WHITE_WORDS, 0u), edge(RSRT_WHITE_WORDS, 0u);
        edge[0] = edge[RSRT_WHITE_BINS - 1] = 0xffffffffu; // the clamped corners are outside every window
        edge[1 * RSRT_WHITE_AXIS + 1] = edge[62 * RSRT_WHITE_AXIS + 62] = 0xffffffffu;
        rsrt_white_params p{31u, 8u, 1000u, 1.0f, 4.0f, 1.0f, {0.0f, 0.0f, 0.0f}, 0u};
        rsrt_white_result r;
        colour_white(zero.data(), &p, &r);
        bad += r.estimated != 0u || r.white[0] != 1.0f;
        p.min_permille = 0u;
        colour_white(edge.data(), &p, &r);
        bad += r.estimated != 1u;
    }
    const rsrt_cdl_params cdls[] = {{{1, 1, 1}, {0, 0, 0}, {1, 1, 1}, 1.0f, 0u, 0u},
                                    {{1.1f, 1.0f, 0.85f}, {0.02f, 0.0f, -0.03f}, {0.9f, 1.0f, 1.2f}, 1.25f, 0u, 0u},
                                    {{0.0f, 16.0f, 0.7f}, {-1.0f, 1.0f, 0.3f}, {0.25f, 4.0f, 2.2f}, 0.0f, 0u, 0u},
                                    {{16.0f, 16.0f, 16.0f}, {1.0f, 1.0f, 1.0f}, {4.0f, 4.0f, 4.0f}, 4.0f, 0u, 0u}};
    const float coords[] = {0.0f, 1.0f, 0.5f, 0.25f, 0.75f, 0.99999994f, 1e-41f, 0.49999997f, 0.50000006f};
    const int nc = (int)(sizeof coords / sizeof coords[0]);
    for (uint32_t size : {2u, 3u})
        for (const rsrt_cdl_params &cdl : cdls) {
            bad += !rsrt_cdl_params_ok(&cdl);
            std::vector<float> lut(4 * (size_t)size * size * size); // exactly n^3 nodes: a read past the last one is the sanitizer's
            colour_bake(size, &cdl, lut.data());
            for (float v : lut) bad += !(v >= 0.0f && v <= 1.0f);
            for (int a = 0; a < nc; a++)
                for (int b = 0; b < nc; b++)
                    for (int c = 0; c < nc; c++) {
                        const float enc[3] = {coords[a], coords[b], coords[c]};
                        float g[3];
                        colour_lut_at(lut.data(), size, enc, 1, g);
                        for (int i = 0; i < 3; i++) bad += !(g[i] >= -1e-6f && g[i] <= 1.000001f);
                    }
            for (float strength : {0.0f, 0.5f, 1.0f}) {
                const rsrt_colour_params colour{{2.0f, 1.0f, 0.5f}, strength, 0u, {0u, 0u, 0u}};
                bad += !rsrt_colour_params_ok(&colour);
                std::vector<unsigned char> out(4 * n);
                colour_display(sums.data(), 1, (int)n, 1.0f, 1.5f, nullptr, 0.0f, nullptr, &colour, strength > 0.0f ? lut.data() : nullptr, strength > 0.0f ? size : 0u,
                               out.data());
                // a NaN channel gives byte 0 (a pixel with a negative channel is the tone map's magenta instead)
                for (size_t i = 0; i < n; i++) {
                    const float *px = &sums[4 * i];
                    if (&cdl == &cdls[0] && std::isnan(px[1]) && !(px[0] < 0.0f) && !(px[2] < 0.0f)) bad += out[4 * i + 1] != 0;
                }
            }
        }
    std::printf(bad ? "colour_host: %d checks failed\n" : "colour_host: ok\n", bad);
    return bad ? 1 : 0;
}
