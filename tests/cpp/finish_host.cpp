// The finished display (csrc/hip/rt_finish.h) run on the CPU over include/rsrt_finish.h, the header the kernel uses — built by
// tests/test_finish.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/finish_ref.py).  With
// -DFINISH_HOST_MAIN it is a program of its own, built with -fsanitize=address,undefined, that walks frames of special values through
// every step, so that the clamped cross, the threshold table's two reads and the LUT gather are clean on the host.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rsrt_finish.h"

namespace {

int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the records of a frame of sdr rgb (h*w*3)
std::vector<float> records(const float *sdr, int h, int w)
{
    std::vector<float> rec((size_t)h * w * 4);
    for (size_t i = 0; i < (size_t)h * w; i++) rsrt_finish_record(sdr + 3 * i, rec.data() + 4 * i);
    return rec;
}

} // namespace

extern "C" void finish_records(const float *sdr, size_t n, float *out /* n*4 */)
{
    for (size_t i = 0; i < n; i++) rsrt_finish_record(sdr + 3 * i, out + 4 * i);
}

// steps 2, 3 and 5 of a frame of sdr rgb: out h*w*3 encoded rgb after the sharpener and the grain
extern "C" void finish_shape(const float *sdr, int h, int w, const rsrt_finish_params *p, float *out)
{
    const std::vector<float> rec = records(sdr, h, w);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const auto at = [&](int xx, int yy) { return rec.data() + 4 * ((size_t)clampi(yy, h - 1) * w + clampi(xx, w - 1)); };
            rsrt_finish_shape(at(x, y - 1), at(x - 1, y), at(x, y), at(x + 1, y), at(x, y + 1), rsrt_finish_hash_base((uint32_t)x, (uint32_t)y, p->seed), p,
                              out + 3 * ((size_t)y * w + x));
        }
}

// steps 2 to 7 of a frame of sdr rgb: out h*w RGBA8 pixels
extern "C" void finish_frame(const float *sdr, int h, int w, const rsrt_finish_params *p, unsigned char *out)
{
    const std::vector<float> rec = records(sdr, h, w);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const auto at = [&](int xx, int yy) { return rec.data() + 4 * ((size_t)clampi(yy, h - 1) * w + clampi(xx, w - 1)); };
            const size_t i = (size_t)y * w + x;
            rsrt_finish_pixel(sdr + 3 * i, at(x, y - 1), at(x - 1, y), at(x, y), at(x + 1, y), at(x, y + 1), (uint32_t)x, (uint32_t)y, p, out + 4 * i);
            out[4 * i + 3] = 255;
        }
}

// step 1 of a frame: sdr_out h*w*3.  gain: h*w or NULL (1); b: ceil(h / 2) x ceil(w / 2) RGBA texels, looked at only with intensity > 0;
// lut4: n^3 nodes of 4 floats, looked at only with colour->lut_strength > 0
extern "C" void finish_sdr(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                           const rsrt_colour_params *colour, const float *lut4, uint32_t n, float *sdr_out)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    std::vector<rsrt_bloom_texel> B((size_t)bw * bh);
    if (intensity > 0.0f)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_bloom_rgb up = intensity > 0.0f ? rsrt_bloom_up_at(B.data(), bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
            rsrt_finish_sdr(sums + 4 * i, total, exposure, intensity, up, gain ? gain[i] : 1.0f, colour, lut4, n, sdr_out + 3 * i);
        }
}

// the whole pass on the CPU: out h*w RGBA8 pixels
extern "C" void finish_display(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                               const rsrt_colour_params *colour, const float *lut4, uint32_t n, const rsrt_finish_params *p, unsigned char *out)
{
    std::vector<float> sdr((size_t)h * w * 3);
    finish_sdr(sums, h, w, total, exposure, gain, intensity, b, colour, lut4, n, sdr.data());
    finish_frame(sdr.data(), h, w, p, out);
}

extern "C" void finish_hash(const uint32_t *x, const uint32_t *y, size_t n, uint32_t seed, uint32_t k, uint32_t *words, float *uniforms)
{
    for (size_t i = 0; i < n; i++) {
        words[i] = rsrt_finish_hash(x[i], y[i], seed, k);
        uniforms[i] = rsrt_finish_uniform(words[i]);
    }
}

extern "C" void finish_quantise(const float *x, const float *u1, const float *u2, size_t n, float dither, unsigned char *out)
{
    for (size_t i = 0; i < n; i++) out[i] = (unsigned char)rsrt_finish_quantise(x[i], dither, u1[i], u2[i]);
}

extern "C" int finish_params_ok(const rsrt_finish_params *p) { return rsrt_finish_params_ok(p); }

extern "C" void finish_defaults(rsrt_finish_params *p)
{
    *p = rsrt_finish_params{RSRT_FINISH_SHARPNESS, RSRT_FINISH_GRAIN, RSRT_FINISH_DITHER, RSRT_FINISH_SEED, RSRT_FINISH_FLAGS, {0u, 0u, 0u}};
}

// size of rsrt_finish_params, then the offsets of grain, dither, seed, flags, _pad, then RSRT_FINISH_NOISE_AWARE
extern "C" void finish_layout(uint32_t *out /* 7 */)
{
    const size_t v[7] = {sizeof(rsrt_finish_params), offsetof(rsrt_finish_params, grain), offsetof(rsrt_finish_params, dither), offsetof(rsrt_finish_params, seed),
                         offsetof(rsrt_finish_params, flags), offsetof(rsrt_finish_params, _pad), RSRT_FINISH_NOISE_AWARE};
    for (int i = 0; i < 7; i++) out[i] = (uint32_t)v[i];
}

#ifdef FINISH_HOST_MAIN
// The sanitizer walk: frames of special sums (buffers of exactly the frame's size: a read past the clamped cross is the sanitizer's)
// through the whole pass at every corner of the parameters, frames of special sdr values through steps 2 to 7, and every threshold with
// its neighbours through the quantiser.
int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-41f, 1e-30f, 3e38f, 65519.0f, 1.0f, 0.18f, 2.5f};
    const int ns = (int)(sizeof special / sizeof special[0]);
    int bad = 0;
    const rsrt_cdl_params cdl{{1.1f, 1.0f, 0.85f}, {0.02f, 0.0f, -0.03f}, {0.9f, 1.0f, 1.2f}, 1.25f, 0u, 0u};
    std::vector<float> lut(4 * 27);
    for (uint32_t i = 0; i < 27u; i++) {
        rsrt_colour_lut_node(3u, i % 3u, (i / 3u) % 3u, i / 9u, &cdl, lut.data() + 4 * (size_t)i);
        lut[4 * (size_t)i + 3] = 1.0f;
    }
    const int shapes[][2] = {{1, 1}, {1, 2}, {3, 1}, {13, 13}, {7, 31}};
    for (const auto &s : shapes) {
        const int h = s[0], w = s[1];
        std::vector<float> sums((size_t)h * w * 4), sdr((size_t)h * w * 3);
        for (size_t i = 0; i < (size_t)h * w; i++) {
            for (int c = 0; c < 3; c++) {
                sums[4 * i + c] = special[(i * 7 + (size_t)c * 3) % ns];
                sdr[3 * i + c] = special[(i * 5 + (size_t)c) % ns];
            }
            sums[4 * i + 3] = 1.0f;
        }
        for (float sharpness : {0.0f, 0.5f, 1.0f})
            for (float grain : {0.0f, 1.0f})
                for (float dither : {0.0f, 1.0f})
                    for (uint32_t flags : {0u, (uint32_t)RSRT_FINISH_NOISE_AWARE})
                        for (float strength : {0.0f, 1.0f}) {
                            const rsrt_finish_params p{sharpness, grain, dither, 12345u, flags, {0u, 0u, 0u}};
                            const rsrt_colour_params colour{{2.0f, 1.0f, 0.5f}, strength, 0u, {0u, 0u, 0u}};
                            bad += !rsrt_finish_params_ok(&p);
                            std::vector<unsigned char> out((size_t)h * w * 4), direct((size_t)h * w * 4);
                            finish_display(sums.data(), h, w, 1.0f, 1.5f, nullptr, 0.0f, nullptr, &colour, strength > 0.0f ? lut.data() : nullptr, strength > 0.0f ? 3u : 0u, &p,
                                           out.data());
                            if (sharpness == 0.0f && grain == 0.0f && dither == 0.0f) // the colour display's bytes
                                for (size_t i = 0; i < (size_t)h * w; i++) {
                                    unsigned char rgb[3];
                                    rsrt_display_pixel_colour(sums.data() + 4 * i, 1.0f, 1.5f, 0.0f, rsrt_bloom_make(0.0f, 0.0f, 0.0f), 1.0f, &colour, lut.data(), 3u, rgb);
                                    for (int c = 0; c < 3; c++) bad += rgb[c] != out[4 * i + c];
                                }
                            finish_frame(sdr.data(), h, w, &p, direct.data());
                            std::vector<float> o((size_t)h * w * 3);
                            finish_shape(sdr.data(), h, w, &p, o.data());
                            for (float v : o) bad += !(v >= 0.0f && v <= 1.0f);
                        }
    }
    // rings of all 0 and all 1 round any centre
    for (float ring : {0.0f, 1.0f})
        for (float centre : {0.0f, 0.5f, 1.0f}) {
            const float sr[3] = {ring * ring, ring * ring, ring * ring}, se[3] = {centre * centre, centre * centre, centre * centre};
            float r[4], e[4];
            rsrt_finish_record(sr, r);
            rsrt_finish_record(se, e);
            for (uint32_t flags : {0u, (uint32_t)RSRT_FINISH_NOISE_AWARE}) {
                float o[3];
                rsrt_finish_sharpen(r, r, e, r, r, 1.0f, flags, o);
                for (float v : o) bad += !(v >= 0.0f && v <= 1.0f);
            }
        }
    // every threshold and its neighbours through the quantiser, at the ends of the dither's range
    for (int k = 0; k < 255; k++) {
        const float t = RSRT_SRGB8_THRESHOLDS[k];
        for (float x : {std::nextafter(t, 0.0f), t, std::nextafter(t, 2.0f)})
            for (float u : {0.0f, 0.99999994f}) {
                const unsigned hard = rsrt_finish_quantise(x, 0.0f, u, u), soft = rsrt_finish_quantise(x, 1.0f, u, u);
                bad += hard != rsrt_srgb8_encode(x);
                bad += soft + 1u < hard || soft > hard + 1u || soft > 255u;
            }
    }
    for (float x : {nan, inf, -inf, -1.0f, 0.0f, 1.0f, 2.0f}) bad += rsrt_finish_quantise(x, 1.0f, 0.5f, 0.25f) != rsrt_srgb8_encode(x);
    std::printf(bad ? "finish_host: %d checks failed\n" : "finish_host: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
