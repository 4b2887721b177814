// The HDR display (csrc/hip/rt_hdr.h) run on the CPU over include/rsrt_hdr.h, the header the kernel uses — built by tests/test_hdr.py
// with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/hdr_ref.py).  With -DHDR_HOST_MAIN it is a
// program of its own, built with -fsanitize=address,undefined, that walks frames of special values through every step at the corners
// of the parameters, so that the threshold table's reads (the search's and the dither's two) and the bloom gather are clean on the host.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rsrt_hdr.h"

extern "C" void hdr_table(float *out /* 1023 */)
{
    for (int i = 0; i < 1023; i++) out[i] = RSRT_PQ10_THRESHOLDS[i];
}

extern "C" void hdr_pq_encode(const float *x, size_t n, uint32_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_pq10_encode(x[i]);
}

extern "C" void hdr_quantise(const float *x, const float *u1, const float *u2, size_t n, float dither, uint32_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_hdr_quantise(x[i], dither, u1[i], u2[i]);
}

extern "C" void hdr_f16_bits(const float *x, size_t n, uint16_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_hdr_f16_bits(x[i]);
}

// steps 2, 3 and 4, one after the other, of n pixels of linear rgb: each out n*3
extern "C" void hdr_steps(const float *lin, size_t n, const rsrt_hdr_params *p, float *sanitised, float *compressed, float *nits709)
{
    const rsrt_hdr_curve cv = rsrt_hdr_curve_of(p);
    for (size_t i = 0; i < n; i++) {
        float x[3] = {lin[3 * i], lin[3 * i + 1], lin[3 * i + 2]};
        rsrt_hdr_sanitise(x);
        for (int c = 0; c < 3; c++) sanitised[3 * i + c] = x[c];
        rsrt_hdr_compress(&cv, x);
        for (int c = 0; c < 3; c++) compressed[3 * i + c] = x[c];
        rsrt_hdr_to_nits(x, p->paper_white_nits, p->peak_nits, nits709 + 3 * i);
    }
}

extern "C" void hdr_curve(const rsrt_hdr_params *p, float out[3])
{
    const rsrt_hdr_curve cv = rsrt_hdr_curve_of(p);
    out[0] = cv.P; out[1] = cv.k; out[2] = cv.d;
}

// steps 2 to 5 of n pixels: nits in the encoding's primaries, n*3
extern "C" void hdr_nits(const float *lin, size_t n, const rsrt_hdr_params *p, float *out)
{
    for (size_t i = 0; i < n; i++) rsrt_hdr_nits_of(lin + 3 * i, p, out + 3 * i);
}

// step 1 of a frame: lin_out h*w*3.  gain: h*w or NULL (1); b: ceil(h / 2) x ceil(w / 2) RGBA texels, looked at only with intensity > 0
extern "C" void hdr_linear(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                           const rsrt_colour_params *colour, float *lin_out)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    std::vector<rsrt_bloom_texel> B((size_t)bw * bh);
    if (intensity > 0.0f)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_bloom_rgb up = intensity > 0.0f ? rsrt_bloom_up_at(B.data(), bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
            rsrt_hdr_linear(sums + 4 * i, total, exposure, intensity, up, gain ? gain[i] : 1.0f, colour, lin_out + 3 * i);
        }
}

// steps 5 and 6 of a frame of Rec.2020 nits: out h*w uint32
extern "C" void hdr_pack_pq10(const float *nits, int h, int w, const rsrt_hdr_params *p, uint32_t *out)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) out[(size_t)y * w + x] = rsrt_hdr_pack_pq10(nits + 3 * ((size_t)y * w + x), (uint32_t)x, (uint32_t)y, p);
}

// steps 2 to 7 of a frame of linear rgb: out h*w uint32 (RSRT_HDR_PQ10) or h*w*4 uint16 (RSRT_HDR_SCRGB16F); levels may be NULL
extern "C" void hdr_frame(const float *lin, int h, int w, const rsrt_hdr_params *p, void *out, rsrt_hdr_levels *levels)
{
    uint32_t max_q = 0;
    uint64_t sum_q = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            float nits[3];
            rsrt_hdr_nits_of(lin + 3 * i, p, nits);
            if (p->encoding == RSRT_HDR_PQ10)
                static_cast<uint32_t *>(out)[i] = rsrt_hdr_pack_pq10(nits, (uint32_t)x, (uint32_t)y, p);
            else
                rsrt_hdr_pack_scrgb(nits, static_cast<uint16_t *>(out) + 4 * i);
            const uint32_t q = rsrt_hdr_level_q(nits);
            max_q = q > max_q ? q : max_q;
            sum_q += q;
        }
    if (levels) rsrt_hdr_levels_from(max_q, sum_q, (uint64_t)h * (uint64_t)w, levels);
}

// the whole pass on the CPU
extern "C" void hdr_display(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                            const rsrt_colour_params *colour, const rsrt_hdr_params *p, void *out, rsrt_hdr_levels *levels)
{
    std::vector<float> lin((size_t)h * w * 3);
    hdr_linear(sums, h, w, total, exposure, gain, intensity, b, colour, lin.data());
    hdr_frame(lin.data(), h, w, p, out, levels);
}

extern "C" int hdr_params_ok(const rsrt_hdr_params *p) { return rsrt_hdr_params_ok(p); }

extern "C" void hdr_defaults(rsrt_hdr_params *p)
{
    *p = rsrt_hdr_params{RSRT_HDR_PAPER_WHITE, RSRT_HDR_PEAK, RSRT_HDR_KNEE, RSRT_HDR_DITHER, RSRT_HDR_SEED, RSRT_HDR_ENCODING, RSRT_HDR_FLAGS, 0u};
}

// sizes of rsrt_hdr_params and rsrt_hdr_levels, the offsets of peak_nits, knee, dither, seed, encoding, flags, _pad, then of max_q, max_cll,
// max_fall, then RSRT_HDR_PQ10 and RSRT_HDR_SCRGB16F
extern "C" void hdr_layout(uint32_t *out /* 14 */)
{
    const size_t v[14] = {sizeof(rsrt_hdr_params), sizeof(rsrt_hdr_levels), offsetof(rsrt_hdr_params, peak_nits), offsetof(rsrt_hdr_params, knee),
                          offsetof(rsrt_hdr_params, dither), offsetof(rsrt_hdr_params, seed), offsetof(rsrt_hdr_params, encoding), offsetof(rsrt_hdr_params, flags),
                          offsetof(rsrt_hdr_params, _pad), offsetof(rsrt_hdr_levels, max_q), offsetof(rsrt_hdr_levels, max_cll), offsetof(rsrt_hdr_levels, max_fall),
                          RSRT_HDR_PQ10, RSRT_HDR_SCRGB16F};
    for (int i = 0; i < 14; i++) out[i] = (uint32_t)v[i];
}

#ifdef HDR_HOST_MAIN
// The sanitizer walk: frames of special sums (buffers of exactly the frame's size) through the whole pass in both encodings at every
// corner of the parameters, with the levels; every threshold with its neighbours through the quantiser at the ends of the dither's
// range; the half conversion over every exponent.
int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-41f, 1e-30f, 3e38f, 65504.0f, 65519.0f, 1.0f, 0.18f, 2.5f, 40.0f};
    const int ns = (int)(sizeof special / sizeof special[0]);
    int bad = 0;
    const int shapes[][2] = {{1, 1}, {1, 2}, {3, 1}, {13, 13}, {7, 31}};
    const float corners[][3] = {{203.0f, 1000.0f, 0.5f}, {203.0f, 1000.0f, 0.0f}, {100.0f, 100.0f, 0.95f}, {1.0f, 10000.0f, 0.95f}, {10000.0f, 10000.0f, 0.0f}, {80.0f, 10000.0f, 0.25f}};
    for (const auto &s : shapes) {
        const int h = s[0], w = s[1];
        const int bw = (w + 1) / 2, bh = (h + 1) / 2;
        std::vector<float> sums((size_t)h * w * 4), gain((size_t)h * w), b((size_t)bw * bh * 4);
        for (size_t i = 0; i < (size_t)h * w; i++) {
            for (int c = 0; c < 3; c++) sums[4 * i + c] = special[(i * 7 + (size_t)c * 3) % ns];
            sums[4 * i + 3] = 1.0f;
            gain[i] = 0.5f + (float)(i % 5);
        }
        for (size_t i = 0; i < b.size(); i++) b[i] = (float)(i % 9) * 0.25f;
        for (const auto &k : corners)
            for (uint32_t enc : {(uint32_t)RSRT_HDR_PQ10, (uint32_t)RSRT_HDR_SCRGB16F})
                for (float dither : {0.0f, 1.0f})
                    for (float intensity : {0.0f, 0.5f}) {
                        if (enc == RSRT_HDR_SCRGB16F && dither > 0.0f) continue;
                        const rsrt_hdr_params p{k[0], k[1], k[2], dither, 12345u, enc, 0u, 0u};
                        const rsrt_colour_params colour{{2.0f, 1.0f, 0.5f}, 0.0f, 0u, {0u, 0u, 0u}};
                        bad += !rsrt_hdr_params_ok(&p);
                        std::vector<unsigned char> out((size_t)h * w * (enc == RSRT_HDR_PQ10 ? 4 : 8));
                        rsrt_hdr_levels lv;
                        hdr_display(sums.data(), h, w, 1.0f, 1.5f, intensity > 0.0f ? gain.data() : nullptr, intensity, b.data(), &colour, &p, out.data(), &lv);
                        const unsigned peak_code = rsrt_pq10_encode(p.peak_nits);
                        if (enc == RSRT_HDR_PQ10)
                            for (size_t i = 0; i < (size_t)h * w; i++) {
                                const uint32_t word = reinterpret_cast<const uint32_t *>(out.data())[i];
                                bad += (word >> 30) != 3u;
                                for (int c = 0; c < 3; c++) bad += ((word >> (10 * c)) & 1023u) > peak_code;
                            }
                        bad += !(lv.max_cll <= p.peak_nits && lv.max_fall <= lv.max_cll);
                    }
    }
    // every threshold and its neighbours through the quantiser, at the ends of the dither's range
    for (int k = 0; k < 1023; k++) {
        const float t = RSRT_PQ10_THRESHOLDS[k];
        for (float x : {std::nextafter(t, 0.0f), t, std::nextafter(t, 20000.0f)})
            for (float u : {0.0f, 0.99999994f}) {
                const unsigned hard = rsrt_hdr_quantise(x, 0.0f, u, u), soft = rsrt_hdr_quantise(x, 1.0f, u, u);
                bad += hard != rsrt_pq10_encode(x) || hard != (unsigned)(x >= t ? k + 1 : k);
                bad += soft + 1u < hard || soft > hard + 1u || soft > 1023u;
            }
    }
    for (float x : {nan, inf, -inf, -1.0f, 0.0f, 10000.0f, 20000.0f}) bad += rsrt_hdr_quantise(x, 1.0f, 0.5f, 0.25f) != rsrt_pq10_encode(x);
    bad += rsrt_pq10_encode(0.0f) != 0u || rsrt_pq10_encode(10000.0f) != 1023u || rsrt_pq10_encode(nan) != 0u;
    // the half conversion: one value an exponent, and the edges
    for (int e = -30; e <= 17; e++) {
        const float v = std::ldexp(1.3333f, e);
        const uint16_t bits = rsrt_hdr_f16_bits(v);
        bad += e >= -14 && e <= 15 && (bits >> 10) != (unsigned)(e + 15);
    }
    bad += rsrt_hdr_f16_bits(1.0f) != 0x3c00u || rsrt_hdr_f16_bits(125.0f) != 0x57d0u || rsrt_hdr_f16_bits(0.0f) != 0u || rsrt_hdr_f16_bits(65520.0f) != 0x7c00u ||
           rsrt_hdr_f16_bits(5.9604645e-08f) != 1u || rsrt_hdr_f16_bits(-2.0f) != 0xc000u || (rsrt_hdr_f16_bits(nan) & 0x7c00u) != 0x7c00u;
    std::printf(bad ? "hdr_host: %d checks failed\n" : "hdr_host: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
