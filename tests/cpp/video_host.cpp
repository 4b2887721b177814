// The video pass (csrc/hip/rt_video.h) run on the CPU over include/rsrt_video.h, the header the kernel uses — built by tests/test_video.py
// with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/video_ref.py).  With -DVIDEO_HOST_MAIN it is a
// program of its own, built with -fsanitize=address,undefined, that walks frames of special values of 1 x 1 to 31 x 7 through the whole
// pass in every standard, depth, layout, range and siting, so that the tables' reads, the clamped taps and the planes' stores are clean.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rsrt_video.h"

// step 2 of n values: the continuous code (not yet divided by N)
extern "C" void video_code(const float *x, size_t n, uint32_t standard, float *out)
{
    for (size_t i = 0; i < n; i++) out[i] = standard == RSRT_VIDEO_HDR10 ? rsrt_video_code_pq(x[i]) : rsrt_video_code_srgb(x[i]);
}

// steps 2 and 3 of n pixels of step 1's channels: each out n*3
extern "C" void video_signal_ycc(const float *x, size_t n, uint32_t standard, float *e, float *ycc)
{
    for (size_t i = 0; i < n; i++) {
        rsrt_video_signal(standard, x + 3 * i, e + 3 * i);
        rsrt_video_ycc(standard, e + 3 * i, ycc + 3 * i);
    }
}

// step 3 alone
extern "C" void video_ycc(const float *e, size_t n, uint32_t standard, float *ycc)
{
    for (size_t i = 0; i < n; i++) rsrt_video_ycc(standard, e + 3 * i, ycc + 3 * i);
}

namespace {

int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// step 4 of one plane c (h x w) at sample (cx, cy)
float reduce_at(const float *c, int h, int w, int cx, int cy, uint32_t siting)
{
    const auto at = [&](int x, int y) { return c[(size_t)clampi(y, h - 1) * w + clampi(x, w - 1)]; };
    const auto h121 = [&](int y) { return rsrt_video_h121(at(2 * cx - 1, y), at(2 * cx, y), at(2 * cx + 1, y)); };
    if (siting == RSRT_VIDEO_SITING_CENTRE) return rsrt_video_centre(at(2 * cx, 2 * cy), at(2 * cx + 1, 2 * cy), at(2 * cx, 2 * cy + 1), at(2 * cx + 1, 2 * cy + 1));
    if (siting == RSRT_VIDEO_SITING_LEFT) return rsrt_video_left(h121(2 * cy), h121(2 * cy + 1));
    return rsrt_video_h121(h121(2 * cy - 1), h121(2 * cy), h121(2 * cy + 1));
}

void put(unsigned char *plane, size_t i, uint32_t word, uint32_t sample_bytes)
{
    plane[i * sample_bytes] = (unsigned char)(word & 0xffu);
    if (sample_bytes == 2u) plane[2 * i + 1] = (unsigned char)(word >> 8);
}

} // namespace

// step 4 of a plane: out ceil(h / 2) x ceil(w / 2)
extern "C" void video_reduce(const float *c, int h, int w, uint32_t siting, float *out)
{
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) out[(size_t)cy * cw + cx] = reduce_at(c, h, w, cx, cy, siting);
}

// steps 4 to 6 of a frame of Y', Cb', Cr' (h*w*3): out rsrt_video_planes bytes
extern "C" void video_frame_ycc(const float *ycc, int h, int w, const rsrt_video_params *p, unsigned char *out)
{
    rsrt_video_planes_out pl;
    rsrt_video_planes((uint32_t)w, (uint32_t)h, p, &pl);
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    std::vector<float> cb((size_t)h * w), cr((size_t)h * w);
    for (size_t i = 0; i < (size_t)h * w; i++) {
        cb[i] = ycc[3 * i + 1];
        cr[i] = ycc[3 * i + 2];
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            put(out + pl.offset[0], (size_t)y * w + x, rsrt_video_word(rsrt_video_luma_code(ycc[3 * ((size_t)y * w + x)], (uint32_t)x, (uint32_t)y, p), p), pl.sample_bytes);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) {
            uint32_t codes[2];
            rsrt_video_chroma_codes(reduce_at(cb.data(), h, w, cx, cy, p->siting), reduce_at(cr.data(), h, w, cx, cy, p->siting), (uint32_t)cx, (uint32_t)cy, p, codes);
            const size_t i = (size_t)cy * cw + cx;
            if (p->layout == RSRT_VIDEO_PLANAR) {
                put(out + pl.offset[1], i, rsrt_video_word(codes[0], p), pl.sample_bytes);
                put(out + pl.offset[2], i, rsrt_video_word(codes[1], p), pl.sample_bytes);
            } else {
                put(out + pl.offset[1], 2 * i, rsrt_video_word(codes[0], p), pl.sample_bytes);
                put(out + pl.offset[1], 2 * i + 1, rsrt_video_word(codes[1], p), pl.sample_bytes);
            }
        }
}

// steps 3 to 6 of a frame of E' (h*w*3)
extern "C" void video_frame(const float *e, int h, int w, const rsrt_video_params *p, unsigned char *out)
{
    std::vector<float> ycc((size_t)h * w * 3);
    for (size_t i = 0; i < (size_t)h * w; i++) rsrt_video_ycc(p->standard, e + 3 * i, ycc.data() + 3 * i);
    video_frame_ycc(ycc.data(), h, w, p, out);
}

// step 1 of a frame: x_out h*w*3 (the sdr, or the Rec.2020 nits with hdr), levels (may be NULL; hdr only).  gain: h*w or NULL (1);
// b: ceil(h / 2) x ceil(w / 2) RGBA texels, looked at only with intensity > 0; lut4: n^3 nodes of 4 floats, looked at only with lut_strength > 0
extern "C" void video_input(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                            const rsrt_colour_params *colour, const float *lut4, uint32_t n, const rsrt_hdr_params *hdr, float *x_out, rsrt_hdr_levels *levels)
{
    const int bw = (int)rsrt_bloom_level_size((uint32_t)w, 1), bh = (int)rsrt_bloom_level_size((uint32_t)h, 1);
    std::vector<rsrt_bloom_texel> B((size_t)bw * bh);
    if (intensity > 0.0f)
        for (size_t i = 0; i < B.size(); i++) rsrt_bloom_store(B.data(), i, rsrt_bloom_make(b[4 * i], b[4 * i + 1], b[4 * i + 2]));
    uint32_t max_q = 0;
    uint64_t sum_q = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_bloom_rgb up = intensity > 0.0f ? rsrt_bloom_up_at(B.data(), bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
            if (hdr) {
                rsrt_hdr_pixel_nits(sums + 4 * i, total, exposure, intensity, up, gain ? gain[i] : 1.0f, colour, hdr, x_out + 3 * i);
                const uint32_t q = rsrt_hdr_level_q(x_out + 3 * i);
                max_q = q > max_q ? q : max_q;
                sum_q += q;
            } else {
                rsrt_finish_sdr(sums + 4 * i, total, exposure, intensity, up, gain ? gain[i] : 1.0f, colour, lut4, n, x_out + 3 * i);
            }
        }
    if (hdr && levels) rsrt_hdr_levels_from(max_q, sum_q, (uint64_t)h * (uint64_t)w, levels);
}

// the whole pass on the CPU
extern "C" void video_display(const float *sums, int h, int w, float total, float exposure, const float *gain, float intensity, const float *b,
                              const rsrt_colour_params *colour, const float *lut4, uint32_t n, const rsrt_hdr_params *hdr, const rsrt_video_params *p,
                              unsigned char *out, rsrt_hdr_levels *levels)
{
    std::vector<float> x((size_t)h * w * 3), e((size_t)h * w * 3);
    video_input(sums, h, w, total, exposure, gain, intensity, b, colour, lut4, n, hdr, x.data(), levels);
    for (size_t i = 0; i < (size_t)h * w; i++) rsrt_video_signal(p->standard, x.data() + 3 * i, e.data() + 3 * i);
    video_frame(e.data(), h, w, p, out);
}

extern "C" int video_params_ok(const rsrt_video_params *p) { return rsrt_video_params_ok(p); }

extern "C" void video_defaults(rsrt_video_params *p)
{
    *p = rsrt_video_params{RSRT_VIDEO_DEFAULT_STANDARD, RSRT_VIDEO_DEFAULT_DEPTH, RSRT_VIDEO_DEFAULT_LAYOUT, RSRT_VIDEO_DEFAULT_RANGE, RSRT_VIDEO_DEFAULT_SITING,
                           RSRT_VIDEO_DEFAULT_DITHER, RSRT_VIDEO_DEFAULT_SEED, RSRT_VIDEO_DEFAULT_FLAGS};
}

// the byte count; out: offset[3], pitch[3], width[3], height[3], planes, sample_bytes as 14 uint64
extern "C" uint64_t video_planes(uint32_t w, uint32_t h, const rsrt_video_params *p, uint64_t *out /* 14 */)
{
    rsrt_video_planes_out pl;
    const size_t n = rsrt_video_planes(w, h, p, &pl);
    for (int i = 0; i < 3; i++) {
        out[i] = pl.offset[i]; out[3 + i] = pl.pitch[i]; out[6 + i] = pl.width[i]; out[9 + i] = pl.height[i];
    }
    out[12] = pl.planes; out[13] = pl.sample_bytes;
    return n;
}

// the size of rsrt_video_params, the offsets of its fields after the first, the size of rsrt_video_planes_out, then the enumerators
extern "C" void video_layout(uint32_t *out /* 18 */)
{
    const size_t v[18] = {sizeof(rsrt_video_params), offsetof(rsrt_video_params, depth), offsetof(rsrt_video_params, layout), offsetof(rsrt_video_params, range),
                          offsetof(rsrt_video_params, siting), offsetof(rsrt_video_params, dither), offsetof(rsrt_video_params, seed), offsetof(rsrt_video_params, flags),
                          sizeof(rsrt_video_planes_out), RSRT_VIDEO_BT709, RSRT_VIDEO_HDR10, RSRT_VIDEO_SEMIPLANAR, RSRT_VIDEO_PLANAR, RSRT_VIDEO_LIMITED, RSRT_VIDEO_FULL,
                          RSRT_VIDEO_SITING_LEFT, RSRT_VIDEO_SITING_CENTRE, RSRT_VIDEO_SITING_TOPLEFT};
    for (int i = 0; i < 18; i++) out[i] = (uint32_t)v[i];
}

#ifdef VIDEO_HOST_MAIN
// The sanitizer walk: frames of special sums (buffers of exactly the frame's size) through the whole pass at every combination of the
// parameters, with a LUT for BT.709 and the levels for HDR10; every threshold of both tables with its neighbours through the code.
int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float special[] = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-41f, 1e-30f, 3e38f, 65504.0f, 65519.0f, 1.0f, 0.18f, 2.5f, 40.0f};
    const int ns = (int)(sizeof special / sizeof special[0]);
    int bad = 0;
    const rsrt_cdl_params cdl{{1.1f, 1.0f, 0.85f}, {0.02f, 0.0f, -0.03f}, {0.9f, 1.0f, 1.2f}, 1.25f, 0u, 0u};
    std::vector<float> lut(4 * 27);
    for (uint32_t i = 0; i < 27u; i++) {
        rsrt_colour_lut_node(3u, i % 3u, (i / 3u) % 3u, i / 9u, &cdl, lut.data() + 4 * (size_t)i);
        lut[4 * (size_t)i + 3] = 1.0f;
    }
    const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 3}, {13, 13}, {7, 31}};
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
        for (uint32_t standard : {RSRT_VIDEO_BT709, RSRT_VIDEO_HDR10})
            for (uint32_t depth : {8u, 10u})
                for (uint32_t layout : {RSRT_VIDEO_SEMIPLANAR, RSRT_VIDEO_PLANAR})
                    for (uint32_t range : {RSRT_VIDEO_LIMITED, RSRT_VIDEO_FULL})
                        for (uint32_t siting : {RSRT_VIDEO_SITING_LEFT, RSRT_VIDEO_SITING_CENTRE, RSRT_VIDEO_SITING_TOPLEFT})
                            for (float dither : {0.0f, 1.0f}) {
                                const rsrt_video_params p{standard, depth, layout, range, siting, dither, 12345u, 0u};
                                if (standard == RSRT_VIDEO_HDR10 && depth == 8u) {
                                    bad += rsrt_video_params_ok(&p) || rsrt_video_planes((uint32_t)w, (uint32_t)h, &p, nullptr) != 0u;
                                    continue;
                                }
                                bad += !rsrt_video_params_ok(&p);
                                const bool hdr10 = standard == RSRT_VIDEO_HDR10;
                                const rsrt_hdr_params hp{203.0f, 1000.0f, 0.5f, 0.0f, 0u, RSRT_HDR_PQ10, 0u, 0u};
                                const rsrt_colour_params colour{{2.0f, 1.0f, 0.5f}, hdr10 ? 0.0f : 0.75f, 0u, {0u, 0u, 0u}};
                                rsrt_video_planes_out pl;
                                std::vector<unsigned char> out(rsrt_video_planes((uint32_t)w, (uint32_t)h, &p, &pl));
                                bad += out.size() != (size_t)(w * h + 2 * bw * bh) * pl.sample_bytes;
                                rsrt_hdr_levels lv;
                                video_display(sums.data(), h, w, 1.0f, 1.5f, dither > 0.0f ? gain.data() : nullptr, dither > 0.0f ? 0.5f : 0.0f, b.data(), &colour, lut.data(), 3u,
                                              hdr10 ? &hp : nullptr, &p, out.data(), &lv);
                                const uint32_t m = depth == 10u ? 4u : 1u, shift = depth == 10u && layout == RSRT_VIDEO_SEMIPLANAR ? 6u : 0u;
                                const uint32_t lo = range == RSRT_VIDEO_FULL ? 0u : 16u * m, hiy = range == RSRT_VIDEO_FULL ? 256u * m - 1u : 235u * m,
                                               hic = range == RSRT_VIDEO_FULL ? 256u * m - 1u : 240u * m;
                                for (size_t i = 0; i < out.size() / pl.sample_bytes; i++) { // no code leaves its range
                                    const uint32_t word = pl.sample_bytes == 2u ? (uint32_t)out[2 * i] | (uint32_t)out[2 * i + 1] << 8 : out[i];
                                    const uint32_t code = word >> shift;
                                    bad += (code << shift) != word || code < lo || code > (i < (size_t)w * h ? hiy : hic);
                                }
                                if (hdr10) bad += !(lv.max_cll <= hp.peak_nits && lv.max_fall <= lv.max_cll);
                            }
    }
    // every threshold of both tables and its neighbours: the code stays inside [b - 0.5, b + 0.5] and never steps back
    for (int which = 0; which < 2; which++) {
        const float *t = which ? RSRT_PQ10_THRESHOLDS : RSRT_SRGB8_THRESHOLDS;
        const int n = which ? 1023 : 255;
        float last = 0.0f;
        for (int k = 0; k < n; k++)
            for (float x : {std::nextafter(t[k], 0.0f), t[k], std::nextafter(t[k], 20000.0f)}) {
                const float e = which ? rsrt_video_code_pq(x) : rsrt_video_code_srgb(x);
                const float b = (float)(x >= t[k] ? k + 1 : k);
                bad += !(e >= b - 0.5f && e <= b + 0.5f) || e < last;
                last = e;
            }
    }
    for (float x : {nan, -inf, -1.0f, -0.0f, 0.0f}) bad += rsrt_video_code_srgb(x) != 0.0f || rsrt_video_code_pq(x) != 0.0f;
    for (float x : {1.0f, 2.0f, inf}) bad += rsrt_video_code_srgb(x) != 255.0f;
    for (float x : {10000.0f, 20000.0f, inf}) bad += rsrt_video_code_pq(x) != 1023.0f;
    std::printf(bad ? "video_host: %d checks failed\n" : "video_host: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
