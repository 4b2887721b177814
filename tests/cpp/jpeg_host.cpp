// jpeg_host.cpp — include/rsrt_jpeg.h evaluated on the CPU for tests/test_jpeg.py: every step as a C function over arrays, so that the
// numpy restatement (tests/jpeg_ref.py) can be held against the header itself and not only against the library built from it.
// Built by the test with g++ -ffp-contract=off as a shared object; with -DJPEG_HOST_MAIN (and csrc/host/image_io.cpp beside it) it is a
// program of its own that runs the host encoder and the sequential coder over the tests' sizes, special values and crafted blocks, for the
// sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rsrt_host.h"
#include "rsrt_jpeg.h"

extern "C" {

void jpeg_ycc(const float *e, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) rsrt_jpeg_ycc(e + 3 * i, out + 3 * i);
}
void jpeg_samples(const float *sdr, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) rsrt_jpeg_samples(sdr + 3 * i, out + 3 * i);
}
void jpeg_fdct(const float *s, size_t n_blocks, float *c)
{
    for (size_t i = 0; i < n_blocks; i++) rsrt_jpeg_fdct(s + 64 * i, c + 64 * i);
}
void jpeg_quantise(const float *c, size_t n, uint32_t q, int dc, int32_t *out)
{
    for (size_t i = 0; i < n; i++) out[i] = rsrt_jpeg_quantise(c[i], q, dc);
}
void jpeg_quantise_block(const float *c, uint32_t chroma, uint32_t quality, int16_t *zz) { rsrt_jpeg_quantise_block(c, chroma, quality, zz); }
void jpeg_qtable(uint32_t quality, uint32_t chroma, uint8_t *out)
{
    for (uint32_t n = 0; n < 64u; n++) out[n] = (uint8_t)rsrt_jpeg_q_at(n, chroma, quality);
}
void jpeg_tables(float *dct, uint8_t *zigzag, uint32_t *dc_codes, uint32_t *ac_codes)
{
    std::memcpy(dct, RSRT_JPEG_DCT, sizeof RSRT_JPEG_DCT);
    std::memcpy(zigzag, RSRT_JPEG_ZIGZAG, sizeof RSRT_JPEG_ZIGZAG);
    std::memcpy(dc_codes, RSRT_JPEG_DC_CODE, sizeof RSRT_JPEG_DC_CODE);
    std::memcpy(ac_codes, RSRT_JPEG_AC_CODE, sizeof RSRT_JPEG_AC_CODE);
}
uint32_t jpeg_block_bits(const int16_t *zz, int pred, uint32_t chroma) { return rsrt_jpeg_block_bits(zz, pred, chroma); }
// out: 208 zeroed bytes
uint32_t jpeg_block_code(const int16_t *zz, int pred, uint32_t chroma, uint8_t *out)
{
    rsrt_jpeg_writer w = {out, 0u};
    const uint32_t n = rsrt_jpeg_block_code(&w, zz, pred, chroma);
    return n == w.n_bits ? n : 0xffffffffu;
}
int64_t jpeg_block_pred(uint64_t i, uint32_t subsampling) { return rsrt_jpeg_block_pred(i, subsampling); }
uint32_t jpeg_block_component(uint64_t i, uint32_t subsampling) { return rsrt_jpeg_block_component(i, subsampling); }
uint64_t jpeg_blocks(uint32_t w, uint32_t h, uint32_t subsampling) { return rsrt_jpeg_blocks(w, h, subsampling); }
uint64_t jpeg_max_bytes(uint32_t w, uint32_t h, uint32_t subsampling) { return rsrt_jpeg_max_bytes(w, h, subsampling); }
uint64_t jpeg_headers(uint8_t *out, uint32_t w, uint32_t h, const rsrt_jpeg_params *p) { return rsrt_jpeg_headers(out, w, h, p); }
uint64_t jpeg_stuff(const uint8_t *scan, uint64_t n_bits, uint8_t *out) { return rsrt_jpeg_stuff(scan, n_bits, out); }
int jpeg_params_ok(const rsrt_jpeg_params *p) { return rsrt_jpeg_params_ok(p); }
void jpeg_defaults(rsrt_jpeg_params *p)
{
    p->quality = RSRT_JPEG_DEFAULT_QUALITY; p->subsampling = RSRT_JPEG_DEFAULT_SUBSAMPLING; p->flags = RSRT_JPEG_DEFAULT_FLAGS; p->reserved = RSRT_JPEG_DEFAULT_RESERVED;
}
// sizeof, the offsets, then the constants
void jpeg_layout(uint32_t *out)
{
    out[0] = (uint32_t)sizeof(rsrt_jpeg_params);
    out[1] = (uint32_t)offsetof(rsrt_jpeg_params, subsampling); out[2] = (uint32_t)offsetof(rsrt_jpeg_params, flags); out[3] = (uint32_t)offsetof(rsrt_jpeg_params, reserved);
    out[4] = RSRT_JPEG_420; out[5] = RSRT_JPEG_444; out[6] = RSRT_JPEG_BLOCK_BITS; out[7] = RSRT_JPEG_HEADER_BYTES;
}

} // extern "C"

#ifdef JPEG_HOST_MAIN
namespace {

int failures = 0;
void expect(bool ok, const char *what, unsigned a = 0, unsigned b = 0, unsigned c = 0)
{
    if (!ok) {
        std::printf("jpeg_host: FAILED %s (%u %u %u)\n", what, a, b, c);
        failures++;
    }
}

// a file through the size protocol: asked with no room, then written into exactly that room
template <class Call>
std::vector<uint8_t> sized(Call call)
{
    size_t n = 0;
    expect(call(nullptr, 0, &n) == 2 && n > RSRT_JPEG_HEADER_BYTES + 2u, "the size is told");
    std::vector<uint8_t> out(n);
    size_t m = 0;
    expect(call(out.data(), n, &m) == 0 && m == n, "the file fits the size told");
    expect(out[0] == 0xff && out[1] == 0xd8 && out[n - 2] == 0xff && out[n - 1] == 0xd9, "SOI and EOI");
    return out;
}

} // namespace

int main()
{
    static const uint32_t sizes[][2] = {{1, 1}, {8, 8}, {9, 17}, {16, 16}, {17, 33}, {5, 67}, {64, 96}}; // w, h
    static const uint32_t bits[] = {0x7fc00000u, 0x7f800000u, 0xff800000u, 0x80000000u, 0xbf800000u, 0x7f7fffffu, 0x7f61b1e6u /* 3e38f */, 0x3f000000u, 0x3e000000u, 0x00000001u};
    for (const auto &wh : sizes)
        for (uint32_t sub = 0; sub < 2u; sub++)
            for (uint32_t quality : {1u, 50u, 90u, 100u}) {
                const uint32_t w = wh[0], h = wh[1];
                std::vector<float> rgb((size_t)w * h * 3);
                for (size_t i = 0; i < rgb.size(); i++) {
                    const uint32_t b = i % 5u == 0u ? bits[(i / 5u) % 10u] : 0x3c000000u + (uint32_t)((i * 2654435761u) >> 7); // specials among values up to about 1
                    std::memcpy(&rgb[i], &b, 4);
                }
                const rsrt_jpeg_params p = {quality, sub, 0u, 0u};
                const std::vector<uint8_t> file = sized([&](void *out, size_t cap, size_t *n) { return rsrt_jpeg_encode_host(rgb.data(), w, h, &p, out, cap, n); });
                expect(file.size() <= rsrt_jpeg_max_bytes(w, h, sub), "the worst case holds", w, h, quality);
                std::vector<int16_t> coefs((size_t)rsrt_jpeg_blocks(w, h, sub) * 64u);
                expect(rsrt_jpeg_coefficients_host(rgb.data(), w, h, &p, coefs.data(), coefs.size()) == 0, "coefficients", w, h, quality);
                const std::vector<uint8_t> again = sized([&](void *out, size_t cap, size_t *n) { return rsrt_jpeg_from_coefficients(coefs.data(), coefs.size(), w, h, &p, out, cap, n); });
                expect(again == file, "the coder alone gives the same file", w, h, quality);
            }
    // crafted blocks, 4:4:4 at 16 x 8 (six blocks): the worst case, a lone coefficient 63, the runs around 16 and 32, the largest differences
    for (uint32_t variant = 0; variant < 8u; variant++) {
        std::vector<int16_t> c(6u * 64u, 0);
        for (size_t b = 0; b < 6u; b++) {
            int16_t *z = c.data() + 64u * b;
            switch (variant) {
            case 0: break;
            case 1: z[63] = (int16_t)(b % 2u ? -1 : 1); break;
            case 2: for (int k = 1; k < 64; k++) z[k] = (int16_t)((k + b) % 2u ? 1023 : -1023); z[0] = (int16_t)(b % 2u ? 1023 : -1024); break;
            case 3: z[16] = 1; break;  // a run of 15
            case 4: z[17] = -1; break; // 16
            case 5: z[32] = 5; break;  // 31
            case 6: z[33] = -5; z[63] = 1; break; // 32, then 29
            default: z[0] = (int16_t)(b / 3u % 2u ? 1023 : -1024); break; // differences of -1024, 2047, -2047 a component
            }
        }
        const rsrt_jpeg_params p = {90u, RSRT_JPEG_444, 0u, 0u};
        sized([&](void *out, size_t cap, size_t *n) { return rsrt_jpeg_from_coefficients(c.data(), c.size(), 16u, 8u, &p, out, cap, n); });
        size_t n = 0;
        c[5] = 1024;
        expect(rsrt_jpeg_from_coefficients(c.data(), c.size(), 16u, 8u, &p, nullptr, 0, &n) == 1, "an AC of 1024 is refused", variant);
        c[5] = 0; c[64] = -1025;
        expect(rsrt_jpeg_from_coefficients(c.data(), c.size(), 16u, 8u, &p, nullptr, 0, &n) == 1, "a DC of -1025 is refused", variant);
    }
    if (failures == 0) std::printf("jpeg_host: ok\n");
    return failures != 0;
}
#endif
