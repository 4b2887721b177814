// image_io.cpp — Radiance .hdr reader, PNG / PFM writers, camera state string, CPU display transform.
//
//  rsrt_load_hdr           what `image::load_from_memory(..).into_rgb32f()` gives the reference for its
//                          HDRIs (src/state.rs:119-132; image 0.25 `hdr` decoder, un-vendored): RGBE,
//                          value = mantissa * 2^(e - 136), all zero when e == 0, rows top to bottom,
//                          new-style per-channel RLE and flat scanlines.
//  rsrt_camera_serialize / rsrt_camera_deserialize
//                          Camera::serialize / deserialize (src/camera.rs:30-89): 24 little-endian bytes
//                          [pos.xyz, yaw, pitch, fov_y] as standard base64 (the --state flag, src/cli.rs:39-43).
//  rsrt_write_png / rsrt_write_pfm
//                          image output (the reference only presents to a window).
//  rsrt_y4m_write          video output: rsrt_display_video's planar frames as a YUV4MPEG2 sequence.
//  rsrt_jpeg_encode_host / rsrt_jpeg_from_coefficients / rsrt_avi_mjpeg_write
//                          JPEG output: include/rsrt_jpeg.h on the CPU, sequential (the device's reference), and JPEG files
//                          as one Motion-JPEG RIFF AVI.
//  rsrt_display_srgb8_host the display transform of include/rsrt_tonemap.h on the CPU, for hosts that
//                          downloaded the f32 sums.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/rsrt_host.h"
#include "../../../include/rsrt_jpeg.h"
#include "../../../include/rsrt_video.h"
#include "../../../include/rsrt_tonemap.h"

namespace {

void set_err(char *err, size_t n, const std::string &m)
{
    if (err && n) std::snprintf(err, n, "%s", m.c_str());
}

bool read_all(const char *path, std::vector<unsigned char> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

// ---- PNG: stored (uncompressed) deflate blocks
uint32_t crc_table[256];
bool crc_ready = false;
void crc_init()
{
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        crc_table[n] = c;
    }
    crc_ready = true;
}
uint32_t crc32(uint32_t crc, const unsigned char *p, size_t n)
{
    if (!crc_ready) crc_init();
    crc ^= 0xffffffffu;
    for (size_t i = 0; i < n; i++) crc = crc_table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return crc ^ 0xffffffffu;
}
void put32(std::vector<unsigned char> &v, uint32_t x)
{
    v.push_back((unsigned char)(x >> 24)); v.push_back((unsigned char)(x >> 16)); v.push_back((unsigned char)(x >> 8)); v.push_back((unsigned char)x);
}
void chunk(std::vector<unsigned char> &png, const char *type, const std::vector<unsigned char> &data)
{
    put32(png, (uint32_t)data.size());
    size_t start = png.size();
    png.insert(png.end(), type, type + 4);
    png.insert(png.end(), data.begin(), data.end());
    put32(png, crc32(0, png.data() + start, png.size() - start));
}

const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

} // namespace

extern "C" {

int rsrt_load_hdr(const char *path, uint32_t *width, uint32_t *height, float **rgb_out, char *err, size_t err_len)
{
    if (!path || !width || !height || !rgb_out) { set_err(err, err_len, "null argument"); return 1; }
    *rgb_out = nullptr;
    std::vector<unsigned char> d;
    if (!read_all(path, d)) { set_err(err, err_len, std::string("cannot open ") + path); return 2; }
    size_t p = 0;
    auto line = [&](std::string &out) -> bool {
        out.clear();
        while (p < d.size() && d[p] != '\n') out += (char)d[p++];
        if (p >= d.size()) return false;
        p++;
        return true;
    };
    std::string l;
    if (!line(l) || (l.rfind("#?RADIANCE", 0) != 0 && l.rfind("#?RGBE", 0) != 0)) { set_err(err, err_len, "not a Radiance HDR file"); return 3; }
    bool format_ok = false;
    for (;;) {
        if (!line(l)) { set_err(err, err_len, "truncated header"); return 3; }
        if (l.empty()) break;
        if (l.rfind("FORMAT=", 0) == 0) format_ok = (l == "FORMAT=32-bit_rle_rgbe");
    }
    if (!format_ok) { set_err(err, err_len, "unsupported FORMAT (need 32-bit_rle_rgbe)"); return 3; }
    if (!line(l)) { set_err(err, err_len, "missing resolution line"); return 3; }
    int h = 0, w = 0;
    if (std::sscanf(l.c_str(), "-Y %d +X %d", &h, &w) != 2 || w <= 0 || h <= 0) { set_err(err, err_len, "unsupported orientation '" + l + "' (need -Y h +X w)"); return 3; }
    float *rgb = (float *)std::malloc((size_t)w * h * 3 * sizeof(float));
    if (!rgb) { set_err(err, err_len, "out of memory"); return 4; }
    std::vector<unsigned char> scan((size_t)w * 4);
    for (int y = 0; y < h; y++) {
        bool rle = false;
        if (w >= 8 && w < 32768 && p + 4 <= d.size() && d[p] == 2 && d[p + 1] == 2 && ((d[p + 2] << 8) | d[p + 3]) == w) rle = true;
        if (rle) {
            p += 4;
            for (int c = 0; c < 4; c++) {
                int x = 0;
                while (x < w) {
                    if (p >= d.size()) { std::free(rgb); set_err(err, err_len, "truncated RLE data"); return 3; }
                    int n = d[p++];
                    if (n > 128) { // run
                        n -= 128;
                        if (p >= d.size() || x + n > w) { std::free(rgb); set_err(err, err_len, "bad RLE run"); return 3; }
                        unsigned char v = d[p++];
                        for (int k = 0; k < n; k++) scan[(size_t)(x++) * 4 + c] = v;
                    } else { // literal
                        if (n == 0 || p + n > d.size() || x + n > w) { std::free(rgb); set_err(err, err_len, "bad RLE literal"); return 3; }
                        for (int k = 0; k < n; k++) scan[(size_t)(x++) * 4 + c] = d[p++];
                    }
                }
            }
        } else {
            if (p + (size_t)w * 4 > d.size()) { std::free(rgb); set_err(err, err_len, "truncated pixel data"); return 3; }
            std::memcpy(scan.data(), d.data() + p, (size_t)w * 4);
            p += (size_t)w * 4;
        }
        for (int x = 0; x < w; x++) {
            const unsigned char *q = &scan[(size_t)x * 4];
            float *o = rgb + ((size_t)y * w + x) * 3;
            if (q[3] == 0) { o[0] = o[1] = o[2] = 0.0f; }
            else {
                const float scale = std::ldexp(1.0f, (int)q[3] - 136); // exp2(e - 128 - 8)
                o[0] = (float)q[0] * scale; o[1] = (float)q[1] * scale; o[2] = (float)q[2] * scale;
            }
        }
    }
    *width = (uint32_t)w;
    *height = (uint32_t)h;
    *rgb_out = rgb;
    return 0;
}

void rsrt_free(void *p) { std::free(p); }

int rsrt_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgba8)
{
    if (!path || !rgba8 || width == 0 || height == 0) return 1;
    std::vector<unsigned char> raw;
    raw.reserve((size_t)height * (1 + (size_t)width * 4));
    for (uint32_t y = 0; y < height; y++) {
        raw.push_back(0); // filter: none
        raw.insert(raw.end(), rgba8 + (size_t)y * width * 4, rgba8 + (size_t)(y + 1) * width * 4);
    }
    std::vector<unsigned char> z = {0x78, 0x01}; // zlib header, no compression
    uint32_t a = 1, b = 0; // adler32
    for (size_t i = 0; i < raw.size(); i++) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
    size_t pos = 0;
    while (pos < raw.size()) {
        const size_t n = std::min<size_t>(65535, raw.size() - pos);
        z.push_back(pos + n == raw.size() ? 1 : 0);
        z.push_back((unsigned char)(n & 0xff)); z.push_back((unsigned char)(n >> 8));
        z.push_back((unsigned char)(~n & 0xff)); z.push_back((unsigned char)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
        pos += n;
    }
    put32(z, (b << 16) | a);
    std::vector<unsigned char> png = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<unsigned char> ihdr;
    put32(ihdr, width); put32(ihdr, height);
    ihdr.push_back(8); ihdr.push_back(6); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0); // 8-bit RGBA
    chunk(png, "IHDR", ihdr);
    chunk(png, "IDAT", z);
    chunk(png, "IEND", {});
    FILE *f = std::fopen(path, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(png.data(), 1, png.size(), f) == png.size();
    std::fclose(f);
    return ok ? 0 : 3;
}

// PFM "PF": rows bottom to top, little-endian (scale -1.0)
int rsrt_write_pfm(const char *path, uint32_t width, uint32_t height, const float *rgb, uint32_t stride_floats)
{
    if (!path || !rgb || width == 0 || height == 0 || stride_floats < 3) return 1;
    FILE *f = std::fopen(path, "wb");
    if (!f) return 2;
    std::fprintf(f, "PF\n%u %u\n-1.0\n", width, height);
    std::vector<float> row((size_t)width * 3);
    for (uint32_t y = height; y-- > 0;) {
        for (uint32_t x = 0; x < width; x++)
            for (int c = 0; c < 3; c++) row[(size_t)x * 3 + c] = rgb[((size_t)y * width + x) * stride_floats + c];
        if (std::fwrite(row.data(), sizeof(float), row.size(), f) != row.size()) { std::fclose(f); return 3; }
    }
    std::fclose(f);
    return 0;
}

// YUV4MPEG2: a text header line, then "FRAME\n" and the Y, Cb, Cr planes of every frame, rows tightly packed, 10-bit samples as
// little-endian uint16 with the code in the low bits: the very bytes of a RSRT_VIDEO_PLANAR frame
int rsrt_y4m_write(const char *path, int append, uint32_t width, uint32_t height, uint32_t fps_num, uint32_t fps_den, const rsrt_video_params *video,
                   const void *planar_frame, size_t n_bytes)
{
    if (!path || !video || !planar_frame || fps_num == 0 || fps_den == 0 || !rsrt_video_params_ok(video) || video->layout != RSRT_VIDEO_PLANAR) return 1;
    const size_t want = rsrt_video_planes(width, height, video, nullptr);
    if (want == 0 || n_bytes != want) return 1;
    FILE *f = std::fopen(path, append ? "r+b" : "wb"); // ("r+b": an append to a file that is not there fails instead of writing frames without a header)
    if (!f) return 2;
    bool ok = !append || std::fseek(f, 0, SEEK_END) == 0;
    if (ok && !append) {
        static const char *const sitings[] = {"LEFT", "CENTRE", "TOPLEFT"};
        const char *const tag = video->depth == 10u ? "420p10" : (video->siting == RSRT_VIDEO_SITING_CENTRE ? "420jpeg" : "420mpeg2");
        ok = std::fprintf(f, "YUV4MPEG2 W%u H%u F%u:%u Ip A1:1 C%s XCOLORRANGE=%s XRSRT_SITING=%s XRSRT_STANDARD=%s\n", width, height, fps_num, fps_den, tag,
                          video->range == RSRT_VIDEO_FULL ? "FULL" : "LIMITED", sitings[video->siting], video->standard == RSRT_VIDEO_HDR10 ? "HDR10" : "BT709") > 0;
    }
    ok = ok && std::fputs("FRAME\n", f) >= 0 && std::fwrite(planar_frame, 1, n_bytes, f) == n_bytes;
    return (std::fclose(f) == 0 && ok) ? 0 : 3;
}

// include/rsrt_jpeg.h steps 1 to 5 over a picture: the quantised coefficients of every block in scan order
static void jpeg_coefficients(const float *sdr_rgb, uint32_t w, uint32_t h, const rsrt_jpeg_params *p, std::vector<int16_t> &coefs)
{
    const bool sub = p->subsampling == RSRT_JPEG_420;
    const uint32_t side = rsrt_jpeg_mcu_side(p->subsampling), mw = rsrt_jpeg_mcus(w, p->subsampling), mh = rsrt_jpeg_mcus(h, p->subsampling);
    coefs.assign((size_t)rsrt_jpeg_blocks(w, h, p->subsampling) * 64u, 0);
    std::vector<float> s((size_t)3 * side * side); // the MCU's samples, three planes of side x side, pixels clamped to the picture
    float blk[64], c[64];
    int16_t *out = coefs.data();
    for (uint32_t my = 0; my < mh; my++)
        for (uint32_t mx = 0; mx < mw; mx++) {
            for (uint32_t y = 0; y < side; y++)
                for (uint32_t x = 0; x < side; x++) {
                    const uint32_t px = mx * side + x < w ? mx * side + x : w - 1u, py = my * side + y < h ? my * side + y : h - 1u;
                    float v[3];
                    rsrt_jpeg_samples(sdr_rgb + ((size_t)py * w + px) * 3u, v);
                    for (int k = 0; k < 3; k++) s[((size_t)k * side + y) * side + x] = v[k];
                }
            for (uint32_t b = 0; b < (sub ? 4u : 1u); b++, out += 64) { // Y00 Y01 Y10 Y11, or Y
                for (uint32_t y = 0; y < 8u; y++)
                    for (uint32_t x = 0; x < 8u; x++) blk[y * 8u + x] = s[((b / 2u) * 8u + y) * side + (b % 2u) * 8u + x];
                rsrt_jpeg_fdct(blk, c);
                rsrt_jpeg_quantise_block(c, 0u, p->quality, out);
            }
            for (uint32_t k = 1; k < 3u; k++, out += 64) { // Cb, Cr
                const float *const pl = s.data() + (size_t)k * side * side;
                for (uint32_t y = 0; y < 8u; y++)
                    for (uint32_t x = 0; x < 8u; x++)
                        blk[y * 8u + x] = sub ? rsrt_video_centre(pl[2u * y * side + 2u * x], pl[2u * y * side + 2u * x + 1u], pl[(2u * y + 1u) * side + 2u * x], pl[(2u * y + 1u) * side + 2u * x + 1u])
                                              : pl[y * side + x];
                rsrt_jpeg_fdct(blk, c);
                rsrt_jpeg_quantise_block(c, 1u, p->quality, out);
            }
        }
}

int rsrt_jpeg_from_coefficients(const int16_t *coefs, size_t n_values, uint32_t width, uint32_t height, const rsrt_jpeg_params *jpeg, void *out, size_t capacity,
                                size_t *n_bytes_out)
{
    if (!coefs || !jpeg || !n_bytes_out || (!out && capacity) || !rsrt_jpeg_params_ok(jpeg) || !rsrt_jpeg_size_ok(width, height, jpeg->subsampling)) return 1;
    const uint64_t n_blocks = rsrt_jpeg_blocks(width, height, jpeg->subsampling);
    if (n_values != n_blocks * 64u) return 1;
    for (size_t i = 0; i < n_values; i++)
        if (!rsrt_jpeg_value_ok(coefs[i], i % 64u == 0u)) return 1;
    std::vector<uint8_t> scan((size_t)n_blocks * (RSRT_JPEG_BLOCK_BITS / 8u) + 1u, 0);
    rsrt_jpeg_writer wr = {scan.data(), 0u};
    for (uint64_t i = 0; i < n_blocks; i++) {
        const int64_t pi = rsrt_jpeg_block_pred(i, jpeg->subsampling);
        rsrt_jpeg_block_code(&wr, coefs + i * 64u, pi < 0 ? 0 : coefs[pi * 64], rsrt_jpeg_block_component(i, jpeg->subsampling) ? 1u : 0u);
    }
    *n_bytes_out = rsrt_jpeg_file(scan.data(), wr.n_bits, width, height, jpeg, static_cast<uint8_t *>(out), capacity);
    return *n_bytes_out <= capacity && out ? 0 : 2;
}

int rsrt_jpeg_encode_host(const float *sdr_rgb, uint32_t width, uint32_t height, const rsrt_jpeg_params *jpeg, void *out, size_t capacity, size_t *n_bytes_out)
{
    if (!sdr_rgb || !jpeg || !n_bytes_out || (!out && capacity) || !rsrt_jpeg_params_ok(jpeg) || !rsrt_jpeg_size_ok(width, height, jpeg->subsampling)) return 1;
    std::vector<int16_t> coefs;
    jpeg_coefficients(sdr_rgb, width, height, jpeg, coefs);
    return rsrt_jpeg_from_coefficients(coefs.data(), coefs.size(), width, height, jpeg, out, capacity, n_bytes_out);
}

int rsrt_jpeg_coefficients_host(const float *sdr_rgb, uint32_t width, uint32_t height, const rsrt_jpeg_params *jpeg, int16_t *coefs_out, size_t n_values)
{
    if (!sdr_rgb || !jpeg || !coefs_out || !rsrt_jpeg_params_ok(jpeg) || !rsrt_jpeg_size_ok(width, height, jpeg->subsampling)) return 1;
    if (n_values != rsrt_jpeg_blocks(width, height, jpeg->subsampling) * 64u) return 1;
    std::vector<int16_t> coefs;
    jpeg_coefficients(sdr_rgb, width, height, jpeg, coefs);
    std::memcpy(coefs_out, coefs.data(), n_values * sizeof(int16_t));
    return 0;
}

// RIFF AVI 1.0: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh, strf } }, LIST movi { 00dc .. }, idx1 }, every number little-endian
int rsrt_avi_mjpeg_write(const char *path, const void *const *frames, const size_t *sizes, size_t n_frames, uint32_t width, uint32_t height, uint32_t fps_num,
                         uint32_t fps_den)
{
    if (!path || !frames || !sizes || n_frames == 0 || width == 0 || height == 0 || fps_num == 0 || fps_den == 0) return 1;
    uint64_t movi = 4u, largest = 0u; // 'movi', then the chunks
    for (size_t i = 0; i < n_frames; i++) {
        if (!frames[i] || sizes[i] == 0) return 1;
        movi += 8u + sizes[i] + (sizes[i] & 1u);
        largest = sizes[i] > largest ? sizes[i] : largest;
        if (movi >= (1ull << 31)) return 1;
    }
    const uint64_t hdrl = 4u + (8u + 56u) + (8u + 4u + (8u + 56u) + (8u + 40u)), idx1 = 16u * (uint64_t)n_frames;
    const uint64_t riff = 4u + (8u + hdrl) + (8u + movi) + (8u + idx1);
    if (riff + 8u >= (1ull << 31)) return 1;
    std::vector<uint8_t> h;
    const auto u32 = [&h](uint64_t v) { for (int k = 0; k < 4; k++) h.push_back((uint8_t)(v >> (8 * k))); };
    const auto u16 = [&h](uint32_t v) { h.push_back((uint8_t)v); h.push_back((uint8_t)(v >> 8)); };
    const auto tag = [&h](const char *t) { h.insert(h.end(), t, t + 4); };
    tag("RIFF"); u32(riff); tag("AVI ");
    tag("LIST"); u32(hdrl); tag("hdrl");
    tag("avih"); u32(56u);
    u32((uint64_t)fps_den * 1000000ull / fps_num);                                              // dwMicroSecPerFrame
    u32((largest * (uint64_t)fps_num + fps_den - 1u) / fps_den > 0xffffffffull ? 0xffffffffull : (largest * (uint64_t)fps_num + fps_den - 1u) / fps_den); // dwMaxBytesPerSec
    u32(0u); u32(0x10u);                                                                        // dwPaddingGranularity, dwFlags = AVIF_HASINDEX
    u32(n_frames); u32(0u); u32(1u); u32(largest); u32(width); u32(height);                     // frames, initial frames, streams, buffer, size
    u32(0u); u32(0u); u32(0u); u32(0u);                                                         // reserved
    tag("LIST"); u32(4u + (8u + 56u) + (8u + 40u)); tag("strl");
    tag("strh"); u32(56u); tag("vids"); tag("MJPG");
    u32(0u); u16(0u); u16(0u); u32(0u);                                                         // flags, priority, language, initial frames
    u32(fps_den); u32(fps_num); u32(0u); u32(n_frames); u32(largest); u32(0xffffffffu); u32(0u); // scale, rate, start, length, buffer, quality, sample size
    u16(0u); u16(0u); u16(width > 0xffffu ? 0xffffu : width); u16(height > 0xffffu ? 0xffffu : height); // rcFrame
    tag("strf"); u32(40u);
    u32(40u); u32(width); u32(height); u16(1u); u16(24u); tag("MJPG"); u32((uint64_t)width * height * 3u > 0xffffffffull ? 0xffffffffull : (uint64_t)width * height * 3u);
    u32(0u); u32(0u); u32(0u); u32(0u);                                                         // pels per metre x, y, colours used, important
    tag("LIST"); u32(movi); tag("movi");
    FILE *f = std::fopen(path, "wb");
    if (!f) return 2;
    bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
    h.clear(); // (the index is built here next and written last)
    uint64_t at = 4u; // a chunk's offset from 'movi'
    for (size_t i = 0; ok && i < n_frames; i++) {
        uint8_t head[8] = {'0', '0', 'd', 'c', (uint8_t)sizes[i], (uint8_t)(sizes[i] >> 8), (uint8_t)(sizes[i] >> 16), (uint8_t)(sizes[i] >> 24)};
        ok = std::fwrite(head, 1, 8, f) == 8 && std::fwrite(frames[i], 1, sizes[i], f) == sizes[i] && (!(sizes[i] & 1u) || std::fputc(0, f) == 0);
        tag("00dc"); u32(0x10u); u32(at); u32(sizes[i]); // AVIIF_KEYFRAME
        at += 8u + sizes[i] + (sizes[i] & 1u);
    }
    const uint8_t ih[8] = {'i', 'd', 'x', '1', (uint8_t)idx1, (uint8_t)(idx1 >> 8), (uint8_t)(idx1 >> 16), (uint8_t)(idx1 >> 24)};
    ok = ok && std::fwrite(ih, 1, 8, f) == 8 && std::fwrite(h.data(), 1, h.size(), f) == h.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 3;
}

void rsrt_display_srgb8_host(const float *sum_rgba, size_t n_pixels, uint32_t sample_total, uint8_t *out_rgba8)
{
    for (size_t i = 0; i < n_pixels; i++) {
        unsigned char rgb[3];
        rsrt_display_pixel(sum_rgba + 4 * i, (float)sample_total, rgb);
        out_rgba8[4 * i] = rgb[0]; out_rgba8[4 * i + 1] = rgb[1]; out_rgba8[4 * i + 2] = rgb[2]; out_rgba8[4 * i + 3] = 255;
    }
}

void rsrt_camera_serialize(const rsrt_camera_desc *cam, char out[33])
{
    unsigned char raw[24];
    std::memcpy(raw, cam, 24); // pos.xyz, yaw, pitch, fov_y — little-endian f32, as bytemuck writes them
    for (int i = 0; i < 8; i++) {
        const uint32_t v = (raw[3 * i] << 16) | (raw[3 * i + 1] << 8) | raw[3 * i + 2];
        out[4 * i] = B64[v >> 18]; out[4 * i + 1] = B64[(v >> 12) & 63]; out[4 * i + 2] = B64[(v >> 6) & 63]; out[4 * i + 3] = B64[v & 63];
    }
    out[32] = 0;
}

int rsrt_camera_deserialize(const char *encoded, rsrt_camera_desc *out, char *err, size_t err_len)
{
    if (!encoded || !out) { set_err(err, err_len, "null argument"); return 1; }
    std::vector<unsigned char> raw;
    uint32_t acc = 0;
    int bits = 0;
    size_t n = std::strlen(encoded), pad = 0;
    if (n % 4 != 0) { set_err(err, err_len, "Invalid padding"); return 2; } // base64 STANDARD engine requires padding
    for (size_t i = 0; i < n; i++) {
        const char c = encoded[i];
        if (c == '=') { pad++; if (i + 2 < n) { set_err(err, err_len, "Invalid byte 61, offset " + std::to_string(i) + "."); return 2; } continue; }
        const char *q = std::strchr(B64, c);
        if (!q || pad) { set_err(err, err_len, "Invalid byte " + std::to_string((int)(unsigned char)c) + ", offset " + std::to_string(i) + "."); return 2; }
        acc = (acc << 6) | (uint32_t)(q - B64);
        bits += 6;
        if (bits >= 8) { bits -= 8; raw.push_back((unsigned char)((acc >> bits) & 0xff)); }
    }
    if (raw.size() != 24) { // src/camera.rs:55-60
        set_err(err, err_len, "Couldn't deserialize camera: binary data (" + std::to_string(raw.size()) + " bytes) not 24 bytes");
        return 3;
    }
    std::memcpy(out, raw.data(), 24);
    return 0;
}

} // extern "C"
