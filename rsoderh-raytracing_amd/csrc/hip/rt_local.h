// rt_local.h — the local exposure pass's kernels, the graded display kernel and their C-ABI (include/rsrt.h "local exposure";
// DESIGN.md §17).  Included at the end of rsrt_api.hip.  All arithmetic is include/rsrt_local.h's.
//
//  rt_local_splat_kernel     the raw grid of a float4 image.  A 256-thread workgroup owns the RT_LC_PW x RT_LC_PH pixels of its block
//                            and with them whole grid columns: (RT_LC_PW / cell) x (RT_LC_PH / cell) of them, 32 cells each.  A wave
//                            reads a row of the block (16 B a lane, coalesced; RT_LC_AHEAD rows are in flight before the first is
//                            used) and counts every pixel into the workgroup's cells in LDS with ONE 64-bit integer add whose result
//                            is not used: the count in the high word, q in the low.  After one __syncthreads the workgroup writes
//                            every cell of its columns once with a plain store, zeros included — no global atomics, no memset in
//                            front of a call, no dependence on what the buffer held.  16 KB of LDS, no scratch memory.  (The meter's
//                            shortcut — lanes that share a cell add once — was measured and lost here: DESIGN.md §17.)
//  rt_local_blur_kernel      the three 1-2-1 tents in one launch, from the raw grid into the second, which is the one the slice reads: a
//                            lane a cell, 27 8-byte loads that the caches serve (one launch a tent was slower at the default cell:
//                            DESIGN.md §17).
//  rt_display_local_kernel   rt_display_exposed_kernel with the slice inside and, with intensity > 0, rt_display_bloomed_kernel's four
//  rt_local_gain_kernel      taps; the second writes the f32 gain instead of bytes.  A workgroup takes RT_LC_TW x RT_LC_TH pixels; the
//                            eight corners come through L2 (staging the tile's columns in LDS was no faster: DESIGN.md §17).
// The tiled displays — these two, rt_display_colour_kernel, rt_display_finish_kernel and rt_display_hdr_kernel — share DisplayChain, the struct they take by value,
// rt_display_gather, which reads a pixel's inputs from it, and display_chain, which makes their entry points' checks and fills it.
#include "../../../include/rsrt_jpeg.h"
#include "../../../include/rsrt_video.h" // (the whole display chain, rsrt_hdr.h and below: display_chain checks every stage's parameters)

#define RT_LC_PW 64
#define RT_LC_PH 64
#define RT_LC_BLOCK 256
#define RT_LC_AHEAD 8                 // loads in flight a lane
#define RT_LC_COLS 64                 // columns of a block at the smallest cell
#define RT_LC_TW 32
#define RT_LC_TH 8

static_assert(RT_LC_PW == RT_WAVE && RT_LC_PW % 64 == 0 && RT_LC_PH % 64 == 0, "a wave reads a row of the block, and a block holds whole columns of every cell");
static_assert(RT_LC_COLS == (RT_LC_PW / 8) * (RT_LC_PH / 8) && RT_LC_PH % (RT_LC_AHEAD * (RT_LC_BLOCK / RT_WAVE)) == 0, "");
static_assert(RT_LC_TW * RT_LC_TH == RT_LC_BLOCK, "");

// grid: gx x gy x 32 cells of (count, sum), every one of which is written; shift = log2(cell)
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_local_splat_kernel(const float4 *img, int w, int h, float total, uint32_t shift, uint2 *grid, uint32_t gx, uint32_t gy)
{
    __shared__ unsigned long long cells[RSRT_LOCAL_GZ * RT_LC_COLS]; // [z][column of the block]: count << 32 | sum
    const uint32_t tid = threadIdx.x, lx = tid % RT_LC_PW, wave = tid / RT_LC_PW;
    const uint32_t ncx = RT_LC_PW >> shift, ncy = RT_LC_PH >> shift, ncols = ncx * ncy;
    for (uint32_t i = tid; i < RSRT_LOCAL_GZ * ncols; i += RT_LC_BLOCK) cells[i] = 0ull;
    __syncthreads();
    const int x = (int)(blockIdx.x * RT_LC_PW + lx), y0 = (int)(blockIdx.y * RT_LC_PH);
    for (uint32_t trip = 0; trip < RT_LC_PH; trip += RT_LC_AHEAD * (RT_LC_BLOCK / RT_WAVE)) { // (the bounds are the workgroup's: no lane leaves early)
        float4 c[RT_LC_AHEAD];
        bool in[RT_LC_AHEAD];
#pragma unroll
        for (uint32_t k = 0; k < RT_LC_AHEAD; k++) {
            const int y = y0 + (int)(trip + k * (RT_LC_BLOCK / RT_WAVE) + wave);
            in[k] = x < w && y < h;
            if (in[k]) c[k] = img[(size_t)y * (size_t)w + (size_t)x];
        }
#pragma unroll
        for (uint32_t k = 0; k < RT_LC_AHEAD; k++) {
            const uint32_t ly = trip + k * (RT_LC_BLOCK / RT_WAVE) + wave;
            uint32_t q = RSRT_LOCAL_SKIPPED;
            if (in[k]) {
                const float sum[3] = {c[k].x, c[k].y, c[k].z};
                q = rsrt_local_q_of(sum, total);
            }
            const uint32_t at = q == RSRT_LOCAL_SKIPPED ? RSRT_LOCAL_SKIPPED : (q >> 8) * ncols + (ly >> shift) * ncx + (lx >> shift);
            if (at != RSRT_LOCAL_SKIPPED) atomicAdd(&cells[at], (1ull << 32) | q);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < RSRT_LOCAL_GZ * ncols; i += RT_LC_BLOCK) {
        const uint32_t cx = blockIdx.x * ncx + i % ncx, cy = blockIdx.y * ncy + (i / ncx) % ncy, z = i / ncols;
        if (cx >= gx || cy >= gy) continue;
        const unsigned long long v = cells[i];
        grid[rsrt_local_word(gx, gy, cx, cy, z) / 2u] = make_uint2((uint32_t)(v >> 32), (uint32_t)v);
    }
}

// dst = the tent of src along x, y and z at once, both gx x gy x 32 cells: 27 cells of src a lane, each weighted by the product of its
// three tent weights (integers: the same words as one tent after the other)
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_local_blur_kernel(const uint2 *src, uint2 *dst, uint32_t gx, uint32_t gy)
{
    const size_t i = (size_t)blockIdx.x * RT_LC_BLOCK + threadIdx.x, n = (size_t)gx * gy * RSRT_LOCAL_GZ;
    if (i >= n) return;
    const int x = (int)(i % gx), y = (int)((i / gx) % gy), z = (int)(i / ((size_t)gx * gy));
    uint2 s = make_uint2(0u, 0u);
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if (x + dx < 0 || x + dx >= (int)gx || y + dy < 0 || y + dy >= (int)gy || z + dz < 0 || z + dz >= (int)RSRT_LOCAL_GZ) continue;
                const uint2 c = src[rsrt_local_word(gx, gy, (uint32_t)(x + dx), (uint32_t)(y + dy), (uint32_t)(z + dz)) / 2u];
                const uint32_t wgt = (dx ? 1u : 2u) * (dy ? 1u : 2u) * (dz ? 1u : 2u);
                s.x += wgt * c.x;
                s.y += wgt * c.y;
            }
    dst[i] = s;
}

// what the tiled display kernels read; a piece that is not asked for is not looked at, and its fields are zero
struct DisplayChain {
    const float4 *img; // w x h sums of `total` samples
    int w, h;
    float total, exposure;
    bool graded; // the local gain: the blurred grid of img, gx x gy x 32 cells of `cell` pixels
    rsrt_local_params local;
    const uint32_t *grid;
    uint32_t gx, gy, cell;
    float intensity; // > 0: the bloom image, bw x bh
    const rsrt_bloom_texel *bloom;
    int bw, bh;
    rsrt_colour_params colour; // lut_strength > 0: the LUT of n^3 nodes
    const float4 *lut;
    uint32_t n;
};

// a pixel's inputs to the chain: the sums of (x, y), 0 <= x < w, 0 <= y < h, its gain (1 without a grade) and up(B) at it (0 without bloom).
// graded: c.graded, or true where the grade is not optional: known at compile time, the luminance's divisions are the mean's, made once
__device__ __forceinline__ void rt_display_gather(const DisplayChain &c, bool graded, int x, int y, float sum[3], float *gain, rsrt_bloom_rgb *up_b)
{
    const float4 a = c.img[(size_t)y * (size_t)c.w + (size_t)x];
    sum[0] = a.x; sum[1] = a.y; sum[2] = a.z;
    *gain = graded ? rsrt_local_gain_at(c.grid, c.gx, c.gy, c.cell, x, y, rsrt_local_q_of(sum, c.total), rsrt_local_mid(c.local.key, c.exposure), &c.local) : 1.0f;
    *up_b = c.intensity > 0.0f ? rsrt_bloom_up_at(c.bloom, c.bw, c.bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f);
}

// out: uchar4 a pixel, or (GAIN) a float
template <bool GAIN>
__device__ __forceinline__ void rt_local_display_tile(const DisplayChain &c, void *out)
{
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH;
    const int x = bx + (int)threadIdx.x % RT_LC_TW, y = by + (int)threadIdx.x / RT_LC_TW;
    if (x >= c.w || y >= c.h) return;
    const size_t i = (size_t)y * (size_t)c.w + (size_t)x;
    float sum[3], gain;
    rsrt_bloom_rgb up_b;
    rt_display_gather(c, true, x, y, sum, &gain, &up_b);
    if (GAIN) {
        static_cast<float *>(out)[i] = gain;
        return;
    }
    unsigned char rgb[3];
    rsrt_display_pixel_local(sum, c.total, c.exposure, c.intensity, up_b, gain, rgb);
    static_cast<uchar4 *>(out)[i] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_local_kernel(DisplayChain c, uchar4 *out) { rt_local_display_tile<false>(c, out); }

__global__ __launch_bounds__(RT_LC_BLOCK) void rt_local_gain_kernel(DisplayChain c, float *out) { rt_local_display_tile<true>(c, out); }

namespace {

// words of one grid of a w x h source at the smallest cell: what either half of the allocation has room for
size_t local_words_max(uint32_t w, uint32_t h) { return 2u * (size_t)rsrt_local_cells(w, 8u) * rsrt_local_cells(h, 8u) * RSRT_LOCAL_GZ; }
size_t local_words(const rsrt_context *ctx) { return 2u * (size_t)rsrt_local_cells(ctx->lc_grid.w, ctx->lc_cell) * rsrt_local_cells(ctx->lc_grid.h, ctx->lc_cell) * RSRT_LOCAL_GZ; }
// the blurred grid: the second half
uint32_t *local_blurred(const rsrt_context *ctx) { return static_cast<uint32_t *>(ctx->lc_grid.p) + local_words_max(ctx->lc_grid.w, ctx->lc_grid.h); }

// display_chain's `demands`: the params an entry point refuses as NULL (others are off when NULL); CHAIN_FLOATS: it writes a float a pixel, not
// bytes; CHAIN_HDR: it writes what hdr->encoding says, 4 or 8 bytes a pixel, and takes no LUT; CHAIN_VIDEO: it writes a frame of
// rsrt_video_planes' size, and `video` says whether hdr belongs (RSRT_VIDEO_HDR10: required, RSRT_HDR_PQ10) or not (RSRT_VIDEO_BT709: NULL);
// CHAIN_JPEG: it writes a JPEG file into n_out bytes of room, whatever their number (the file's size is the coder's to say), or with
// CHAIN_JPEG_COEFS the picture's 64 * rsrt_jpeg_blocks coefficients; `jpeg` is required and the picture must be one a file can hold
enum : uint32_t { CHAIN_LOCAL = 1u, CHAIN_COLOUR = 2u, CHAIN_FINISH = 4u, CHAIN_FLOATS = 8u, CHAIN_HDR = 16u, CHAIN_VIDEO = 32u, CHAIN_JPEG = 64u, CHAIN_JPEG_COEFS = 128u };

// Every check of the tiled displays, in the order the faults are reported in: the source, the local, colour, finish, hdr and video params, the bloom
// intensity, the output's size, then what the context has to hold where it is asked for: the grid, the bloom image, the LUT.  Fills c.
rsrt_status display_chain(rsrt_context *ctx, const char *what, uint32_t demands, uint32_t source, uint32_t sample_total, float exposure,
                          const rsrt_local_params *local, const rsrt_colour_params *colour, const rsrt_finish_params *finish, const rsrt_hdr_params *hdr,
                          float intensity, const void *host, size_t n_out, DisplayChain *c, const rsrt_video_params *video = nullptr,
                          const rsrt_jpeg_params *jpeg = nullptr)
{
    ImageView v;
    rsrt_status st = bloom_source(ctx, what, source, sample_total, exposure, &v);
    if (st) return st;
    if ((demands & CHAIN_LOCAL) && !local) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: params is NULL", what);
    if (local && !rsrt_local_params_ok(local))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want shadows and highlights in [0, 1], key finite and > 0, max_stops in [0, 16], flags 0", what);
    if ((demands & CHAIN_COLOUR) && !colour) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: colour is NULL", what);
    if (colour && !rsrt_colour_params_ok(colour)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want white finite and > 0, lut_strength in [0, 1], flags 0", what);
    if ((demands & CHAIN_FINISH) && !finish) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: finish is NULL", what);
    if (finish && !rsrt_finish_params_ok(finish))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want sharpness, grain and dither in [0, 1], flags RSRT_FINISH_NOISE_AWARE or 0", what);
    if ((demands & CHAIN_HDR) && !hdr) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: hdr is NULL", what);
    if (hdr && !rsrt_hdr_params_ok(hdr))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want paper_white_nits in [1, 10000], peak_nits from there to 10000, knee in [0, 0.95], dither in [0, 1] "
                                                     "and 0 with RSRT_HDR_SCRGB16F, encoding RSRT_HDR_PQ10 or RSRT_HDR_SCRGB16F, flags 0", what);
    if (hdr && colour && colour->lut_strength > 0.0f)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: lut_strength must be 0 (the colour LUT is display-referred SDR and does not apply to HDR output)", what);
    if (demands & CHAIN_VIDEO) {
        if (!video) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: video is NULL", what);
        if (!rsrt_video_params_ok(video))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want standard RSRT_VIDEO_BT709 or RSRT_VIDEO_HDR10, depth 8 or 10 (10 with RSRT_VIDEO_HDR10), a known layout, "
                                                         "range and siting, dither in [0, 1], flags 0", what);
        if (video->standard == RSRT_VIDEO_HDR10 ? !hdr || hdr->encoding != RSRT_HDR_PQ10 : hdr != nullptr)
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: hdr must be given with encoding RSRT_HDR_PQ10 for RSRT_VIDEO_HDR10 and be NULL for RSRT_VIDEO_BT709", what);
    }
    if (demands & CHAIN_JPEG) {
        if (!jpeg) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: jpeg is NULL", what);
        if (!rsrt_jpeg_params_ok(jpeg)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want quality in 1 .. 100, subsampling RSRT_JPEG_420 or RSRT_JPEG_444, flags 0, reserved 0", what);
    }
    if (!rsrt_bloom_finite_nonneg(intensity)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: bloom_intensity must be finite and >= 0", what);
    if (demands & CHAIN_JPEG) {
        if (!rsrt_jpeg_size_ok(v.w, v.h, jpeg->subsampling))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: a %u x %u picture is more than a JPEG file of this library holds (sides to 65535, a worst case below 2^32 bits)", what, v.w, v.h);
        const size_t values = (size_t)rsrt_jpeg_blocks(v.w, v.h, jpeg->subsampling) * 64u;
        if (!host || ((demands & CHAIN_JPEG_COEFS) && n_out != values))
            return (demands & CHAIN_JPEG_COEFS) ? fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: expected %zu values", what, values) : fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: host_out is NULL", what);
    }
    const bool floats = demands & CHAIN_FLOATS;
    const size_t want = (demands & CHAIN_VIDEO) ? rsrt_video_planes(v.w, v.h, video, nullptr) : floats ? v.pixels() : v.pixels() * (hdr && hdr->encoding == RSRT_HDR_SCRGB16F ? 8 : 4);
    if (!(demands & CHAIN_JPEG) && (!host || n_out != want)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: expected %zu %s", what, want, floats ? "floats" : "bytes");
    *c = DisplayChain{}; // (what is not asked for stays zero)
    c->img = v.img; c->w = (int)v.w; c->h = (int)v.h; c->total = v.total; c->exposure = exposure;
    if (local) {
        if (!ctx->lc_have) return fail(ctx, RSRT_ERR_NOT_READY, "no local exposure grid (rsrt_local_exposure first)");
        if ((st = built_for(ctx, what, "grid", ctx->lc_grid, v))) return st;
        c->graded = true;
        c->local = *local;
        c->grid = local_blurred(ctx);
        c->cell = ctx->lc_cell;
        c->gx = rsrt_local_cells(v.w, c->cell); c->gy = rsrt_local_cells(v.h, c->cell);
    }
    c->intensity = intensity;
    if (intensity > 0.0f) {
        if ((st = bloom_ready(ctx, what, v))) return st;
        c->bloom = static_cast<const rsrt_bloom_texel *>(ctx->bl_pyr.p);
        c->bw = (int)rsrt_bloom_level_size(v.w, 1); c->bh = (int)rsrt_bloom_level_size(v.h, 1);
    }
    c->colour = colour ? *colour : rsrt_colour_params{{1.0f, 1.0f, 1.0f}, 0.0f, 0u, {0u, 0u, 0u}};
    if (c->colour.lut_strength > 0.0f) {
        if (!ctx->cl_n) return fail(ctx, RSRT_ERR_NOT_READY, "no colour LUT (rsrt_colour_lut_build or rsrt_colour_lut_upload first)");
        c->lut = ctx->cl_lut;
        c->n = ctx->cl_n;
    }
    return RSRT_OK;
}

dim3 display_tiles(const DisplayChain &c) { return dim3(((uint32_t)c.w + RT_LC_TW - 1u) / RT_LC_TW, ((uint32_t)c.h + RT_LC_TH - 1u) / RT_LC_TH); }

} // namespace

extern "C" {

rsrt_status rsrt_local_exposure(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t cell, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ImageView v;
    rsrt_status st = exposure_source(ctx, "local_exposure", source, sample_total, &v);
    if (st) return st;
    if (!rsrt_local_cell_ok(cell)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "local_exposure: cell must be 8, 16, 32 or 64");
    if (v.w > 0x3fffffffu || v.h > 0x3fffffffu) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "local_exposure: source too large");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const size_t px = v.pixels();
    if (!ctx->lc_grid.is(v.w, v.h)) ctx->lc_have = false; // (the allocation that held the grid goes)
    if ((st = ensure_sized(ctx, ctx->lc_grid, v.w, v.h, (2u * local_words_max(v.w, v.h) * sizeof(uint32_t) + px - 1u) / px))) return st;
    if ((st = begin_work(ctx, stream))) return st;
    ctx->lc_have = false; // (a failed launch leaves no grid)
    const uint32_t gx = rsrt_local_cells(v.w, cell), gy = rsrt_local_cells(v.h, cell), shift = cell == 8u ? 3u : (cell == 16u ? 4u : (cell == 32u ? 5u : 6u));
    uint2 *const raw = static_cast<uint2 *>(ctx->lc_grid.p), *const blurred = raw + local_words_max(v.w, v.h) / 2u;
    const unsigned blocks = (unsigned)(((size_t)gx * gy * RSRT_LOCAL_GZ + RT_LC_BLOCK - 1u) / RT_LC_BLOCK);
    rt_local_splat_kernel<<<dim3((v.w + RT_LC_PW - 1u) / RT_LC_PW, (v.h + RT_LC_PH - 1u) / RT_LC_PH), dim3(RT_LC_BLOCK), 0, stream>>>(v.img, (int)v.w, (int)v.h, v.total,
                                                                                                                                   shift, raw, gx, gy);
    rt_local_blur_kernel<<<dim3(blocks), dim3(RT_LC_BLOCK), 0, stream>>>(raw, blurred, gx, gy);
    HIP_TRY(ctx, hipGetLastError());
    ctx->lc_cell = cell;
    ctx->lc_have = true;
    return end_work(ctx, stream);
}

rsrt_status rsrt_local_exposure_download(rsrt_context *ctx, uint32_t *host_words, size_t n_words, uint32_t dims_out[4])
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "local_exposure_download"); if (st0) return st0; }
    if (!ctx->lc_have) return fail(ctx, RSRT_ERR_NOT_READY, "no local exposure grid (rsrt_local_exposure first)");
    const size_t n = local_words(ctx);
    if (host_words || n_words) {
        if (!host_words || n_words != n) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "local_exposure_download: expected %zu words", n);
        { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
        HIP_TRY(ctx, hipMemcpy(host_words, local_blurred(ctx), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (dims_out) {
        dims_out[0] = rsrt_local_cells(ctx->lc_grid.w, ctx->lc_cell);
        dims_out[1] = rsrt_local_cells(ctx->lc_grid.h, ctx->lc_cell);
        dims_out[2] = RSRT_LOCAL_GZ;
        dims_out[3] = ctx->lc_cell;
    }
    return RSRT_OK;
}

rsrt_status rsrt_local_exposure_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "local_exposure_reset"); if (st0) return st0; }
    ctx->lc_have = false;
    return RSRT_OK;
}

rsrt_status rsrt_local_gain_download(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params, float *host_gain,
                                     size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!host_gain) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "local_gain_download: host_gain is NULL");
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "local_gain_download", CHAIN_LOCAL | CHAIN_FLOATS, source, sample_total, exposure, params, nullptr, nullptr, nullptr, 0.0f, host_gain,
                                         n_floats, &c);
    if (st) return st;
    return read_back(ctx, host_gain, n_floats * sizeof(float), 0, [&](void *tmp) {
        rt_local_gain_kernel<<<display_tiles(c), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, static_cast<float *>(tmp));
        return RSRT_OK;
    });
}

rsrt_status rsrt_display_local_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params,
                                     float bloom_intensity, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "display_local_srgb8", CHAIN_LOCAL, source, sample_total, exposure, params, nullptr, nullptr, nullptr, bloom_intensity, host_rgba8,
                                         n_bytes, &c);
    if (st) return st;
    return read_back(ctx, host_rgba8, n_bytes, 0, [&](void *tmp) {
        rt_display_local_kernel<<<display_tiles(c), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
