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
#include "../../../include/rsrt_local.h"

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

// img: w x h sums; grid: the blurred grid of it; b: bw x bh, looked at only with intensity > 0; out: uchar4 a pixel, or (GAIN) a float
template <bool GAIN>
__device__ __forceinline__ void rt_local_display_tile(const float4 *img, int w, int h, float total, float exposure, rsrt_local_params p, const uint32_t *grid,
                                                      uint32_t gx, uint32_t gy, uint32_t cell, float intensity, const rsrt_bloom_texel *b, int bw, int bh, void *out)
{
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH;
    const int x = bx + (int)threadIdx.x % RT_LC_TW, y = by + (int)threadIdx.x / RT_LC_TW;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    const float4 a = img[i];
    const float sum[3] = {a.x, a.y, a.z};
    const float gain = rsrt_local_gain_at(grid, gx, gy, cell, x, y, rsrt_local_q_of(sum, total), rsrt_local_mid(p.key, exposure), &p);
    if (GAIN) {
        static_cast<float *>(out)[i] = gain;
        return;
    }
    unsigned char rgb[3];
    rsrt_display_pixel_local(sum, total, exposure, intensity, intensity > 0.0f ? rsrt_bloom_up_at(b, bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f), gain, rgb);
    static_cast<uchar4 *>(out)[i] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_local_kernel(const float4 *img, int w, int h, float total, float exposure, rsrt_local_params p,
                                                                       const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, float intensity,
                                                                       const rsrt_bloom_texel *b, int bw, int bh, uchar4 *out)
{
    rt_local_display_tile<false>(img, w, h, total, exposure, p, grid, gx, gy, cell, intensity, b, bw, bh, out);
}

__global__ __launch_bounds__(RT_LC_BLOCK) void rt_local_gain_kernel(const float4 *img, int w, int h, float total, float exposure, rsrt_local_params p,
                                                                    const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, float *out)
{
    rt_local_display_tile<true>(img, w, h, total, exposure, p, grid, gx, gy, cell, 0.0f, nullptr, 0, 0, out);
}

namespace {

// words of one grid of a w x h source at the smallest cell: what either half of the allocation has room for
size_t local_words_max(uint32_t w, uint32_t h) { return 2u * (size_t)rsrt_local_cells(w, 8u) * rsrt_local_cells(h, 8u) * RSRT_LOCAL_GZ; }
size_t local_words(const rsrt_context *ctx) { return 2u * (size_t)rsrt_local_cells(ctx->lc_grid.w, ctx->lc_cell) * rsrt_local_cells(ctx->lc_grid.h, ctx->lc_cell) * RSRT_LOCAL_GZ; }
// the blurred grid: the second half
uint32_t *local_blurred(const rsrt_context *ctx) { return static_cast<uint32_t *>(ctx->lc_grid.p) + local_words_max(ctx->lc_grid.w, ctx->lc_grid.h); }

// rsrt_display_local_srgb8 (host_gain NULL) and rsrt_local_gain_download (host_rgba8 NULL)
rsrt_status local_display(rsrt_context *ctx, const char *what, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params,
                          float intensity, uint8_t *host_rgba8, float *host_gain, size_t n_out)
{
    ImageView v;
    rsrt_status st = bloom_source(ctx, what, source, sample_total, exposure, &v);
    if (st) return st;
    const size_t n = v.pixels();
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: params is NULL", what);
    if (!rsrt_local_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want shadows and highlights in [0, 1], key finite and > 0, max_stops in [0, 16], flags 0", what);
    if (!rsrt_bloom_finite_nonneg(intensity)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: bloom_intensity must be finite and >= 0", what);
    if (host_gain ? n_out != n : (!host_rgba8 || n_out != n * 4))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: expected %zu %s", what, host_gain ? n : n * 4, host_gain ? "floats" : "bytes");
    if (!ctx->lc_have) return fail(ctx, RSRT_ERR_NOT_READY, "no local exposure grid (rsrt_local_exposure first)");
    if (!ctx->lc_grid.is(v.w, v.h))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the grid was built for %ux%u, the source is %ux%u", what, ctx->lc_grid.w, ctx->lc_grid.h, v.w, v.h);
    if (intensity > 0.0f) {
        if (!ctx->bl_have) return fail(ctx, RSRT_ERR_NOT_READY, "no bloom image (rsrt_bloom first)");
        if (!ctx->bl_pyr.is(v.w, v.h))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the bloom image was built for %ux%u, the source is %ux%u", what, ctx->bl_pyr.w, ctx->bl_pyr.h, v.w, v.h);
    }
    const uint32_t cell = ctx->lc_cell, gx = rsrt_local_cells(v.w, cell), gy = rsrt_local_cells(v.h, cell);
    const dim3 tiles((v.w + RT_LC_TW - 1u) / RT_LC_TW, (v.h + RT_LC_TH - 1u) / RT_LC_TH);
    return read_back(ctx, host_gain ? static_cast<void *>(host_gain) : host_rgba8, n * 4u, 0, [&](void *tmp) {
        if (host_gain)
            rt_local_gain_kernel<<<tiles, dim3(RT_LC_BLOCK), 0, ctx->stream>>>(v.img, (int)v.w, (int)v.h, v.total, exposure, *params, local_blurred(ctx), gx, gy, cell,
                                                                              static_cast<float *>(tmp));
        else
            rt_display_local_kernel<<<tiles, dim3(RT_LC_BLOCK), 0, ctx->stream>>>(v.img, (int)v.w, (int)v.h, v.total, exposure, *params, local_blurred(ctx), gx, gy, cell,
                                                                                 intensity, static_cast<const rsrt_bloom_texel *>(ctx->bl_pyr.p),
                                                                                 (int)rsrt_bloom_level_size(v.w, 1), (int)rsrt_bloom_level_size(v.h, 1),
                                                                                 static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

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
    return local_display(ctx, "local_gain_download", source, sample_total, exposure, params, 0.0f, nullptr, host_gain, n_floats);
}

rsrt_status rsrt_display_local_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params,
                                     float bloom_intensity, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return local_display(ctx, "display_local_srgb8", source, sample_total, exposure, params, bloom_intensity, host_rgba8, nullptr, n_bytes);
}

} // extern "C"
