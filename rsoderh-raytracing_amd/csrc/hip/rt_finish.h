// rt_finish.h — the finished display's kernel and its C-ABI (include/rsrt.h "finished display").  Included at the end of
// rsrt_api.hip.  All arithmetic is include/rsrt_finish.h's.
//
//  rt_display_finish_kernel<true>   sharpness > 0.  A 256-thread workgroup owns rt_display_colour_kernel's tile of RT_LC_TW x RT_LC_TH
//                                   pixels.  Round one: every lane evaluates rsrt_finish_sdr of its own pixel — the grid, the bloom image
//                                   and the LUT read exactly as the colour display reads them — keeps the sdr in registers and stores the
//                                   record (enc rgb, luma) in LDS.  Round two: lanes 0 .. 83 do the same for the one-pixel ring round the
//                                   tile (34 x 10 = 340 records in all; the chain runs 1.33 times a pixel).  Coordinates are clamped to the
//                                   picture, so a slot past the picture's edge holds the edge pixel's record, which is what the header's
//                                   clamped cross reads there, and no lane leaves before the barrier.  One __syncthreads; then each lane
//                                   sharpens its pixel from five LDS records, adds grain, squares back, dithers and stores one uchar4.
//                                   LDS: one float4 a record (5440 B).  A wave's lanes read two rows of 32 consecutive 16-byte records.
//                                   A 16-byte LDS read is served in four groups of 16 lanes that are not contiguous — lanes {0-3, 12-15,
//                                   20-27} and {4-11, 16-19, 28-31} of each half-wave — and banks repeat every 256 B, 16 records.  A
//                                   half-wave is one row, so lane l reads record base + l: taken modulo 16 either group's lanes are
//                                   sixteen different records, every bank once, whatever the base — at any row pitch and for the x - 1
//                                   and x + 1 taps as well — so nothing serialises and no padding is needed.  By the per-instruction
//                                   rates (4 LDS cycles a 16-byte wave read, 2 a 4-byte one; derived, not measured) five 16-byte reads a
//                                   lane are 20 cycles a wave where three planes of floats would be 15 reads and 30, and the fourth float
//                                   carries the luma the noise limiter wants.
//  rt_display_finish_kernel<false>  sharpness 0: no ring, no LDS, no barrier; one thread a pixel, like rt_display_colour_kernel.
//  No scratch memory in either.
#include "../../../include/rsrt_finish.h"

#define RT_FN_SW (RT_LC_TW + 2)                     // staged records a row
#define RT_FN_SH (RT_LC_TH + 2)
#define RT_FN_RING (2 * RT_FN_SW + 2 * RT_LC_TH)    // 84: the ring's records

static_assert(RT_FN_RING <= RT_LC_BLOCK, "the ring is one round of the workgroup");

// what both display kernels evaluate at a pixel: the sdr of (x, y), 0 <= x < w, 0 <= y < h
__device__ __forceinline__ void rt_finish_sdr_at(const float4 *img, int w, int x, int y, float total, float exposure, bool graded, const rsrt_local_params &p,
                                                 const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, float intensity, const rsrt_bloom_texel *b, int bw,
                                                 int bh, const rsrt_colour_params &colour, const float4 *lut, uint32_t n, float sdr[3])
{
    const float4 a = img[(size_t)y * (size_t)w + (size_t)x];
    const float sum[3] = {a.x, a.y, a.z};
    const float gain = graded ? rsrt_local_gain_at(grid, gx, gy, cell, x, y, rsrt_local_q_of(sum, total), rsrt_local_mid(p.key, exposure), &p) : 1.0f;
    rsrt_finish_sdr(sum, total, exposure, intensity, intensity > 0.0f ? rsrt_bloom_up_at(b, bw, bh, x, y) : rsrt_bloom_make(0.0f, 0.0f, 0.0f), gain, &colour,
                    reinterpret_cast<const float *>(lut), n, sdr);
}

// img: w x h sums; grid, b, lut: as rt_display_colour_kernel takes them; fp: passed rsrt_finish_params_ok, sharpness > 0 exactly when SHARPEN
template <bool SHARPEN>
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_finish_kernel(const float4 *img, int w, int h, float total, float exposure, bool graded, rsrt_local_params p,
                                                                        const uint32_t *grid, uint32_t gx, uint32_t gy, uint32_t cell, float intensity,
                                                                        const rsrt_bloom_texel *b, int bw, int bh, rsrt_colour_params colour, const float4 *lut,
                                                                        uint32_t n, rsrt_finish_params fp, uchar4 *out)
{
    const int tid = (int)threadIdx.x, lx = tid % RT_LC_TW, ly = tid / RT_LC_TW;
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH, x = bx + lx, y = by + ly;
    float sdr[3], e[4];
    unsigned char rgb[3];
    if constexpr (SHARPEN) {
        __shared__ float4 rec[RT_FN_SW * RT_FN_SH]; // rec[(sy + 1) * RT_FN_SW + sx + 1] is the record of pixel (bx + sx, by + sy), clamped to the picture
        {
            const int cx = x < w ? x : w - 1, cy = y < h ? y : h - 1;
            rt_finish_sdr_at(img, w, cx, cy, total, exposure, graded, p, grid, gx, gy, cell, intensity, b, bw, bh, colour, lut, n, sdr);
            rsrt_finish_record(sdr, e);
            rec[(ly + 1) * RT_FN_SW + lx + 1] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (tid < RT_FN_RING) { // the row above, the row below, the column to the left, the column to the right
            int sx, sy;
            if (tid < 2 * RT_FN_SW) {
                sx = tid % RT_FN_SW - 1;
                sy = tid < RT_FN_SW ? -1 : RT_LC_TH;
            } else {
                const int k = tid - 2 * RT_FN_SW;
                sx = k < RT_LC_TH ? -1 : RT_LC_TW;
                sy = k % RT_LC_TH;
            }
            int cx = bx + sx, cy = by + sy;
            cx = cx < 0 ? 0 : (cx < w ? cx : w - 1);
            cy = cy < 0 ? 0 : (cy < h ? cy : h - 1);
            float s2[3], r2[4];
            rt_finish_sdr_at(img, w, cx, cy, total, exposure, graded, p, grid, gx, gy, cell, intensity, b, bw, bh, colour, lut, n, s2);
            rsrt_finish_record(s2, r2);
            rec[(sy + 1) * RT_FN_SW + sx + 1] = make_float4(r2[0], r2[1], r2[2], r2[3]);
        }
        __syncthreads();
        if (x >= w || y >= h) return;
        const int at = (ly + 1) * RT_FN_SW + lx + 1;
        const float4 qb = rec[at - RT_FN_SW], qd = rec[at - 1], qf = rec[at + 1], qh = rec[at + RT_FN_SW];
        const float rb[4] = {qb.x, qb.y, qb.z, qb.w}, rd[4] = {qd.x, qd.y, qd.z, qd.w}, rf[4] = {qf.x, qf.y, qf.z, qf.w}, rh[4] = {qh.x, qh.y, qh.z, qh.w};
        rsrt_finish_pixel(sdr, rb, rd, e, rf, rh, (uint32_t)x, (uint32_t)y, &fp, rgb);
    } else {
        if (x >= w || y >= h) return;
        rt_finish_sdr_at(img, w, x, y, total, exposure, graded, p, grid, gx, gy, cell, intensity, b, bw, bh, colour, lut, n, sdr);
        rsrt_finish_record(sdr, e);
        rsrt_finish_pixel(sdr, e, e, e, e, e, (uint32_t)x, (uint32_t)y, &fp, rgb);
    }
    out[(size_t)y * (size_t)w + (size_t)x] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

extern "C" {

rsrt_status rsrt_display_finished_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                                        float bloom_intensity, const rsrt_colour_params *colour, const rsrt_finish_params *finish, uint8_t *host_rgba8,
                                        size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    const char *const what = "display_finished_srgb8";
    ImageView v;
    rsrt_status st = bloom_source(ctx, what, source, sample_total, exposure, &v);
    if (st) return st;
    const size_t n = v.pixels();
    if (local && !rsrt_local_params_ok(local))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want shadows and highlights in [0, 1], key finite and > 0, max_stops in [0, 16], flags 0", what);
    if (!colour) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: colour is NULL", what);
    if (!rsrt_colour_params_ok(colour)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want white finite and > 0, lut_strength in [0, 1], flags 0", what);
    if (!finish) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: finish is NULL", what);
    if (!rsrt_finish_params_ok(finish))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: want sharpness, grain and dither in [0, 1], flags RSRT_FINISH_NOISE_AWARE or 0", what);
    if (!rsrt_bloom_finite_nonneg(bloom_intensity)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: bloom_intensity must be finite and >= 0", what);
    if (!host_rgba8 || n_bytes != n * 4) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: expected %zu bytes", what, n * 4);
    if (local) {
        if (!ctx->lc_have) return fail(ctx, RSRT_ERR_NOT_READY, "no local exposure grid (rsrt_local_exposure first)");
        if (!ctx->lc_grid.is(v.w, v.h))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the grid was built for %ux%u, the source is %ux%u", what, ctx->lc_grid.w, ctx->lc_grid.h, v.w, v.h);
    }
    if (bloom_intensity > 0.0f) {
        if (!ctx->bl_have) return fail(ctx, RSRT_ERR_NOT_READY, "no bloom image (rsrt_bloom first)");
        if (!ctx->bl_pyr.is(v.w, v.h))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the bloom image was built for %ux%u, the source is %ux%u", what, ctx->bl_pyr.w, ctx->bl_pyr.h, v.w, v.h);
    }
    if (colour->lut_strength > 0.0f && !ctx->cl_n) return fail(ctx, RSRT_ERR_NOT_READY, "no colour LUT (rsrt_colour_lut_build or rsrt_colour_lut_upload first)");
    const uint32_t cell = local ? ctx->lc_cell : RSRT_LOCAL_CELL, gx = rsrt_local_cells(v.w, cell), gy = rsrt_local_cells(v.h, cell);
    const rsrt_local_params lp = local ? *local : rsrt_local_params{0.0f, 0.0f, RSRT_LOCAL_KEY, 0.0f, 0u, 0u};
    const dim3 tiles((v.w + RT_LC_TW - 1u) / RT_LC_TW, (v.h + RT_LC_TH - 1u) / RT_LC_TH);
    const auto kernel = finish->sharpness > 0.0f ? rt_display_finish_kernel<true> : rt_display_finish_kernel<false>;
    return read_back(ctx, host_rgba8, n * 4u, 0, [&](void *tmp) {
        kernel<<<tiles, dim3(RT_LC_BLOCK), 0, ctx->stream>>>(v.img, (int)v.w, (int)v.h, v.total, exposure, local != nullptr, lp, local ? local_blurred(ctx) : nullptr, gx,
                                                             gy, cell, bloom_intensity, static_cast<const rsrt_bloom_texel *>(ctx->bl_pyr.p),
                                                             (int)rsrt_bloom_level_size(v.w, 1), (int)rsrt_bloom_level_size(v.h, 1), *colour, ctx->cl_lut, ctx->cl_n, *finish,
                                                             static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
