// rt_finish.h — the finished display's kernel and its C-ABI (include/rsrt.h "finished display").  Included at the end of
// rsrt_api.hip.  All arithmetic is include/rsrt_finish.h's.
//
//  rt_display_finish_kernel<true>   sharpness > 0.  A 256-thread workgroup owns rt_display_colour_kernel's tile of RT_LC_TW x RT_LC_TH
//                                   pixels.  Round one: every lane evaluates rsrt_finish_sdr of its own pixel — its inputs gathered by
//                                   rt_display_gather from the same DisplayChain (rt_local.h) — keeps the sdr in registers and stores the
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
//  No scratch memory in either.  The entry point's checks are display_chain's (rt_local.h); its own are the choice between the two.
#include "../../../include/rsrt_finish.h"

#define RT_FN_SW (RT_LC_TW + 2)                     // staged records a row
#define RT_FN_SH (RT_LC_TH + 2)
#define RT_FN_RING (2 * RT_FN_SW + 2 * RT_LC_TH)    // 84: the ring's records

static_assert(RT_FN_RING <= RT_LC_BLOCK, "the ring is one round of the workgroup");

// fp: passed rsrt_finish_params_ok, sharpness > 0 exactly when SHARPEN
template <bool SHARPEN>
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_finish_kernel(DisplayChain c, rsrt_finish_params fp, uchar4 *out)
{
    const int w = c.w, h = c.h;
    const auto sdr_at = [&c](int px, int py, float s[3]) { // step 1 at a pixel of the picture
        float sum[3], gain;
        rsrt_bloom_rgb up_b;
        rt_display_gather(c, c.graded, px, py, sum, &gain, &up_b);
        rsrt_finish_sdr(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, reinterpret_cast<const float *>(c.lut), c.n, s);
    };
    const int tid = (int)threadIdx.x, lx = tid % RT_LC_TW, ly = tid / RT_LC_TW;
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH, x = bx + lx, y = by + ly;
    float sdr[3], e[4];
    unsigned char rgb[3];
    if constexpr (SHARPEN) {
        __shared__ float4 rec[RT_FN_SW * RT_FN_SH]; // rec[(sy + 1) * RT_FN_SW + sx + 1] is the record of pixel (bx + sx, by + sy), clamped to the picture
        {
            const int cx = x < w ? x : w - 1, cy = y < h ? y : h - 1;
            sdr_at(cx, cy, sdr);
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
            sdr_at(cx, cy, s2);
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
        sdr_at(x, y, sdr);
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
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "display_finished_srgb8", CHAIN_COLOUR | CHAIN_FINISH, source, sample_total, exposure, local, colour, finish, nullptr, bloom_intensity,
                                         host_rgba8, n_bytes, &c);
    if (st) return st;
    const auto kernel = finish->sharpness > 0.0f ? rt_display_finish_kernel<true> : rt_display_finish_kernel<false>;
    return read_back(ctx, host_rgba8, n_bytes, 0, [&](void *tmp) {
        kernel<<<display_tiles(c), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, *finish, static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
