// rt_noise.h — the noise estimate's kernel and C-ABI (include/rsrt.h "noise estimate").  Included at the end of
// rsrt_api.hip.
//
//  snapshot              a device-to-device copy of the accumulator (the sum of n1 samples) into a library-owned buffer of its size.
//  rt_noise_tile_kernel  one wave per tile: lane l walks the tile's pixels l, l + 64, ... (row-major inside the tile), reads the
//                        accumulator's and the snapshot's float4 of each pixel inside the frame, adds the pixel's error in that order
//                        and the wave sums its 64 partial sums with six butterfly steps; lane 0 writes the tile's mean.  A 16-pixel
//                        tile row is 256 B, so one step of a wave reads four rows of each buffer; four steps' loads are issued before
//                        the first is used.  32 B of unique traffic a pixel, 4 B a tile; no LDS, no atomics, no scratch memory.  The
//                        arithmetic is include/rsrt_noise.h.
#include "../../../include/rsrt_noise.h"

#define RT_NS_WAVES 4u // tiles (waves) a workgroup
#define RT_NS_AHEAD 4  // steps whose loads are in flight together

__global__ __launch_bounds__(RT_NS_WAVES * RT_WAVE) void rt_noise_tile_kernel(const float4 *acc, const float4 *snap, float *tiles, uint32_t W, uint32_t H,
                                                                              uint32_t tile_w, uint32_t tile_h, uint32_t tiles_x, uint32_t n_tiles, float n1,
                                                                              float n2)
{
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1u);
    const uint32_t tile = blockIdx.x * RT_NS_WAVES + threadIdx.x / RT_WAVE; // the same for a whole wave
    if (tile >= n_tiles) return;
    const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
    const uint32_t x0 = tx * tile_w, y0 = ty * tile_h;
    const uint32_t T = tile_w * tile_h;
    const uint32_t dx = RT_WAVE % tile_w, dy = RT_WAVE / tile_w; // pixel i + 64 from pixel i
    uint32_t x = lane % tile_w, y = lane / tile_w;
    float v = 0.0f;
    for (uint32_t i = lane; i < T; i += RT_WAVE * RT_NS_AHEAD) {
        float4 c1[RT_NS_AHEAD], c2[RT_NS_AHEAD];
        bool in[RT_NS_AHEAD];
#pragma unroll
        for (int k = 0; k < RT_NS_AHEAD; k++) {
            in[k] = i + RT_WAVE * (uint32_t)k < T && x0 + x < W && y0 + y < H;
            if (in[k]) {
                const size_t p = (size_t)(y0 + y) * W + (size_t)(x0 + x);
                c2[k] = acc[p];
                c1[k] = snap[p];
            }
            x += dx;
            y += dy;
            if (x >= tile_w) { x -= tile_w; y++; }
        }
#pragma unroll
        for (int k = 0; k < RT_NS_AHEAD; k++)
            if (in[k]) {
                const float s1[3] = {c1[k].x, c1[k].y, c1[k].z}, s2[3] = {c2[k].x, c2[k].y, c2[k].z};
                v = v + rsrt_noise_pixel(s1, n1, s2, n2);
            }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, RT_WAVE); // (every lane of the wave is here: the return above is per wave)
    if (lane == 0) tiles[tile] = v / (float)rsrt_noise_tile_count(tx, ty, tile_w, tile_h, W, H);
}

extern "C" {

rsrt_status rsrt_noise_snapshot(rsrt_context *ctx, uint32_t sample_total, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "noise_snapshot");
    if (st) return st;
    if (sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_snapshot: sample_total must be > 0");
    if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    ctx->ns_total = 0; // (a new buffer or a failed copy leaves no snapshot)
    if ((st = ensure_sized(ctx, ctx->ns_snap, ctx->acc.w, ctx->acc.h, sizeof(float4))) || (st = begin_work(ctx, stream))) return st;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ns_snap.p, ctx->acc.p, ctx->acc.bytes(), hipMemcpyDeviceToDevice, stream));
    ctx->ns_total = sample_total;
    return end_work(ctx, stream);
}

rsrt_status rsrt_noise_estimate(rsrt_context *ctx, uint32_t sample_total, const rsrt_noise_params *params, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_estimate: params is NULL");
    rsrt_status st = whole_frame(ctx, "noise_estimate");
    if (st) return st;
    const rsrt_noise_params &p = *params;
    if (p.flags != 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_estimate: flags must be 0");
    if (!rsrt_noise_tile_ok(p.tile_w, p.tile_h))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_estimate: tile %ux%u: pixel count must be a multiple of 64 and at most 4096", p.tile_w, p.tile_h);
    if (!(p.threshold >= 0.0f)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_estimate: threshold must be >= 0");
    if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    if (ctx->ns_total == 0 || !ctx->ns_snap.is(ctx->acc.w, ctx->acc.h))
        return fail(ctx, RSRT_ERR_NOT_READY, "noise_estimate: no snapshot of this accumulator (rsrt_noise_snapshot first)");
    if (sample_total <= ctx->ns_total)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_estimate: sample_total %u is not above the snapshot's %u", sample_total, ctx->ns_total);
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const uint32_t W = ctx->acc.w, H = ctx->acc.h;
    const uint32_t tiles_x = (W - 1u) / p.tile_w + 1u, tiles_y = (H - 1u) / p.tile_h + 1u;
    const size_t n_tiles = (size_t)tiles_x * tiles_y;
    if (n_tiles > ctx->ns_tiles_cap) {
        { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
        (void)hipFree(ctx->ns_tiles);
        ctx->ns_tiles = nullptr;
        ctx->ns_tiles_cap = 0;
        ctx->ns_have = false;
        HIP_TRY(ctx, hipMalloc(&ctx->ns_tiles, n_tiles * sizeof(float)));
        ctx->ns_tiles_cap = n_tiles;
    }
    if ((st = begin_work(ctx, stream))) return st;
    rt_noise_tile_kernel<<<dim3((unsigned)((n_tiles + RT_NS_WAVES - 1u) / RT_NS_WAVES)), dim3(RT_NS_WAVES * RT_WAVE), 0, stream>>>(
        ctx->acc.p, static_cast<const float4 *>(ctx->ns_snap.p), ctx->ns_tiles, W, H, p.tile_w, p.tile_h, tiles_x, (uint32_t)n_tiles, (float)ctx->ns_total, (float)sample_total);
    HIP_TRY(ctx, hipGetLastError());
    ctx->ns_tx = tiles_x;
    ctx->ns_ty = tiles_y;
    ctx->ns_threshold = p.threshold;
    ctx->ns_have = true;
    return end_work(ctx, stream);
}

rsrt_status rsrt_noise_download(rsrt_context *ctx, float *host_tiles, size_t n_floats, rsrt_noise_summary *out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "noise_download"); if (st0) return st0; }
    if (!ctx->ns_have) return fail(ctx, RSRT_ERR_NOT_READY, "no noise estimate (rsrt_noise_estimate first)");
    const size_t n = (size_t)ctx->ns_tx * ctx->ns_ty;
    if (host_tiles && n_floats != n) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "noise_download: expected %zu floats", n);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    std::vector<float> own;
    if (!host_tiles) { own.resize(n); host_tiles = own.data(); }
    HIP_TRY(ctx, hipMemcpy(host_tiles, ctx->ns_tiles, n * sizeof(float), hipMemcpyDeviceToHost));
    if (!out) return RSRT_OK;
    float mx = host_tiles[0], sum = 0.0f;
    uint32_t above = 0;
    for (size_t i = 0; i < n; i++) { // row-major, in order
        const float e = host_tiles[i];
        if (e > mx) mx = e;
        sum = sum + e;
        above += rsrt_noise_above(e, ctx->ns_threshold) ? 1u : 0u;
    }
    out->max_error = mx;
    out->mean_error = sum / (float)n;
    out->tiles_x = ctx->ns_tx;
    out->tiles_y = ctx->ns_ty;
    out->tiles_above = above;
    out->_pad = 0;
    return RSRT_OK;
}

rsrt_status rsrt_noise_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "noise_reset"); if (st0) return st0; }
    drop_noise(ctx);
    return RSRT_OK;
}

} // extern "C"
