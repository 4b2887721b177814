// rt_sky.h — the procedural daylight sky's kernels and their C-ABI (include/rsrt.h "environment", rsrt_environment_sky and
// rsrt_environment_download).  Included at the end of rsrt_api.hip.  All arithmetic is include/rsrt_sky.h's.
//
//  rt_sky_shares_kernel  the small prepass: one thread a row and a column.  A row's share is sin and cos of its theta and the first Perez
//                        factor of Y, x, y (three exp2 and three divisions), a column's cos and sin of its phi — the very functions the
//                        per-texel evaluation calls (rsrt_sky_row_of, rsrt_sky_col_of), so the same bits.  W x 8 B and H x 20 B in the
//                        context's scratch, which the alias builder takes over afterwards on the same stream.
//  rt_sky_fill_kernel    one lane a texel.  A workgroup is 256 consecutive columns of one row at a time (blockIdx.y picks the row and
//                        strides by gridDim.y, so a map taller than the grid's 65535 rows is still covered): the row's share is read
//                        through a wave-uniform address, the column's with one 8-byte load a lane before the loop, and the texel
//                        leaves as one float4 — 64 lanes x 16 B, a wave's store is 1 KiB of consecutive bytes.  A texel costs one
//                        atan2, one sqrt, three exp2 and the matrix; the constants arrive by value in the kernel's arguments.  No LDS,
//                        no scratch memory.
#include "../../../include/rsrt_sky.h"

#define RT_SKY_BLOCK 256

__global__ __launch_bounds__(RT_SKY_BLOCK) void rt_sky_shares_kernel(rsrt_sky_constants k, uint32_t width, uint32_t height, rsrt_sky_col *cols, rsrt_sky_row *rows)
{
    const uint32_t i = blockIdx.x * RT_SKY_BLOCK + threadIdx.x;
    if (i < width) cols[i] = rsrt_sky_col_of(i, width);
    if (i < height) rows[i] = rsrt_sky_row_of(&k, i, height);
}

// cols: width entries, rows: height entries, out: width x height texels; grid (ceil(width / 256), at most height)
__global__ __launch_bounds__(RT_SKY_BLOCK) void rt_sky_fill_kernel(rsrt_sky_constants k, uint32_t width, uint32_t height, const rsrt_sky_col *__restrict__ cols,
                                                                   const rsrt_sky_row *__restrict__ rows, float4 *__restrict__ out)
{
    const uint32_t x = blockIdx.x * RT_SKY_BLOCK + threadIdx.x;
    if (x >= width) return;
    const rsrt_sky_col c = cols[x];
    for (uint32_t y = blockIdx.y; y < height; y += gridDim.y) {
        float rgb[3];
        rsrt_sky_texel(&k, rows[y], c, rgb);
        out[(size_t)y * width + x] = make_float4(rgb[0], rgb[1], rgb[2], 0.0f); // alpha 0, as uploaded maps have
    }
}

extern "C" {

// Fills `slot` with the sky of `params` at width x height and builds its alias table, all on the device.  The contract is
// rsrt_upload_environment's: the temporal history goes first, a refused call leaves every slot as it was.
rsrt_status rsrt_environment_sky(rsrt_context *ctx, uint32_t slot, uint32_t width, uint32_t height, const rsrt_sky_params *params)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ctx->tp_frames = 0; // the temporal history saw the old environment
    if (!params || width == 0 || height == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment_sky: NULL params or zero size");
    if (!rsrt_sky_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT,
                    "environment_sky: want finite parameters, sun_elevation in 1..90 degrees, turbidity in 2..10, ground_albedo, scale and sun_illuminance >= 0, "
                    "sun_radius in 0..0.1, flags 0");
    if ((uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment too large");
    if (slot > 63) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment slot %u > 63", slot);
    const size_t n = (size_t)width * height;
    rsrt_sky_constants k;
    memset(&k, 0, sizeof k);
    rsrt_sky_prepare(params, height, &k);
    // the shares: cols[width] | rows[height]
    const size_t cols_bytes = (size_t)width * sizeof(rsrt_sky_col);
    rsrt_status st = ensure_scratch(ctx, cols_bytes + (size_t)height * sizeof(rsrt_sky_row));
    if (st) return st;
    if (ctx->envs.size() <= slot) ctx->envs.resize(slot + 1);
    Env &e = ctx->envs[slot];
    if ((st = sync_all(ctx))) return st;
    if (e.rgba) { (void)hipFree(e.rgba); e.rgba = nullptr; }
    if (e.alias) { (void)hipFree(e.alias); e.alias = nullptr; }
    e.width = e.height = 0;
    HIP_TRY(ctx, hipMalloc(&e.rgba, n * sizeof(float4)));
    HIP_TRY(ctx, hipMalloc(&e.alias, n * sizeof(uint4)));
    if ((st = begin_work(ctx, ctx->stream))) return st;
    rsrt_sky_col *const cols = static_cast<rsrt_sky_col *>(ctx->scratch);
    rsrt_sky_row *const rows = reinterpret_cast<rsrt_sky_row *>(static_cast<char *>(ctx->scratch) + cols_bytes);
    const uint32_t longest = width > height ? width : height;
    rt_sky_shares_kernel<<<dim3((longest + RT_SKY_BLOCK - 1u) / RT_SKY_BLOCK), dim3(RT_SKY_BLOCK), 0, ctx->stream>>>(k, width, height, cols, rows);
    rt_sky_fill_kernel<<<dim3((width + RT_SKY_BLOCK - 1u) / RT_SKY_BLOCK, height < 65535u ? height : 65535u), dim3(RT_SKY_BLOCK), 0, ctx->stream>>>(k, width, height, cols,
                                                                                                                                                   rows, e.rgba);
    HIP_TRY(ctx, hipGetLastError());
    if ((st = end_work(ctx, ctx->stream))) return st;
    e.width = width;
    e.height = height;
    st = rsrt_environment_build_alias(ctx, slot, nullptr, 0, nullptr); // AliasTable::build_by_luminance on the device, after the fill on the same stream
    if (st) { e.width = e.height = 0; }
    return st;
}

// The texels of `slot` to the host: what was uploaded or what rsrt_environment_sky made, alpha 0.  (On the device a texel's alpha
// word is the library's own — pack_environment keeps a copy of the alias table's pmf there — so it is not returned.)
rsrt_status rsrt_environment_download(rsrt_context *ctx, uint32_t slot, float *host_rgba, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (slot >= ctx->envs.size() || !ctx->envs[slot].rgba || ctx->envs[slot].width == 0) return fail(ctx, RSRT_ERR_NOT_READY, "environment slot %u is empty", slot);
    const Env &e = ctx->envs[slot];
    const size_t n = (size_t)e.width * e.height;
    const rsrt_status st = download_floats(ctx, "environment_download", e.rgba, n * 4u, host_rgba, n_floats);
    if (st) return st;
    for (size_t i = 0; i < n; i++) host_rgba[4u * i + 3u] = 0.0f;
    return RSRT_OK;
}

} // extern "C"
