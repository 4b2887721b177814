// rt_colour.h — the white-balance meter's kernel, the colour LUT's bake kernel, the colour display kernel and their C-ABI
// (include/rsrt.h "white balance and colour grading").  Included at the end of rsrt_api.hip.  All arithmetic is
// include/rsrt_colour.h's.
//
//  rt_white_hist_kernel       rt_exposure_hist_kernel's trips — a 256-thread workgroup walks trips of 2048 consecutive pixels, eight
//                             16-byte loads a lane in flight — over a 4097-word histogram.  Four per-wave copies (65552 B) do not fit
//                             under the 64 KB static limit, so the workgroup's four waves share ONE copy in LDS (16388 B) and count in
//                             it with integer adds whose results are not used; a wave whose 64 pixels share a word (a wall, the sky)
//                             lets lane 0 add 64.  After one __syncthreads every non-zero word goes to the histogram in global memory
//                             with one integer atomic; at most one workgroup a CU.  Integers only: the result does not depend on the
//                             order of anything.  Two histograms in the context, as the exposure meter has them: a call adds into
//                             the zero one and its workgroup 0 zeroes the other for the call after, so a meter call is one launch.
//  rt_colour_lut_kernel       one thread a node: rsrt_colour_lut_node, stored as a float4 (alpha 1).
//  rt_display_colour_kernel   rt_display_local_kernel's tile and DisplayChain (rt_local.h) with rsrt_display_pixel_colour; the grid is
//                             read only with a local grade, the bloom image only with intensity > 0 (rt_display_gather), the LUT — four
//                             16-byte nodes a pixel, through L2 — only with lut_strength > 0.  No scratch memory, no LDS.
#include "../../../include/rsrt_colour.h"

#define RT_WB_BLOCK 256u
#define RT_WB_AHEAD 8u              // loads in flight a lane
#define RT_WB_NONE 0xffffffffu      // a lane past the image's end
#define RT_WB_STRIDE 4608u          // words from one histogram to the other: each starts a 2 KB line of its own

static_assert(RT_WB_STRIDE >= RSRT_WHITE_WORDS && RT_WB_STRIDE % 512u == 0u, "");

// hist: zero before the launch; next: zeroed here for the call after this one
__global__ __launch_bounds__(RT_WB_BLOCK) void rt_white_hist_kernel(const float4 *img, size_t n, float total, uint32_t *hist, uint32_t *next)
{
    __shared__ uint32_t h[RSRT_WHITE_WORDS];
    if (blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < RSRT_WHITE_WORDS; w += RT_WB_BLOCK) next[w] = 0u;
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1u);
    for (uint32_t i = threadIdx.x; i < RSRT_WHITE_WORDS; i += RT_WB_BLOCK) h[i] = 0u;
    __syncthreads();
    const size_t trip = (size_t)RT_WB_BLOCK * RT_WB_AHEAD;
    for (size_t base = (size_t)blockIdx.x * trip; base < n; base += (size_t)gridDim.x * trip) { // (base is the workgroup's: no lane leaves early)
        float4 c[RT_WB_AHEAD];
        bool in[RT_WB_AHEAD];
#pragma unroll
        for (uint32_t k = 0; k < RT_WB_AHEAD; k++) {
            const size_t p = base + (size_t)k * RT_WB_BLOCK + threadIdx.x;
            in[k] = p < n;
            if (in[k]) c[k] = img[p];
        }
#pragma unroll
        for (uint32_t k = 0; k < RT_WB_AHEAD; k++) {
            uint32_t word = RT_WB_NONE;
            if (in[k]) {
                const float sum[3] = {c[k].x, c[k].y, c[k].z};
                word = rsrt_white_word(sum, total);
            }
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
            if (__ballot(word == first) == ~0ull) { // all 64 lanes are here, and they agree
                if (first != RT_WB_NONE && lane == 0u) atomicAdd(&h[first], (uint32_t)RT_WAVE);
            } else if (word != RT_WB_NONE) {
                atomicAdd(&h[word], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < RSRT_WHITE_WORDS; w += RT_WB_BLOCK) {
        const uint32_t s = h[w];
        if (s) atomicAdd(&hist[w], s);
    }
}

__global__ __launch_bounds__(256) void rt_colour_lut_kernel(float4 *lut, uint32_t n, rsrt_cdl_params p)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n * n * n) return;
    float rgb[3];
    rsrt_colour_lut_node(n, i % n, (i / n) % n, i / (n * n), &p, rgb);
    lut[i] = make_float4(rgb[0], rgb[1], rgb[2], 1.0f);
}

// rt_display_local_kernel's tile with the white point and the LUT
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_colour_kernel(DisplayChain c, uchar4 *out)
{
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH;
    const int x = bx + (int)threadIdx.x % RT_LC_TW, y = by + (int)threadIdx.x / RT_LC_TW;
    if (x >= c.w || y >= c.h) return;
    float sum[3], gain;
    rsrt_bloom_rgb up_b;
    rt_display_gather(c, c.graded, x, y, sum, &gain, &up_b);
    unsigned char rgb[3];
    rsrt_display_pixel_colour(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, reinterpret_cast<const float *>(c.lut), c.n, rgb);
    out[(size_t)y * (size_t)c.w + (size_t)x] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

namespace {

const MeterShape kWhiteMeter = {RSRT_WHITE_WORDS, RT_WB_STRIDE, RT_WB_BLOCK, RT_WB_AHEAD, rt_white_hist_kernel};

size_t lut_nodes(uint32_t n) { return (size_t)n * n * n; }

// room for an n^3 LUT; what the context held is gone when the allocation had to grow
rsrt_status lut_room(rsrt_context *ctx, uint32_t n)
{
    if (ctx->cl_lut && ctx->cl_cap >= lut_nodes(n)) return RSRT_OK;
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    (void)hipFree(ctx->cl_lut);
    ctx->cl_lut = nullptr;
    ctx->cl_cap = 0;
    ctx->cl_n = 0;
    HIP_TRY(ctx, hipMalloc(&ctx->cl_lut, lut_nodes(n) * sizeof(float4)));
    ctx->cl_cap = lut_nodes(n);
    return RSRT_OK;
}

} // namespace

extern "C" {

rsrt_status rsrt_white_meter(rsrt_context *ctx, uint32_t source, uint32_t sample_total, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ImageView v;
    const rsrt_status st = exposure_source(ctx, "white_meter", source, sample_total, &v);
    return st ? st : meter_launch(ctx, ctx->wb, kWhiteMeter, v, stream_of(ctx, hip_stream));
}

rsrt_status rsrt_white_download(rsrt_context *ctx, const rsrt_white_params *params, uint32_t *host_hist, size_t n_words, rsrt_white_result *out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "white_download"); if (st0) return st0; }
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "white_download: params is NULL");
    if (!rsrt_white_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "white_download: want gate in 1 .. 31, iterations <= 8, min_permille <= 1000, strength and blend in [0, 1], "
                                                     "max_stops in [0, 4], previous all 0 or finite and > 0, flags 0");
    if (host_hist && n_words != RSRT_WHITE_WORDS) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "white_download: expected %u words", RSRT_WHITE_WORDS);
    if (!ctx->wb.have) return fail(ctx, RSRT_ERR_NOT_READY, "no chroma histogram (rsrt_white_meter first)");
    return meter_download(ctx, ctx->wb, kWhiteMeter, host_hist, [&](const uint32_t *hist) {
        if (out) rsrt_white_from_histogram(hist, params, out);
    });
}

rsrt_status rsrt_white_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    return meter_reset(ctx, ctx->wb, "white_reset");
}

rsrt_status rsrt_colour_lut_build(rsrt_context *ctx, uint32_t n, const rsrt_cdl_params *cdl, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "colour_lut_build"); if (st0) return st0; }
    if (!rsrt_colour_lut_size_ok(n)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_build: n must be 2, 3, 17, 33 or 65");
    if (!cdl) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_build: cdl is NULL");
    if (!rsrt_cdl_params_ok(cdl))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_build: want slope in [0, 16], offset in [-1, 1], power in [0.25, 4], saturation in [0, 4], flags 0");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    rsrt_status st = lut_room(ctx, n);
    if (st || (st = begin_work(ctx, stream))) return st;
    ctx->cl_n = 0; // (a failed launch leaves no LUT)
    rt_colour_lut_kernel<<<dim3((unsigned)((lut_nodes(n) + 255u) / 256u)), dim3(256), 0, stream>>>(ctx->cl_lut, n, *cdl);
    HIP_TRY(ctx, hipGetLastError());
    ctx->cl_n = n;
    return end_work(ctx, stream);
}

rsrt_status rsrt_colour_lut_upload(rsrt_context *ctx, uint32_t n, const float *host_rgb, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "colour_lut_upload"); if (st0) return st0; }
    if (!rsrt_colour_lut_size_ok(n)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_upload: n must be 2, 3, 17, 33 or 65");
    if (!host_rgb || n_floats != 3u * lut_nodes(n)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_upload: expected %zu floats", 3u * lut_nodes(n));
    std::vector<float4> nodes(lut_nodes(n));
    for (size_t i = 0; i < nodes.size(); i++) {
        const float *c = host_rgb + 3u * i;
        if (!(rsrt_colour_in(c[0], 0.0f, 1.0f) && rsrt_colour_in(c[1], 0.0f, 1.0f) && rsrt_colour_in(c[2], 0.0f, 1.0f)))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_upload: node %zu is not finite and in [0, 1]", i);
        nodes[i] = make_float4(c[0], c[1], c[2], 1.0f);
    }
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; } // (a display may still read the LUT this one replaces)
    rsrt_status st = lut_room(ctx, n);
    if (st) return st;
    ctx->cl_n = 0;
    HIP_TRY(ctx, hipMemcpy(ctx->cl_lut, nodes.data(), nodes.size() * sizeof(float4), hipMemcpyHostToDevice));
    ctx->cl_n = n;
    return RSRT_OK;
}

rsrt_status rsrt_colour_lut_download(rsrt_context *ctx, float *host_rgb, size_t n_floats, uint32_t *n_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "colour_lut_download"); if (st0) return st0; }
    if (!ctx->cl_n) return fail(ctx, RSRT_ERR_NOT_READY, "no colour LUT (rsrt_colour_lut_build or rsrt_colour_lut_upload first)");
    const size_t nodes = lut_nodes(ctx->cl_n);
    if (host_rgb || n_floats) {
        if (!host_rgb || n_floats != 3u * nodes) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "colour_lut_download: expected %zu floats", 3u * nodes);
        { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
        std::vector<float4> tmp(nodes);
        HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->cl_lut, nodes * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nodes; i++) {
            host_rgb[3u * i] = tmp[i].x;
            host_rgb[3u * i + 1] = tmp[i].y;
            host_rgb[3u * i + 2] = tmp[i].z;
        }
    }
    if (n_out) *n_out = ctx->cl_n;
    return RSRT_OK;
}

rsrt_status rsrt_colour_lut_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "colour_lut_reset"); if (st0) return st0; }
    ctx->cl_n = 0;
    return RSRT_OK;
}

rsrt_status rsrt_display_colour_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                                      float bloom_intensity, const rsrt_colour_params *colour, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "display_colour_srgb8", CHAIN_COLOUR, source, sample_total, exposure, local, colour, nullptr, nullptr, bloom_intensity, host_rgba8,
                                         n_bytes, &c);
    if (st) return st;
    return read_back(ctx, host_rgba8, n_bytes, 0, [&](void *tmp) {
        rt_display_colour_kernel<<<display_tiles(c), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
