// rt_upsample.h — the guided upsampling's kernel and C-ABI (include/rsrt.h "guided upsampling").  Included at the end of
// rsrt_api.hip, after rt_denoise.h, whose AOV and prepare kernels it launches unchanged.
//
//  guide pass   rt_aov_kernel (rt_denoise.h) into the guide buffer: first-hit records of the OUTPUT size W x H.
//  low pass     rt_dn_prepare_kernel (rt_denoise.h) into scratch of this pass's own: the demodulated colour (float4) and the packed
//               features (4 x binary16) of the low frame w x h.
//  rt_up_kernel the high pass: nine taps of the low frame around X * w / W, weighted by a tent of radius 2 and the denoiser's normal and
//               relative-depth terms against the guide's features, remodulated with the guide's albedo.  A workgroup is 64 x 4 output
//               pixels, a wave one output row: its taps of one low row fall on at most 34 consecutive low pixels (544 B of colour, 272 B
//               of features), the guide record is two contiguous float4 loads a lane (2 KiB a wave), the output one float4 store.  48 B
//               of unique traffic an output pixel; no LDS, no atomics, no scratch memory.  The per-pixel arithmetic is
//               include/rsrt_upsample.h.
#include "../../../include/rsrt_upsample.h"

__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_up_kernel(const float4 *r_lo, const ushort4 *f_lo, const float4 *guide, float4 *out, uint32_t w,
                                                                    uint32_t h, uint32_t W, uint32_t H, float sigma_n, float sigma_z, float guide_total,
                                                                    int demodulate)
{
    const uint32_t X = blockIdx.x * RT_DN_BX + threadIdx.x, Y = blockIdx.y * RT_DN_BY + threadIdx.y;
    if (X >= W || Y >= H) return;
    const size_t P = (size_t)Y * W + (size_t)X;
    float g[8], fr[4], a[3];
    dn_aov(guide, P, g);
    rsrt_dn_features(g, guide_total, fr);
    rsrt_dn_albedo(g, guide_total, a);
    const float fp[4] = {dn_f(dn_h(fr[0])), dn_f(dn_h(fr[1])), dn_f(dn_h(fr[2])), dn_f(dn_h(fr[3]))};
    const float kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
    const float u = rsrt_up_coord(X, w, W), v = rsrt_up_coord(Y, h, H);
    const int xn = rsrt_up_nearest(u), yn = rsrt_up_nearest(v);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = yn + dy;
        if (qy < 0 || qy >= (int)h) continue;
        const float hy = rsrt_up_tent(qy, v);
        const float4 *rrow = r_lo + (size_t)qy * w;
        const ushort4 *frow = f_lo + (size_t)qy * w;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = xn + dx;
            if (qx < 0 || qx >= (int)w) continue;
            const float hx = rsrt_up_tent(qx, u);
            const float4 cq = rrow[qx];
            const ushort4 gq = frow[qx];
            const float rq[3] = {cq.x, cq.y, cq.z}, fq[4] = {dn_f(gq.x), dn_f(gq.y), dn_f(gq.z), dn_f(gq.w)};
            rsrt_up_tap(hx * hy, fp, kn, kz, rq, fq, acc);
        }
    }
    float nearest[3] = {0.0f, 0.0f, 0.0f}, o[3];
    if (!(acc[3] > 0.0f)) { // the weights sum to nothing (or to NaN): the nearest low pixel
        const float4 c = r_lo[(size_t)min(yn, (int)h - 1) * w + (size_t)min(xn, (int)w - 1)];
        nearest[0] = c.x; nearest[1] = c.y; nearest[2] = c.z;
    }
    rsrt_up_finish(acc, nearest, a, demodulate, o);
    out[P] = make_float4(o[0], o[1], o[2], 1.0f);
}

namespace {

// the library's guide buffer: width x height records, zeroed; independent of the accumulator (a bound one must match)
rsrt_status ensure_guide(rsrt_context *ctx, uint32_t width, uint32_t height)
{
    if (ctx->guide && ctx->guide_w == width && ctx->guide_h == height) return RSRT_OK;
    if (ctx->guide && ctx->guide != ctx->guide_owned)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bound guide buffer is %ux%u but %ux%u was requested", ctx->guide_w, ctx->guide_h, width, height);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (ctx->guide_owned) { (void)hipFree(ctx->guide_owned); ctx->guide_owned = nullptr; ctx->guide = nullptr; ctx->guide_w = ctx->guide_h = 0; }
    const size_t bytes = (size_t)width * height * 2u * sizeof(float4);
    HIP_TRY(ctx, hipMalloc(&ctx->guide_owned, bytes));
    HIP_TRY(ctx, hipMemsetAsync(ctx->guide_owned, 0, bytes, ctx->stream)); // (on the context's stream: see ensure_aov)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->guide = ctx->guide_owned;
    ctx->guide_w = width;
    ctx->guide_h = height;
    return RSRT_OK;
}

// the low pass's colour (float4) and packed features (ushort4) for the accumulator's size, and the library-owned output for the guide's.
// Scratch of its own: the denoiser's may hold the last denoise output, which is one of this pass's inputs.
rsrt_status ensure_upsample_buffers(rsrt_context *ctx, bool own_output)
{
    const bool scratch_ok = ctx->up_scratch && ctx->up_w == ctx->acc_w && ctx->up_h == ctx->acc_h;
    const bool out_ok = !own_output || (ctx->up_out && ctx->up_out_w == ctx->guide_w && ctx->up_out_h == ctx->guide_h);
    if (scratch_ok && out_ok) return RSRT_OK;
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (!scratch_ok) {
        (void)hipFree(ctx->up_scratch);
        ctx->up_scratch = nullptr;
        ctx->up_w = ctx->up_h = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->up_scratch, (size_t)ctx->acc_w * ctx->acc_h * (sizeof(float4) + sizeof(ushort4))));
        ctx->up_w = ctx->acc_w;
        ctx->up_h = ctx->acc_h;
    }
    if (!out_ok) {
        if (ctx->up_last == ctx->up_out) ctx->up_last = nullptr;
        (void)hipFree(ctx->up_out);
        ctx->up_out = nullptr;
        ctx->up_out_w = ctx->up_out_h = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->up_out, (size_t)ctx->guide_w * ctx->guide_h * sizeof(float4)));
        ctx->up_out_w = ctx->guide_w;
        ctx->up_out_h = ctx->guide_h;
    }
    return RSRT_OK;
}

} // namespace

extern "C" {

rsrt_status rsrt_guide_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                              uint32_t sample_count, uint32_t flags, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if (flags != 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_render: flags must be 0");
    if (ctx->world != 1) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_render: whole frame only (partition of %u ranks)", ctx->world);
    if (width == 0 || height == 0 || width > RSRT_UP_MAX_SIZE || height > RSRT_UP_MAX_SIZE)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_render: bad resolution %ux%u (1 .. %u)", width, height, RSRT_UP_MAX_SIZE);
    if ((uint64_t)sample_begin + sample_count > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "sample range overflows u32");
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    rsrt_status st = ensure_guide(ctx, width, height);
    if (st) return st;
    if (sample_count == 0) return RSRT_OK;
    return launch_aov(ctx, camera, width, height, sample_begin, sample_count, ctx->guide, stream);
}

rsrt_status rsrt_guide_bind(rsrt_context *ctx, void *device_f32x8, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (!device_f32x8) {
        if (ctx->guide != ctx->guide_owned) ctx->guide_w = ctx->guide_h = 0; // (a bound buffer's size says nothing about the library's)
        ctx->guide = ctx->guide_owned;
        return RSRT_OK;
    }
    if (width == 0 || height == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", width, height);
    if ((uintptr_t)device_f32x8 % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide pointer must be 16-byte aligned");
    if (ctx->guide_owned) { (void)hipFree(ctx->guide_owned); ctx->guide_owned = nullptr; }
    ctx->guide = static_cast<float4 *>(device_f32x8);
    ctx->guide_w = width;
    ctx->guide_h = height;
    return RSRT_OK;
}

rsrt_status rsrt_guide_clear(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->guide) return fail(ctx, RSRT_ERR_NOT_READY, "no guide buffer");
    rsrt_status st = begin_work(ctx, ctx->stream);
    if (st) return st;
    HIP_TRY(ctx, hipMemsetAsync(ctx->guide, 0, (size_t)ctx->guide_w * ctx->guide_h * 2u * sizeof(float4), ctx->stream));
    return end_work(ctx, ctx->stream);
}

rsrt_status rsrt_guide_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->guide) return fail(ctx, RSRT_ERR_NOT_READY, "no guide buffer");
    if (!host || n_floats != (size_t)ctx->guide_w * ctx->guide_h * 8u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_download: expected %zu floats", (size_t)ctx->guide_w * ctx->guide_h * 8u);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    HIP_TRY(ctx, hipMemcpy(host, ctx->guide, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return RSRT_OK;
}

rsrt_status rsrt_upsample(rsrt_context *ctx, uint32_t sample_total, uint32_t aov_sample_total, uint32_t guide_sample_total,
                          const rsrt_upsample_params *params, void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: params is NULL");
    if (ctx->world != 1) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: whole frame only (partition of %u ranks)", ctx->world);
    if (!ctx->accum) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    if (!ctx->aov) return fail(ctx, RSRT_ERR_NOT_READY, "upsample: no AOV buffer (rsrt_aov_render or rsrt_aov_bind first)");
    if (!ctx->guide) return fail(ctx, RSRT_ERR_NOT_READY, "upsample: no guide buffer (rsrt_guide_render or rsrt_guide_bind first)");
    if (ctx->aov_w != ctx->acc_w || ctx->aov_h != ctx->acc_h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: AOV buffer is %ux%u, accumulator %ux%u", ctx->aov_w, ctx->aov_h, ctx->acc_w, ctx->acc_h);
    if (ctx->guide_w < ctx->acc_w || ctx->guide_h < ctx->acc_h || ctx->guide_w > RSRT_UP_MAX_SIZE || ctx->guide_h > RSRT_UP_MAX_SIZE)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: guide is %ux%u, accumulator %ux%u (the guide is at least as large, at most %u)", ctx->guide_w,
                    ctx->guide_h, ctx->acc_w, ctx->acc_h, RSRT_UP_MAX_SIZE);
    const rsrt_upsample_params &p = *params;
    if (p.flags & ~(uint32_t)(RSRT_UPSAMPLE_DEMODULATE | RSRT_UPSAMPLE_DENOISED | RSRT_UPSAMPLE_TEMPORAL))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: unknown flags 0x%x", p.flags);
    const bool denoised = (p.flags & RSRT_UPSAMPLE_DENOISED) != 0, temporal = (p.flags & RSRT_UPSAMPLE_TEMPORAL) != 0;
    if (denoised && temporal) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: RSRT_UPSAMPLE_DENOISED and RSRT_UPSAMPLE_TEMPORAL exclude each other");
    if (denoised || temporal) sample_total = 1u; // a colour, not a sum
    if (!sigma_ok(p.sigma_normal) || !sigma_ok(p.sigma_depth)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: sigmas must lie in [1e-6, 1e6]");
    if (sample_total == 0 || aov_sample_total == 0 || guide_sample_total == 0)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: sample_total, aov_sample_total and guide_sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: output pointer must be 16-byte aligned");
    if (denoised && !ctx->dn_last) return fail(ctx, RSRT_ERR_NOT_READY, "upsample: no denoised image (rsrt_denoise first)");
    if (temporal && (!ctx->tp_frames || ctx->tp_w != ctx->acc_w || ctx->tp_h != ctx->acc_h))
        return fail(ctx, RSRT_ERR_NOT_READY, "upsample: no temporal frame since the last reset (rsrt_temporal_accumulate first)");
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    rsrt_status st = ensure_upsample_buffers(ctx, device_out_rgba32f == nullptr);
    if (st || (st = begin_work(ctx, stream))) return st;
    const uint32_t w = ctx->acc_w, h = ctx->acc_h, W = ctx->guide_w, H = ctx->guide_h;
    const size_t n = (size_t)w * h;
    float4 *r_lo = static_cast<float4 *>(ctx->up_scratch);
    ushort4 *f_lo = reinterpret_cast<ushort4 *>(r_lo + n);
    float4 *out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : ctx->up_out;
    const float4 *colour = denoised ? ctx->dn_last : (temporal ? temporal_history(ctx) : ctx->accum);
    const int demod = (p.flags & RSRT_UPSAMPLE_DEMODULATE) ? 1 : 0;
    rt_dn_prepare_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(colour, ctx->aov, n, (float)sample_total, (float)aov_sample_total, demod, 0,
                                                                                      r_lo, f_lo);
    const dim3 grid((W + RT_DN_BX - 1) / RT_DN_BX, (H + RT_DN_BY - 1) / RT_DN_BY), block(RT_DN_BX, RT_DN_BY);
    rt_up_kernel<<<grid, block, 0, stream>>>(r_lo, f_lo, ctx->guide, out, w, h, W, H, p.sigma_normal, p.sigma_depth, (float)guide_sample_total, demod);
    HIP_TRY(ctx, hipGetLastError());
    ctx->up_last = out;
    ctx->up_last_w = W;
    ctx->up_last_h = H;
    return end_work(ctx, stream);
}

rsrt_status rsrt_upsampled_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->up_last) return fail(ctx, RSRT_ERR_NOT_READY, "no upsampled image (rsrt_upsample first)");
    const size_t want = (size_t)ctx->up_last_w * ctx->up_last_h * 4u;
    if (!host || n_floats != want) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsampled_download: expected %zu floats", want);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    HIP_TRY(ctx, hipMemcpy(host, ctx->up_last, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return RSRT_OK;
}

rsrt_status rsrt_upsampled_display_srgb8(rsrt_context *ctx, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    if (!ctx->up_last) return fail(ctx, RSRT_ERR_NOT_READY, "no upsampled image (rsrt_upsample first)");
    return display_from_n(ctx, ctx->up_last, (size_t)ctx->up_last_w * ctx->up_last_h, 1u, host_rgba8, n_bytes);
}

} // extern "C"
