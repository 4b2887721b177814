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

extern "C" {

rsrt_status rsrt_guide_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                              uint32_t sample_count, uint32_t flags, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if (flags != 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_render: flags must be 0");
    rsrt_status st = whole_frame(ctx, "guide_render");
    if (st) return st;
    if (width == 0 || height == 0 || width > RSRT_UP_MAX_SIZE || height > RSRT_UP_MAX_SIZE)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "guide_render: bad resolution %ux%u (1 .. %u)", width, height, RSRT_UP_MAX_SIZE);
    if ((uint64_t)sample_begin + sample_count > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "sample range overflows u32");
    if ((st = buffer_ensure(ctx, ctx->guide, width, height))) return st; // (independent of the accumulator's size)
    if (sample_count == 0) return RSRT_OK;
    return launch_aov(ctx, camera, width, height, sample_begin, sample_count, ctx->guide.p, stream_of(ctx, hip_stream));
}

rsrt_status rsrt_guide_bind(rsrt_context *ctx, void *device_f32x8, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_bind(ctx, ctx->guide, device_f32x8, width, height);
}

rsrt_status rsrt_guide_clear(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_clear(ctx, ctx->guide);
}

rsrt_status rsrt_guide_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_download(ctx, "guide_download", ctx->guide, host, n_floats);
}

rsrt_status rsrt_upsample(rsrt_context *ctx, uint32_t sample_total, uint32_t aov_sample_total, uint32_t guide_sample_total,
                          const rsrt_upsample_params *params, void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: params is NULL");
    rsrt_status st = whole_frame(ctx, "upsample");
    if (st || (st = accumulator_and_aov(ctx, "upsample", &ctx->guide))) return st;
    const uint32_t w = ctx->acc.w, h = ctx->acc.h, W = ctx->guide.w, H = ctx->guide.h;
    if (W < w || H < h || W > RSRT_UP_MAX_SIZE || H > RSRT_UP_MAX_SIZE)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "upsample: guide is %ux%u, accumulator %ux%u (the guide is at least as large, at most %u)", W, H, w, h, RSRT_UP_MAX_SIZE);
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
    ImageView colour;
    if ((st = resolve_image(ctx, "upsample", "upsample: ", denoised ? IMAGE_DENOISED : (temporal ? IMAGE_TEMPORAL : IMAGE_MEAN), sample_total, true, &colour))) return st;
    const hipStream_t stream = stream_of(ctx, hip_stream);
    // The low pass's colour (float4) and packed features (ushort4) for the accumulator's size — scratch of its own: the denoiser's may hold
    // the last denoise output, which is one of this pass's inputs — and, unless the caller gave one, the output for the guide's size.
    if ((st = ensure_sized(ctx, ctx->up_scratch, w, h, sizeof(float4) + sizeof(ushort4)))) return st;
    if (!device_out_rgba32f) {
        if (!ctx->up_out.is(W, H) && ctx->up_last.img == ctx->up_out.p) ctx->up_last = ImageView{}; // (it goes with the buffer it is in)
        if ((st = ensure_sized(ctx, ctx->up_out, W, H, sizeof(float4)))) return st;
    }
    if ((st = begin_work(ctx, stream))) return st;
    const size_t n = (size_t)w * h;
    float4 *r_lo = static_cast<float4 *>(ctx->up_scratch.p);
    ushort4 *f_lo = reinterpret_cast<ushort4 *>(r_lo + n);
    float4 *out = static_cast<float4 *>(device_out_rgba32f ? device_out_rgba32f : ctx->up_out.p);
    const int demod = (p.flags & RSRT_UPSAMPLE_DEMODULATE) ? 1 : 0;
    rt_dn_prepare_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(colour.img, ctx->aov.p, n, colour.total, (float)aov_sample_total, demod, 0, r_lo,
                                                                                      f_lo);
    const dim3 grid((W + RT_DN_BX - 1) / RT_DN_BX, (H + RT_DN_BY - 1) / RT_DN_BY), block(RT_DN_BX, RT_DN_BY);
    rt_up_kernel<<<grid, block, 0, stream>>>(r_lo, f_lo, ctx->guide.p, out, w, h, W, H, p.sigma_normal, p.sigma_depth, (float)guide_sample_total, demod);
    HIP_TRY(ctx, hipGetLastError());
    ctx->up_last = ImageView{out, W, H, 1.0f};
    return end_work(ctx, stream);
}

rsrt_status rsrt_upsampled_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return image_download(ctx, "upsampled_download", IMAGE_UPSAMPLED, host, n_floats);
}

rsrt_status rsrt_upsampled_display_srgb8(rsrt_context *ctx, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    return image_display(ctx, "upsampled_display_srgb8", IMAGE_UPSAMPLED, 1u, host_rgba8, n_bytes);
}

} // extern "C"
