// rt_temporal.h — the temporal pass's kernel and C-ABI (include/rsrt.h "temporal pass").  Included at the end of
// rsrt_api.hip, after rt_denoise.h.
//
//  rt_temporal_kernel  one thread a pixel, 64 x 4 workgroups like rt_dn_level_kernel: a wave is one row of 64 pixels, so its bilinear
//                      taps fall on about two rows of the previous frame.  It reads the sum (16 B), the AOV record (32 B) and up to 4
//                      taps of previous history and features (16 + 16 B each, mostly from the caches), and writes history and
//                      features (32 B): about 112 B of unique traffic a pixel.  No LDS.  The per-pixel arithmetic is
//                      include/rsrt_temporal.h.
//  rt_temporal_moments_kernel  the same pass with the luminance moments (RSRT_TEMPORAL_MOMENTS): one float4 record more a pixel, read
//                      through the same taps and written.
#include "../../../include/rsrt_temporal.h"

// the previous frame's buffers, as rsrt_tp_pixel reads them
struct TpPrev {
    const float4 *c_, *f_;
    __host__ __device__ void col(unsigned q, float o[4]) const
    {
        const float4 v = c_[q];
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    __host__ __device__ void feat(unsigned q, float o[4]) const
    {
        const float4 v = f_[q];
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
};

__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_temporal_kernel(rsrt_tp_frame fr, const float4 *accum, const float4 *aov, const float4 *prev_col,
                                                                          const float4 *prev_feat, float4 *out_col, float4 *out_feat)
{
    const int x = (int)(blockIdx.x * RT_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RT_DN_BY + threadIdx.y);
    if (x >= (int)fr.width || y >= (int)fr.height) return;
    const size_t p = (size_t)y * fr.width + (size_t)x;
    const float4 s = accum[p];
    const float sum[3] = {s.x, s.y, s.z};
    float a[8], o[4], f[4];
    dn_aov(aov, p, a);
    rsrt_tp_pixel(&fr, TpPrev{prev_col, prev_feat}, x, y, sum, a, o, f);
    out_col[p] = make_float4(o[0], o[1], o[2], o[3]);
    out_feat[p] = make_float4(f[0], f[1], f[2], f[3]);
}

// the previous frame's buffers and moment records, as rsrt_tp_pixel_moments reads them
struct TpPrevM : TpPrev {
    const float4 *m_;
    __host__ __device__ void mom(unsigned q, float o[4]) const
    {
        const float4 v = m_[q];
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
};

// rt_temporal_kernel plus the luminance moments (RSRT_TEMPORAL_MOMENTS): 16 B more read (the previous record, per valid tap, mostly from
// the caches) and 16 B more written a pixel.  History and features are the plain kernel's, bit for bit.
__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_temporal_moments_kernel(rsrt_tp_frame fr, const float4 *accum, const float4 *aov,
                                                                                  const float4 *prev_col, const float4 *prev_feat,
                                                                                  const float4 *prev_mom, float4 *out_col, float4 *out_feat,
                                                                                  float4 *out_mom)
{
    const int x = (int)(blockIdx.x * RT_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RT_DN_BY + threadIdx.y);
    if (x >= (int)fr.width || y >= (int)fr.height) return;
    const size_t p = (size_t)y * fr.width + (size_t)x;
    const float4 s = accum[p];
    const float sum[3] = {s.x, s.y, s.z};
    float a[8], o[4], f[4], m[4];
    dn_aov(aov, p, a);
    TpPrevM prev;
    prev.c_ = prev_col;
    prev.f_ = prev_feat;
    prev.m_ = prev_mom;
    rsrt_tp_pixel_moments(&fr, prev, x, y, sum, a, o, f, m);
    out_col[p] = make_float4(o[0], o[1], o[2], o[3]);
    out_feat[p] = make_float4(f[0], f[1], f[2], f[3]);
    out_mom[p] = make_float4(m[0], m[1], m[2], m[3]);
}

namespace {

void tp_camera_of(const float c[13], rsrt_tp_camera *out) { rsrt_tp_camera_init(out, c, c + 3, c[12]); }

} // namespace

extern "C" {

rsrt_status rsrt_temporal_accumulate(rsrt_context *ctx, const rsrt_camera *camera, uint32_t sample_total, uint32_t aov_sample_total,
                                     const rsrt_temporal_params *params, void *hip_stream)
{
    return rsrt_temporal_accumulate_ex(ctx, camera, sample_total, aov_sample_total, params, 0u, hip_stream);
}

rsrt_status rsrt_temporal_accumulate_ex(rsrt_context *ctx, const rsrt_camera *camera, uint32_t sample_total, uint32_t aov_sample_total,
                                        const rsrt_temporal_params *params, uint32_t flags, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (flags & ~(uint32_t)RSRT_TEMPORAL_MOMENTS) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: unknown flags 0x%x", flags);
    const bool moments = (flags & RSRT_TEMPORAL_MOMENTS) != 0;
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: camera is NULL");
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: params is NULL");
    rsrt_status st = whole_frame(ctx, "temporal");
    if (st || (st = accumulator_and_aov(ctx, "temporal"))) return st;
    const rsrt_temporal_params &p = *params;
    if (p.max_history < 1u || p.max_history > (1u << 24))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: max_history %u (1 .. 2^24)", p.max_history);
    if (!(p.depth_tolerance >= 1.0e-6f && p.depth_tolerance <= 1.0e6f))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: depth_tolerance must lie in [1e-6, 1e6]");
    if (!(p.normal_tolerance >= -1.0f && p.normal_tolerance <= 1.0f))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: normal_tolerance must lie in [-1, 1]");
    if (sample_total == 0 || aov_sample_total == 0)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "temporal: sample_total and aov_sample_total must be > 0");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const uint32_t w = ctx->acc.w, h = ctx->acc.h;
    const size_t n = (size_t)w * h;
    // history 0, history 1, features 0, features 1 (float4 each), and on the first MOMENTS frame the two moment buffers (float4 each).  A new
    // allocation starts without history: accumulator_size_changed() dropped it with the old one
    if ((st = ensure_sized(ctx, ctx->tp_hist, w, h, 4u * sizeof(float4))) || (moments && (st = ensure_sized(ctx, ctx->tp_mom, w, h, 2u * sizeof(float4)))) ||
        (st = begin_work(ctx, stream)))
        return st;
    float cam[13];
    memcpy(cam, camera->pos, 12);
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) cam[3 + 3 * j + k] = camera->rot_transform[j][k];
    cam[12] = camera->fov_y;
    rsrt_tp_frame fr;
    memset(&fr, 0, sizeof fr);
    tp_camera_of(cam, &fr.cur);
    tp_camera_of(ctx->tp_frames ? ctx->tp_cam : cam, &fr.prev);
    fr.width = w;
    fr.height = h;
    fr.sample_total = (float)sample_total;
    fr.aov_sample_total = (float)aov_sample_total;
    fr.max_history = (float)p.max_history;
    fr.depth_tolerance = p.depth_tolerance;
    fr.normal_tolerance = p.normal_tolerance;
    fr.aspect = (float)w / (float)h;
    fr.has_prev = ctx->tp_frames > 0 && ctx->tp_moments == (moments ? 1u : 0u); // (a MOMENTS toggle drops the history)
    fr.identity = fr.has_prev && rsrt_tp_same_camera(&fr.cur, &fr.prev); // (a resize frees the buffers, so W and H are the previous frame's)
    const uint32_t src = ctx->tp_cur, dst = src ^ 1u;
    float4 *hist = static_cast<float4 *>(ctx->tp_hist.p), *feat = hist + 2u * n, *mom = static_cast<float4 *>(ctx->tp_mom.p);
    const dim3 grid((w + RT_DN_BX - 1) / RT_DN_BX, (h + RT_DN_BY - 1) / RT_DN_BY), block(RT_DN_BX, RT_DN_BY);
    if (moments)
        rt_temporal_moments_kernel<<<grid, block, 0, stream>>>(fr, ctx->acc.p, ctx->aov.p, hist + src * n, feat + src * n, mom + src * n,
                                                               hist + dst * n, feat + dst * n, mom + dst * n);
    else
        rt_temporal_kernel<<<grid, block, 0, stream>>>(fr, ctx->acc.p, ctx->aov.p, hist + src * n, feat + src * n, hist + dst * n, feat + dst * n);
    HIP_TRY(ctx, hipGetLastError());
    ctx->tp_cur = dst;
    ctx->tp_frames++;
    ctx->tp_moments = moments ? 1u : 0u;
    memcpy(ctx->tp_cam, cam, sizeof cam);
    return end_work(ctx, stream);
}

rsrt_status rsrt_temporal_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    ctx->tp_frames = 0;
    return RSRT_OK;
}

rsrt_status rsrt_temporal_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return image_download(ctx, "temporal_download", IMAGE_TEMPORAL, host, n_floats);
}

rsrt_status rsrt_temporal_moments_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->tp_hist.p || !ctx->tp_frames || !ctx->tp_moments || !ctx->tp_mom.p)
        return fail(ctx, RSRT_ERR_NOT_READY, "the last temporal frame carried no moments (rsrt_temporal_accumulate_ex with RSRT_TEMPORAL_MOMENTS first)");
    return download_floats(ctx, "temporal_moments_download", temporal_moments(ctx), ctx->tp_hist.pixels() * 4u, host, n_floats);
}

} // extern "C"
