// rt_fog.h — the volumetric fog pass's kernels and their C-ABI (include/rsrt.h "volumetric fog").  Included at the end
// of rsrt_api.hip.  All arithmetic is include/rsrt_fog.h's.
//
//  rt_fog_kernel          the march, in rt_aov_kernel's shape: the scene view is chosen by lds_float4s (the whole image staged in LDS, or
//                         global memory), a few workgroups per CU stride over the frame, one lane is one pixel.  Per sample: start_path's
//                         camera ray, the draw after it, the closest hit (aov_closest_hit), the phase term and delta.  Per step: the
//                         point, one exp2 and the shadow walk — the threaded tree walk with the any-hit exit, which answers "hit or
//                         not" as the full walk does because the walk never prunes.  Every lane of a wave runs sample_count x steps
//                         trips; the walks inside differ in length.  16 B read and written a pixel.  No scratch memory.
//  rt_fog_compose_kernel  one thread a pixel: out = colour * mean transmittance + mean inscatter.  32 B read, 16 B written a pixel.
//  rt_fog_source_kernel   the rebuild's pass over the LOW records (arithmetic in include/rsrt_fog_upsample.h): one thread a
//                         low pixel, record -> mean inscatter / (1 - mean transmittance).  16 B read and written a low pixel.
//  rt_fog_rebuild_kernel  one thread an output pixel: 16 B of source and 32 B of first-hit record read, nine source terms of the low frame
//                         (plain global loads; neighbouring lanes share them, about 4 B a pixel of new traffic at half size), the
//                         pixel's own transmittance from its first hit, 16 B written.
#include "../../../include/rsrt_fog.h"
#include "../../../include/rsrt_fog_upsample.h"

// does the ray (o, d) hit anything the tree holds: rsrt_cast_rays mode 1's did_hit (cast_ray_bvh alone, no fallback)
template <class View>
__device__ __forceinline__ bool fog_occluded(const View &S, const DevScene &sc, V3 o, V3 d)
{
#ifdef RT_INSTRUMENT
    DbgCounters dbg;
#endif
    Hit h;
    h.t = RT_INFINITY; h.ref = 0; h.src = SRC_BVH; h.u = h.v = 0.0f;
    uint32_t cur = 0, work = 0;
    unsigned long long flat_rem = 0ull;
    while (cur != RT_END) trace_dispatch<0>(DBG_ARG S, sc, o, d, false, true, 0xffffffffu, 50u, cur, h, nullptr, work, flat_rem, nullptr, 1u, 60u);
    return h.did_hit();
}

template <int SV>
__global__ __launch_bounds__(RT_BLOCK) void rt_fog_kernel(RenderParams P, rsrt_fog_constants K, float4 *rec)
{
    const DevScene &sc = P.scene;
    if (SV != 0) stage_scene_lds(sc);
    const typename PoolView<SV>::type S = PoolView<SV>::make(sc);
    const uint32_t n = P.width * P.height;
    const V3 ld = v3(K.light_dir[0], K.light_dir[1], K.light_dir[2]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t px = i % P.width, py = i / P.width;
        const float4 r0 = rec[i];
        float r[4] = {r0.x, r0.y, r0.z, r0.w};
        for (uint32_t k = 0; k < P.sample_count; k++) {
            PathState s;
            start_path(P, px, py, P.sample_begin + k, s);
            const float xi = (K.flags & RSRT_FOG_JITTER) ? random_uniform(s.rng) : 0.5f;
            Hit h;
            aov_closest_hit(S, sc, s.o, s.d, h);
            const float o[3] = {s.o.x, s.o.y, s.o.z}, d[3] = {s.d.x, s.d.y, s.d.z};
            const float L = rsrt_fog_segment(&K, h.did_hit(), h.t), delta = rsrt_fog_delta(&K, L);
            float s_sun[3], sum[3] = {0.0f, 0.0f, 0.0f};
            rsrt_fog_sun(&K, rsrt_fog_phase(&K, rsrt_fog_cos_theta(&K, d)), s_sun);
            for (uint32_t j = 0; j < K.steps; j++) {
                const float t = rsrt_fog_t(j, xi, delta);
                float x[3];
                rsrt_fog_point(o, d, t, x);
                const bool lit = !fog_occluded(S, sc, v3(x[0], x[1], x[2]), ld);
                rsrt_fog_step(&K, sum, rsrt_fog_transmittance(&K, t), lit, s_sun);
            }
            rsrt_fog_record(&K, r, sum, delta, L);
        }
        rec[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// img: sums of `total` samples (1: a colour); rec: the fog records of the same size, of n samples
__global__ __launch_bounds__(256) void rt_fog_compose_kernel(const float4 *img, float total, const float4 *rec, float n, size_t count, float4 *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float4 s = img[i], q = rec[i];
    const float c[3] = {s.x / total, s.y / total, s.z / total}, r[4] = {q.x, q.y, q.z, q.w};
    float o[3];
    rsrt_fog_compose(c, r, n, o);
    out[i] = make_float4(o[0], o[1], o[2], 1.0f);
}

// rec: the low fog records, of n samples; src: their demodulated form
__global__ __launch_bounds__(256) void rt_fog_source_kernel(const float4 *rec, float n, size_t count, float4 *src)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float4 q = rec[i];
    const float r[4] = {q.x, q.y, q.z, q.w};
    float s[3];
    rsrt_fogup_source(r, n, s);
    src[i] = make_float4(s[0], s[1], s[2], 0.0f);
}

// img: sums of `total` samples, W x H; g: the first-hit records of the same size, of g_total samples; src: rt_fog_source_kernel's, w x h
__global__ __launch_bounds__(256) void rt_fog_rebuild_kernel(const float4 *img, float total, const float4 *g, float g_total, const float4 *src, uint32_t w,
                                                             uint32_t h, uint32_t W, uint32_t H, rsrt_fog_constants K, float4 *out)
{
    const size_t P = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (P >= (size_t)W * H) return;
    const uint32_t X = (uint32_t)(P % W), Y = (uint32_t)(P / W);
    const float u = rsrt_up_coord(X, w, W), v = rsrt_up_coord(Y, h, H);
    const int xn = rsrt_up_nearest(u), yn = rsrt_up_nearest(v);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = yn + dy;
        if (qy < 0 || qy >= (int)h) continue;
        const float hy = rsrt_up_tent(qy, v);
        const float4 *row = src + (size_t)qy * w;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = xn + dx;
            if (qx < 0 || qx >= (int)w) continue;
            const float hx = rsrt_up_tent(qx, u);
            const float4 c = row[qx];
            const float sq[3] = {c.x, c.y, c.z};
            rsrt_fogup_tap(hx * hy, sq, acc);
        }
    }
    float a[8], o[3];
    dn_aov(g, P, a);
    const float4 s = img[P];
    const float colour[3] = {s.x / total, s.y / total, s.z / total};
    rsrt_fogup_finish(colour, acc, rsrt_fogup_tau(&K, a, g_total), o);
    out[P] = make_float4(o[0], o[1], o[2], 1.0f);
}

namespace {

rsrt_status launch_fog(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin, uint32_t sample_count,
                       const rsrt_fog_constants &K, float4 *rec, hipStream_t stream)
{
    RenderParams P;
    memset(&P, 0, sizeof P);
    P.scene = ctx->scene;
    memcpy(P.cam_pos, camera->pos, 12);
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) P.cam_rot[3 * j + k] = camera->rot_transform[j][k];
    P.fov_y = camera->fov_y;
    P.width = width; P.height = height;
    P.sample_begin = sample_begin; P.sample_count = sample_count;
    const bool lds = P.scene.lds_float4s != 0;
    const size_t smem = lds ? (size_t)P.scene.lds_float4s * sizeof(float4) : 0u;
    const void *kfn = lds ? reinterpret_cast<const void *>(&rt_fog_kernel<1>) : reinterpret_cast<const void *>(&rt_fog_kernel<0>);
    if (lds) HIP_TRY(ctx, hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const uint64_t n = (uint64_t)width * height;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + RT_BLOCK - 1) / RT_BLOCK, (uint64_t)ctx->cus * 8u);
    rsrt_status st = begin_work(ctx, stream);
    if (st) return st;
    rsrt_fog_constants k = K;
    void *kargs[] = {&P, &k, &rec};
    HIP_TRY(ctx, hipLaunchKernel(kfn, dim3(blocks), dim3(RT_BLOCK), kargs, smem, stream));
    return end_work(ctx, stream);
}

} // namespace

extern "C" {

rsrt_status rsrt_fog_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                            uint32_t sample_count, const rsrt_fog_params *params, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_render: camera is NULL");
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_render: params is NULL");
    rsrt_status st = whole_frame(ctx, "fog_render");
    if (st) return st;
    if (!rsrt_fog_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT,
                    "fog_render: want density in [0, 1e6] with density * max_distance finite, albedo in [0, 1], |anisotropy| <= 0.95, light_dir a unit "
                    "vector, light_irradiance and ambient finite and >= 0, max_distance finite and > 0, steps in 1..%u, flags 0 or RSRT_FOG_JITTER, "
                    "and one sample's sum and inscatter finite (rsrt_fog.h: density * albedo * (phase * light_irradiance + ambient), times steps and "
                    "times the march's length)",
                    RSRT_FOG_MAX_STEPS);
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", width, height);
    if ((uint64_t)sample_begin + sample_count > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "sample range overflows u32");
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if ((st = buffer_ensure(ctx, ctx->fog, width, height))) return st;
    if (sample_count == 0) return RSRT_OK;
    rsrt_fog_constants K;
    memset(&K, 0, sizeof K);
    rsrt_fog_prepare(params, &K);
    return launch_fog(ctx, camera, width, height, sample_begin, sample_count, K, ctx->fog.p, stream_of(ctx, hip_stream));
}

rsrt_status rsrt_fog_bind(rsrt_context *ctx, void *device_f32x4, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_bind(ctx, ctx->fog, device_f32x4, width, height);
}

rsrt_status rsrt_fog_clear(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_clear(ctx, ctx->fog);
}

rsrt_status rsrt_fog_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_download(ctx, "fog_download", ctx->fog, host, n_floats);
}

rsrt_status rsrt_fog_apply(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t fog_sample_total, void *device_out_rgba32f,
                           void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "fog_apply");
    if (st) return st;
    if (source == IMAGE_FOG) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: the fog image is not a source of its own pass");
    if (source == IMAGE_LENS || source == IMAGE_MOTION) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: the fog goes before the lens and the shutter (source %u)", source);
    if (source > IMAGE_FOG) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: unknown source %u", source);
    if (fog_sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: fog_sample_total must be > 0");
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: output pointer must be 16-byte aligned");
    if (!ctx->fog.p) return fail(ctx, RSRT_ERR_NOT_READY, "fog_apply: no fog records (rsrt_fog_render or rsrt_fog_bind first)");
    ImageView v;
    if ((st = resolve_image(ctx, "fog_apply", "fog_apply: ", source, sample_total, false, &v))) return st;
    if (ctx->fog.w != v.w || ctx->fog.h != v.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply: %s is %ux%u, the source %ux%u", ctx->fog.name, ctx->fog.w, ctx->fog.h, v.w, v.h);
    const hipStream_t stream = stream_of(ctx, hip_stream);
    // the library-owned output follows the size of the source the fog image was built from
    if (!device_out_rgba32f) {
        if (!ctx->fg_out.is(v.w, v.h) && ctx->fg_last.img == ctx->fg_out.p) ctx->fg_last = ImageView{}; // (the allocation that held the fog image goes)
        if ((st = ensure_sized(ctx, ctx->fg_out, v.w, v.h, sizeof(float4)))) return st;
    }
    if ((st = begin_work(ctx, stream))) return st;
    ctx->fg_last = ImageView{}; // (a failed launch leaves no fog image)
    const size_t n = v.pixels();
    float4 *const out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : static_cast<float4 *>(ctx->fg_out.p);
    rt_fog_compose_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(v.img, v.total, ctx->fog.p, (float)fog_sample_total, n, out);
    HIP_TRY(ctx, hipGetLastError());
    ctx->fg_last = ImageView{out, v.w, v.h, 1.0f};
    ctx->fg_rec = source == IMAGE_UPSAMPLED ? &ctx->guide : &ctx->aov;
    return end_work(ctx, stream);
}

rsrt_status rsrt_fog_apply_upsampled(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t fog_sample_total,
                                     uint32_t record_sample_total, const rsrt_fog_params *params, void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "fog_apply_upsampled");
    if (st) return st;
    if (source == IMAGE_FOG) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: the fog image is not a source of its own pass");
    if (source == IMAGE_LENS || source == IMAGE_MOTION) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: the fog goes before the lens and the shutter (source %u)", source);
    if (source > IMAGE_FOG) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: unknown source %u", source);
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: params is NULL");
    if (!rsrt_fog_params_ok(params)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: params are not ones rsrt_fog_render accepts");
    if (fog_sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: fog_sample_total must be > 0");
    if (record_sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: record_sample_total must be > 0");
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: output pointer must be 16-byte aligned");
    if (!ctx->fog.p) return fail(ctx, RSRT_ERR_NOT_READY, "fog_apply_upsampled: no fog records (rsrt_fog_render or rsrt_fog_bind first)");
    ImageView v;
    if ((st = resolve_image(ctx, "fog_apply_upsampled", "fog_apply_upsampled: ", source, sample_total, false, &v))) return st;
    // the first-hit records of the source's size: the guide for the upsampled image, the AOV buffer otherwise
    const PixelBuffer *const rec = source == IMAGE_UPSAMPLED ? &ctx->guide : &ctx->aov;
    if (!rec->p) return fail(ctx, RSRT_ERR_NOT_READY, "fog_apply_upsampled: no %s", rec->name);
    if (rec->w != v.w || rec->h != v.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: %s is %ux%u, the source %ux%u", rec->name, rec->w, rec->h, v.w, v.h);
    if (ctx->fog.w > v.w || ctx->fog.h > v.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "fog_apply_upsampled: %s is %ux%u, larger than the source %ux%u", ctx->fog.name, ctx->fog.w, ctx->fog.h, v.w, v.h);
    const hipStream_t stream = stream_of(ctx, hip_stream);
    if ((st = ensure_sized(ctx, ctx->fg_src, ctx->fog.w, ctx->fog.h, sizeof(float4)))) return st;
    if (!device_out_rgba32f) {
        if (!ctx->fg_out.is(v.w, v.h) && ctx->fg_last.img == ctx->fg_out.p) ctx->fg_last = ImageView{}; // (the allocation that held the fog image goes)
        if ((st = ensure_sized(ctx, ctx->fg_out, v.w, v.h, sizeof(float4)))) return st;
    }
    if ((st = begin_work(ctx, stream))) return st;
    ctx->fg_last = ImageView{}; // (a failed launch leaves no fog image)
    rsrt_fog_constants K;
    memset(&K, 0, sizeof K);
    rsrt_fog_prepare(params, &K);
    const size_t n = v.pixels(), low = ctx->fog.pixels();
    float4 *const src = static_cast<float4 *>(ctx->fg_src.p);
    float4 *const out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : static_cast<float4 *>(ctx->fg_out.p);
    rt_fog_source_kernel<<<dim3((unsigned)((low + 255) / 256)), dim3(256), 0, stream>>>(ctx->fog.p, (float)fog_sample_total, low, src);
    rt_fog_rebuild_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(v.img, v.total, rec->p, (float)record_sample_total, src, ctx->fog.w, ctx->fog.h,
                                                                                     v.w, v.h, K, out);
    HIP_TRY(ctx, hipGetLastError());
    ctx->fg_last = ImageView{out, v.w, v.h, 1.0f};
    ctx->fg_rec = rec;
    return end_work(ctx, stream);
}

rsrt_status rsrt_fog_image_download(rsrt_context *ctx, float *host_rgba, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "fog_image_download"); if (st0) return st0; }
    return image_download(ctx, "fog_image_download", IMAGE_FOG, host_rgba, n_floats);
}

rsrt_status rsrt_fog_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "fog_reset"); if (st0) return st0; }
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    ctx->fg_last = ImageView{};
    release(ctx->fg_out);
    release(ctx->fg_src);
    ctx->fog.p = nullptr; // a bound buffer is the caller's again; the library's own goes
    (void)hipFree(ctx->fog.owned);
    ctx->fog.owned = nullptr;
    ctx->fog.w = ctx->fog.h = 0;
    return RSRT_OK;
}

} // extern "C"
