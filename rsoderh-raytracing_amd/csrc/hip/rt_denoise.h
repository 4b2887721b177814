// rt_denoise.h — the denoiser's kernels and C-ABI (include/rsrt.h "denoiser").  Included at the end of rsrt_api.hip.
//
//  rt_aov_kernel        the AOV pass: every pixel casts the camera rays rsrt_render casts for its samples (start_path), takes each
//                       one's closest hit exactly as the ray-query probe's mode 0 does (threaded tree walk, then the brute-force
//                       fallback) and adds material colour / 1 / normal / distance to its 8-float record, in sample order.
//  rt_dn_prepare_kernel the filter's input: demodulated mean colour (float4) and the packed guide features (4 x binary16: mean
//                       normal, mean distance), or the plain mean when no level is run.
//  rt_dn_level_kernel   one a-trous level: 25 taps of step 2^i.  A wave is one row of 64 pixels, so each tap row is a 1 KiB
//                       contiguous float4 read plus 512 B of features; the 24 bytes a tap reads come from the caches (a 1080p
//                       level reads 50 MB of unique data and writes 33 MB; its 25 taps request 1.24 GB).  Measured on house
//                       1920x1080 (profiles/denoise_house_1080p.json): 87 us a level, 22 us the prepare pass, 0.46 ms for five
//                       levels.  The per-pixel arithmetic is include/rsrt_denoise.h.
#include "../../../include/rsrt_denoise.h"

#define RT_DN_BX 64 // level kernel: a workgroup is 64 x 4 pixels, a wave one row of it
#define RT_DN_BY 4

// closest hit of one ray as rsrt_cast_rays mode 0 computes it (rt_cast_rays_kernel, TRAV 0)
template <class View>
__device__ __forceinline__ void aov_closest_hit(const View &S, const DevScene &sc, V3 o, V3 d, Hit &h)
{
#ifdef RT_INSTRUMENT
    DbgCounters dbg;
#endif
    h.t = RT_INFINITY; h.ref = 0; h.src = SRC_BVH; h.u = h.v = 0.0f;
    uint32_t cur = 0, work = 0;
    unsigned long long flat_rem = 0ull;
    uint32_t wmem[RT_WSTATE_WORDS];
    while (cur != RT_END) trace_dispatch<0>(DBG_ARG S, sc, o, d, false, false, 12u, 50u, cur, h, nullptr, work, flat_rem, wmem, 1u, 60u);
    if (h.did_hit()) hit_barycentrics(S, h, o, d);
    if (!h.did_hit()) { // cast_ray's brute-force fallback
        for (uint32_t k = 0; k < sc.n_spheres; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_SPHERE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_SPHERE; }
        }
        for (uint32_t k = 0; k < sc.n_planes; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_PLANE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_PLANE; }
        }
    }
}

// SV 1: the whole scene image in LDS (staged once per workgroup; the grid is a few workgroups per CU that stride over the frame)
template <int SV>
__global__ __launch_bounds__(RT_BLOCK) void rt_aov_kernel(RenderParams P, float4 *aov)
{
    const DevScene &sc = P.scene;
    if (SV != 0) stage_scene_lds(sc);
    const typename PoolView<SV>::type S = PoolView<SV>::make(sc);
    const uint32_t n = P.width * P.height;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t px = i % P.width, py = i / P.width;
        float4 a0 = aov[2u * (size_t)i], a1 = aov[2u * (size_t)i + 1u];
        for (uint32_t k = 0; k < P.sample_count; k++) {
            PathState s;
            start_path(P, px, py, P.sample_begin + k, s);
            Hit h;
            aov_closest_hit(S, sc, s.o, s.d, h);
            if (!h.did_hit()) continue;
            const Surface f = resolve_hit(S, h, s.o, s.d);
            const float4 m = S.mat(4u * f.material_id); // rsrt_material.color
            a0.x = a0.x + m.x; a0.y = a0.y + m.y; a0.z = a0.z + m.z; a0.w = a0.w + 1.0f;
            a1.x = a1.x + f.normal.x; a1.y = a1.y + f.normal.y; a1.z = a1.z + f.normal.z; a1.w = a1.w + h.t;
        }
        aov[2u * (size_t)i] = a0;
        aov[2u * (size_t)i + 1u] = a1;
    }
}

__device__ __forceinline__ void dn_aov(const float4 *aov, size_t i, float r[8])
{
    const float4 a0 = aov[2u * i], a1 = aov[2u * i + 1u];
    r[0] = a0.x; r[1] = a0.y; r[2] = a0.z; r[3] = a0.w; r[4] = a1.x; r[5] = a1.y; r[6] = a1.z; r[7] = a1.w;
}
__device__ __forceinline__ unsigned short dn_h(float x) { return __half_as_ushort(__float2half_rn(x)); }
__device__ __forceinline__ float dn_f(unsigned short x) { return __half2float(__ushort_as_half(x)); }

// passthrough (no level to run): out = sum / sample_total, alpha 1
__global__ void rt_dn_prepare_kernel(const float4 *accum, const float4 *aov, size_t n, float sample_total, float aov_total, int demodulate,
                                     int passthrough, float4 *r_out, ushort4 *feat)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = accum[i];
    if (passthrough) { r_out[i] = make_float4(s.x / sample_total, s.y / sample_total, s.z / sample_total, 1.0f); return; }
    const float sum[3] = {s.x, s.y, s.z};
    float a[8], r[3], f[4];
    dn_aov(aov, i, a);
    rsrt_dn_prepare(sum, sample_total, a, aov_total, demodulate, r);
    rsrt_dn_features(a, aov_total, f);
    r_out[i] = make_float4(r[0], r[1], r[2], 1.0f);
    feat[i] = make_ushort4(dn_h(f[0]), dn_h(f[1]), dn_h(f[2]), dn_h(f[3]));
}

// one level; LAST: remodulate (demodulate != 0) and write the output
template <bool LAST>
__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_dn_level_kernel(const float4 *src, const ushort4 *feat, const float4 *aov, float4 *dst,
                                                                          uint32_t w, uint32_t h, uint32_t level, float sigma_c, float sigma_n,
                                                                          float sigma_z, float aov_total, int demodulate)
{
    const int x = (int)(blockIdx.x * RT_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RT_DN_BY + threadIdx.y);
    if (x >= (int)w || y >= (int)h) return;
    const size_t p = (size_t)y * w + (size_t)x;
    const float4 c = src[p];
    const ushort4 g = feat[p];
    const float rp[3] = {c.x, c.y, c.z}, fp[4] = {dn_f(g.x), dn_f(g.y), dn_f(g.z), dn_f(g.w)};
    const float kc = rsrt_dn_kc(sigma_c, level), kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
    const int step = 1 << level;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= (int)h) continue;
        const float4 *srow = src + (size_t)qy * w;
        const ushort4 *frow = feat + (size_t)qy * w;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= (int)w) continue;
            const float4 cq = srow[qx];
            const ushort4 gq = frow[qx];
            const float rq[3] = {cq.x, cq.y, cq.z}, fq[4] = {dn_f(gq.x), dn_f(gq.y), dn_f(gq.z), dn_f(gq.w)};
            rsrt_dn_tap(rsrt_dn_b3(dx) * rsrt_dn_b3(dy), rp, fp, kc, kn, kz, rq, fq, acc);
        }
    }
    float a[3] = {1.0f, 1.0f, 1.0f}, out[3];
    if (LAST && demodulate) {
        float r[8];
        dn_aov(aov, p, r);
        rsrt_dn_albedo(r, aov_total, a);
    }
    rsrt_dn_finish(acc, a, LAST && demodulate, out);
    dst[p] = make_float4(out[0], out[1], out[2], 1.0f);
}

namespace {

// the AOV pass of samples [sample_begin, sample_begin + sample_count) into `aov`, a width x height record buffer (the AOV buffer, or the
// upsampler's guide: rt_upsample.h)
rsrt_status launch_aov(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin, uint32_t sample_count,
                       float4 *aov, hipStream_t stream)
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
    const void *kfn = lds ? reinterpret_cast<const void *>(&rt_aov_kernel<1>) : reinterpret_cast<const void *>(&rt_aov_kernel<0>);
    if (lds) HIP_TRY(ctx, hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const uint64_t n = (uint64_t)width * height;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + RT_BLOCK - 1) / RT_BLOCK, (uint64_t)ctx->cus * 8u);
    rsrt_status st = begin_work(ctx, stream);
    if (st) return st;
    void *kargs[] = {&P, &aov};
    HIP_TRY(ctx, hipLaunchKernel(kfn, dim3(blocks), dim3(RT_BLOCK), kargs, smem, stream));
    return end_work(ctx, stream);
}

bool sigma_ok(float s) { return s >= 1.0e-6f && s <= 1.0e6f; }

// the clamp / variance pass and the L >= 1 levels after rt_dn_prepare_kernel wrote ping and feat (rt_variance.h)
void sv_filter(rsrt_context *ctx, hipStream_t stream, const rsrt_denoise_params &p, bool temporal, float4 *ping, float4 *pong, const ushort4 *feat,
               float4 *out, uint32_t w, uint32_t h, float aov_total);

} // namespace

extern "C" {

rsrt_status rsrt_aov_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                            uint32_t sample_count, uint32_t flags, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if (flags != 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "aov_render: flags must be 0");
    rsrt_status st = whole_frame(ctx, "aov_render");
    if (st) return st;
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", width, height);
    if ((uint64_t)sample_begin + sample_count > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "sample range overflows u32");
    if ((st = ensure_accumulator(ctx, width, height)) || (st = buffer_ensure(ctx, ctx->aov, width, height))) return st; // (the AOV buffer follows the accumulator)
    if (sample_count == 0) return RSRT_OK;
    return launch_aov(ctx, camera, width, height, sample_begin, sample_count, ctx->aov.p, stream_of(ctx, hip_stream));
}

rsrt_status rsrt_aov_bind(rsrt_context *ctx, void *device_f32x8, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_bind(ctx, ctx->aov, device_f32x8, width, height);
}

rsrt_status rsrt_aov_clear(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_clear(ctx, ctx->aov);
}

rsrt_status rsrt_aov_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_download(ctx, "aov_download", ctx->aov, host, n_floats);
}

rsrt_status rsrt_denoise(rsrt_context *ctx, uint32_t sample_total, uint32_t aov_sample_total, const rsrt_denoise_params *params,
                         void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: params is NULL");
    rsrt_status st = whole_frame(ctx, "denoise");
    if (st || (st = accumulator_and_aov(ctx, "denoise"))) return st;
    const rsrt_denoise_params &p = *params;
    if (p.iterations > 8u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: iterations %u (at most 8)", p.iterations);
    if (p.flags & ~(uint32_t)(RSRT_DENOISE_DEMODULATE | RSRT_DENOISE_TEMPORAL | RSRT_DENOISE_VARIANCE | RSRT_DENOISE_CLAMP))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: unknown flags 0x%x", p.flags);
    if ((p.flags & RSRT_DENOISE_VARIANCE) && !(p.flags & RSRT_DENOISE_DEMODULATE))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: RSRT_DENOISE_VARIANCE requires RSRT_DENOISE_DEMODULATE");
    const bool temporal = (p.flags & RSRT_DENOISE_TEMPORAL) != 0; // the temporal pass's colour (its weight channel is ignored), sample_total 1
    if (temporal) sample_total = 1u;
    if (!sigma_ok(p.sigma_color) || !sigma_ok(p.sigma_normal) || !sigma_ok(p.sigma_depth))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: sigmas must lie in [1e-6, 1e6]");
    if (sample_total == 0 || aov_sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: sample_total and aov_sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "denoise: output pointer must be 16-byte aligned");
    ImageView colour;
    if ((st = resolve_image(ctx, "denoise", "denoise: ", temporal ? IMAGE_TEMPORAL : IMAGE_MEAN, sample_total, true, &colour))) return st;
    if (temporal && (p.flags & RSRT_DENOISE_VARIANCE) && !ctx->tp_moments)
        return fail(ctx, RSRT_ERR_NOT_READY, "denoise: the last temporal frame carried no moments (RSRT_TEMPORAL_MOMENTS)");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const uint32_t w = ctx->acc.w, h = ctx->acc.h;
    const size_t n = (size_t)w * h;
    // ping, pong, the library-owned output (float4 each) and the packed features (ushort4)
    if ((st = ensure_sized(ctx, ctx->dn_scratch, w, h, 3u * sizeof(float4) + sizeof(ushort4))) || (st = begin_work(ctx, stream))) return st;
    float4 *ping = static_cast<float4 *>(ctx->dn_scratch.p), *pong = ping + n, *own = pong + n;
    ushort4 *feat = reinterpret_cast<ushort4 *>(own + n);
    float4 *out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : own;
    const float at_f = (float)aov_sample_total;
    const int demod = (p.flags & RSRT_DENOISE_DEMODULATE) ? 1 : 0;
    const uint32_t L = p.iterations;
    rt_dn_prepare_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(colour.img, ctx->aov.p, n, colour.total, at_f, demod, L == 0, L == 0 ? out : ping, feat);
    const dim3 grid((w + RT_DN_BX - 1) / RT_DN_BX, (h + RT_DN_BY - 1) / RT_DN_BY), block(RT_DN_BX, RT_DN_BY);
    if (L > 0 && (p.flags & (RSRT_DENOISE_VARIANCE | RSRT_DENOISE_CLAMP))) {
        sv_filter(ctx, stream, p, temporal, ping, pong, feat, out, w, h, at_f);
    } else {
        for (uint32_t i = 0; i < L; i++) {
            const float4 *src = (i % 2u == 0u) ? ping : pong;
            if (i + 1u == L)
                rt_dn_level_kernel<true><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, out, w, h, i, p.sigma_color, p.sigma_normal, p.sigma_depth, at_f, demod);
            else
                rt_dn_level_kernel<false><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, (i % 2u == 0u) ? pong : ping, w, h, i, p.sigma_color,
                                                                      p.sigma_normal, p.sigma_depth, at_f, demod);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    ctx->dn_last = out;
    return end_work(ctx, stream);
}

rsrt_status rsrt_denoised_download(rsrt_context *ctx, float *host, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return image_download(ctx, "denoised_download", IMAGE_DENOISED, host, n_floats);
}

rsrt_status rsrt_denoised_display_srgb8(rsrt_context *ctx, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    return image_display(ctx, "denoised_display_srgb8", IMAGE_DENOISED, 1u, host_rgba8, n_bytes);
}

} // extern "C"
