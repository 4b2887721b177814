// rt_dof.h — the depth-of-field pass's kernels and their C-ABI (include/rsrt.h "depth of field").  Included at the end
// of rsrt_api.hip.  All arithmetic is include/rsrt_dof.h's.
//
//  rt_dof_prepare_kernel  one thread a pixel: the source's sum, the first-hit record and the camera -> the prepared texel (colour, signed
//                         blur radius).  48 B read, 16 B written a pixel.
//  rt_dof_gather_kernel   the lens blur.  A 256-thread workgroup makes a tile of RT_DOF_TW x RT_DOF_TH outputs.  It stages the tile and
//                         a halo of max_radius prepared texels in LDS (16 B a lane and load, all of a lane's loads issued before the
//                         first is used; a texel outside the frame is staged as radius 0, which has k == 0 at every distance >= 1 and is
//                         skipped like the header's) with each texel's area weight beside it (one division a staged texel, none a tap),
//                         takes the largest ceil(|r|) among them as the workgroup's loop bound — a tile wholly in focus reads one tap a
//                         pixel — and runs the tap loop from LDS.  (TW + 2 R) x (TH + 2 R) x 20 B of dynamic LDS: 45 KB at radius
//                         16, 20 KB at radius 8.  The tap distance is a scalar load from the table.  No scratch memory.
#include "../../../include/rsrt_dof.h"

#define RT_DOF_TW 16
#define RT_DOF_TH 16
#define RT_DOF_BLOCK (RT_DOF_TW * RT_DOF_TH)
#define RT_DOF_MAX_STAGED ((RT_DOF_TW + 2 * RSRT_DOF_MAX_RADIUS) * (RT_DOF_TH + 2 * RSRT_DOF_MAX_RADIUS))
#define RT_DOF_LOADS ((RT_DOF_MAX_STAGED + RT_DOF_BLOCK - 1) / RT_DOF_BLOCK) // loads in flight a lane, at most

// img: sums of fr.total samples; rec: the first-hit records of the same size (2 float4 a pixel)
__global__ __launch_bounds__(256) void rt_dof_prepare_kernel(rsrt_dof_frame fr, const float4 *img, const float4 *rec, rsrt_dof_texel *prep)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)fr.width * (size_t)fr.height) return;
    const float4 s = img[i];
    const float sum[3] = {s.x, s.y, s.z};
    float a[8];
    dn_aov(rec, i, a);
    prep[i] = rsrt_dof_prepare(&fr, (int)(i % (size_t)fr.width), (int)(i / (size_t)fr.width), sum, a);
}

// prep, out: w x h; R = max_radius in 1 .. RSRT_DOF_MAX_RADIUS; dynamic LDS: (TW + 2 R) (TH + 2 R) (sizeof(float4) + sizeof(float))
__global__ __launch_bounds__(RT_DOF_BLOCK) void rt_dof_gather_kernel(const float4 *prep, int w, int h, int R, float4 *out)
{
    extern __shared__ float4 rt_dof_lds[];
    __shared__ int bound;
    const int sw = RT_DOF_TW + 2 * R, n = sw * (RT_DOF_TH + 2 * R);
    float4 *const s = rt_dof_lds;                            // the staged texels: s[ty * sw + tx] is the texel (gx0 + tx, gy0 + ty)
    float *const sa = reinterpret_cast<float *>(s + n);      // ... and their area weights
    const int tid = (int)threadIdx.x, bx = (int)blockIdx.x * RT_DOF_TW, by = (int)blockIdx.y * RT_DOF_TH, gx0 = bx - R, gy0 = by - R;
    if (tid == 0) bound = 0;
    float4 c[RT_DOF_LOADS];
#pragma unroll
    for (int k = 0; k < RT_DOF_LOADS; k++) {
        const int i = k * RT_DOF_BLOCK + tid;
        if (i < n) {
            const int gx = gx0 + i % sw, gy = gy0 + i / sw;
            c[k] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? prep[(size_t)gy * (size_t)w + (size_t)gx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    __syncthreads(); // (bound is 0 before anyone raises it)
    int reach = 0;
#pragma unroll
    for (int k = 0; k < RT_DOF_LOADS; k++) {
        const int i = k * RT_DOF_BLOCK + tid;
        if (i < n) {
            s[i] = c[k];
            sa[i] = rsrt_dof_area(rsrt_dof_spread(c[k].w));
            const int m = rsrt_dof_ceil_abs(c[k].w);
            reach = m > reach ? m : reach;
        }
    }
    atomicMax(&bound, reach);
    __syncthreads();
    const int B = bound < R ? bound : R; // (|r| <= R already: the prepare step clamps)
    const int lx = tid % RT_DOF_TW, ly = tid / RT_DOF_TW, x = bx + lx, y = by + ly;
    if (x >= w || y >= h) return;
    const int at = (ly + R) * sw + lx + R;
    const float r_p = s[at].w, a_p = rsrt_dof_spread(r_p), w_p = sa[at];
    rsrt_dof_acc acc = RSRT_DOF_ACC_INIT;
    for (int dy = -B; dy <= B; dy++) {
        const int row = at + dy * sw;
#pragma unroll 4
        for (int dx = -B; dx <= B; dx++) {
            const float4 q = s[row + dx];
            rsrt_dof_tap(&acc, r_p, a_p, w_p, q.x, q.y, q.z, q.w, sa[row + dx], rsrt_dof_dist(dx, dy));
        }
    }
    out[(size_t)y * (size_t)w + (size_t)x] = make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, 1.0f);
}

namespace {

// the first-hit records `source` is blurred by: the AOV buffer (of the accumulator's size), for the upsampled image the guide, and for
// the fog image the ones of the image it was built from
rsrt_status dof_records(rsrt_context *ctx, const char *what, uint32_t source, const PixelBuffer **rec)
{
    if (source == IMAGE_LENS) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the lens image is not a source of its own pass", what);
    if (source == IMAGE_FOG) {
        if (!ctx->fg_last.img || !ctx->fg_rec) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no fog image (rsrt_fog_apply first)", what);
        if (!ctx->fg_rec->p) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no %s (the fog image was built from an image of its size)", what, ctx->fg_rec->name);
        *rec = ctx->fg_rec;
        return RSRT_OK;
    }
    if (source > IMAGE_LENS) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: unknown source %u", what, source);
    if (source == IMAGE_UPSAMPLED) {
        if (!ctx->guide.p) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no guide buffer (rsrt_guide_render or rsrt_guide_bind first)", what);
        *rec = &ctx->guide;
        return RSRT_OK;
    }
    const rsrt_status st = accumulator_and_aov(ctx, what);
    *rec = &ctx->aov;
    return st;
}

void dof_camera(const rsrt_camera *camera, float cam[13])
{
    memcpy(cam, camera->pos, 12);
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) cam[3 + 3 * j + k] = camera->rot_transform[j][k];
    cam[12] = camera->fov_y;
}

} // namespace

extern "C" {

rsrt_status rsrt_dof(rsrt_context *ctx, uint32_t source, uint32_t sample_total, const rsrt_camera *camera, const rsrt_dof_params *params,
                     void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "dof");
    if (st) return st;
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: camera is NULL");
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: params is NULL");
    if (!rsrt_dof_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: want focus_distance finite and > 0, aperture finite and >= 0, max_radius in 1..%d, flags 0", RSRT_DOF_MAX_RADIUS);
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: output pointer must be 16-byte aligned");
    const PixelBuffer *rec = nullptr;
    if ((st = dof_records(ctx, "dof", source, &rec))) return st;
    ImageView v;
    if ((st = resolve_image(ctx, "dof", "dof: ", source, sample_total, false, &v))) return st;
    if (rec->w != v.w || rec->h != v.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: %s is %ux%u, the source %ux%u", rec->name, rec->w, rec->h, v.w, v.h);
    if (v.w > 0x3fffffffu || v.h > 0x3fffffffu) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof: source too large");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    // the prepared texels and, unless the caller gave one, the output: two float4 a pixel of the source's size
    if (!ctx->df_buf.is(v.w, v.h)) ctx->df_last = ImageView{}; // (the allocation that held the lens image, or its radii, goes)
    if ((st = ensure_sized(ctx, ctx->df_buf, v.w, v.h, 2u * sizeof(float4)))) return st;
    if ((st = begin_work(ctx, stream))) return st;
    ctx->df_last = ImageView{}; // (a failed launch leaves no lens image)
    float cam[13];
    dof_camera(camera, cam);
    rsrt_dof_frame fr;
    memset(&fr, 0, sizeof fr);
    rsrt_dof_frame_init(&fr, cam, cam + 3, cam[12], v.w, v.h, v.total, params);
    const size_t n = v.pixels();
    float4 *const prep = static_cast<float4 *>(ctx->df_buf.p);
    float4 *const out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : prep + n;
    rt_dof_prepare_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(fr, v.img, rec->p, reinterpret_cast<rsrt_dof_texel *>(prep));
    const int R = (int)params->max_radius;
    const size_t lds = (size_t)(RT_DOF_TW + 2 * R) * (size_t)(RT_DOF_TH + 2 * R) * (sizeof(float4) + sizeof(float));
    rt_dof_gather_kernel<<<dim3((v.w + RT_DOF_TW - 1u) / RT_DOF_TW, (v.h + RT_DOF_TH - 1u) / RT_DOF_TH), dim3(RT_DOF_BLOCK), lds, stream>>>(prep, (int)v.w, (int)v.h,
                                                                                                                                           R, out);
    HIP_TRY(ctx, hipGetLastError());
    ctx->df_last = ImageView{out, v.w, v.h, 1.0f};
    ctx->df_rec = rec;
    return end_work(ctx, stream);
}

rsrt_status rsrt_dof_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "dof_download"); if (st0) return st0; }
    if (!ctx->df_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "no lens image (rsrt_dof first)");
    if (host_rgba || n_floats) {
        const rsrt_status st = download_floats(ctx, "dof_download", ctx->df_last.img, ctx->df_last.pixels() * 4u, host_rgba, n_floats);
        if (st) return st;
    }
    if (width) *width = ctx->df_last.w;
    if (height) *height = ctx->df_last.h;
    return RSRT_OK;
}

rsrt_status rsrt_dof_coc_download(rsrt_context *ctx, float *host_r, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "dof_coc_download"); if (st0) return st0; }
    if (!ctx->df_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "no lens image (rsrt_dof first)");
    const size_t n = ctx->df_last.pixels();
    if (!host_r || n_floats != n) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof_coc_download: expected %zu floats", n);
    std::vector<float> texels(n * 4u);
    const rsrt_status st = download_floats(ctx, "dof_coc_download", ctx->df_buf.p, n * 4u, texels.data(), texels.size());
    if (st) return st;
    for (size_t i = 0; i < n; i++) host_r[i] = texels[4u * i + 3u];
    return RSRT_OK;
}

rsrt_status rsrt_dof_depth_at(rsrt_context *ctx, uint32_t source, const rsrt_camera *camera, uint32_t x, uint32_t y, float *z_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "dof_depth_at");
    if (st) return st;
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof_depth_at: camera is NULL");
    if (!z_out) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof_depth_at: z_out is NULL");
    const PixelBuffer *rec = nullptr;
    if ((st = dof_records(ctx, "dof_depth_at", source, &rec))) return st;
    if (x >= rec->w || y >= rec->h) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "dof_depth_at: pixel (%u, %u) outside %ux%u", x, y, rec->w, rec->h);
    if ((st = sync_all(ctx))) return st;
    float a[8];
    HIP_TRY(ctx, hipMemcpy(a, rec->p + 2u * ((size_t)y * rec->w + x), sizeof a, hipMemcpyDeviceToHost));
    float cam[13];
    dof_camera(camera, cam);
    const rsrt_dof_params p = {RSRT_DOF_FOCUS_DISTANCE, RSRT_DOF_APERTURE, RSRT_DOF_RADIUS, RSRT_DOF_FLAGS}; // (the depth depends on none of them)
    rsrt_dof_frame fr;
    memset(&fr, 0, sizeof fr);
    rsrt_dof_frame_init(&fr, cam, cam + 3, cam[12], rec->w, rec->h, 1.0f, &p);
    *z_out = rsrt_dof_depth(&fr, (int)x, (int)y, a);
    return RSRT_OK;
}

rsrt_status rsrt_dof_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "dof_reset"); if (st0) return st0; }
    ctx->df_last = ImageView{};
    return RSRT_OK;
}

} // extern "C"
