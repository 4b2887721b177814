// rt_motion.h — the camera motion blur pass's kernels and their C-ABI (include/rsrt.h "camera motion blur").  Included
// at the end of rsrt_api.hip.  All arithmetic is include/rsrt_motion.h's.
//
//  rt_motion_prepare_kernel  one 16 x 16 workgroup a tile, one thread a pixel: the source's sum, the first-hit record and the two cameras
//                            -> the prepared texel (colour and l as one float4, z, u), and the tile's maximum: a max over the total
//                            order (l's bit pattern — monotone, l >= 0 — then the lower row-major index), across the wave by shuffles,
//                            across the four waves through LDS; whatever the reduction's shape, the same texel wins.  48 B read, 28 B
//                            written a pixel, 12 B a tile.
//  rt_motion_gather_kernel   one 16 x 16 workgroup a tile.  It forms the neighbour maximum from the (at most) nine tile records itself:
//                            uniform loads.  Under half a pixel it copies the tile and ends.  Otherwise it stages the tile and a halo
//                            of B = ceil(nl) prepared texels in LDS (colour and l: 16 B, z: 4 B a texel; all of a lane's loads issued
//                            before the first is used; a texel outside the frame is staged with l = -1, which no texel inside has, and
//                            its tap is skipped) and runs the taps from LDS at the tile's offsets.  (16 + 2 B)^2 x 20 B of dynamic LDS:
//                            45 KB at B = 16, 11.25 KB at B = 4.  No static LDS in front of it, no scratch memory.
#include "../../../include/rsrt_motion.h"

#define RT_MOTION_TILE 16
#define RT_MOTION_BLOCK (RT_MOTION_TILE * RT_MOTION_TILE)
#define RT_MOTION_MAX_HALO 16
#define RT_MOTION_MAX_STAGED ((RT_MOTION_TILE + 2 * RT_MOTION_MAX_HALO) * (RT_MOTION_TILE + 2 * RT_MOTION_MAX_HALO))
#define RT_MOTION_LOADS ((RT_MOTION_MAX_STAGED + RT_MOTION_BLOCK - 1) / RT_MOTION_BLOCK) // loads in flight a lane, at most
static_assert(RT_MOTION_TILE == RSRT_MOTION_TILE && RT_MOTION_MAX_HALO == RSRT_MOTION_MAX_RADIUS && RSRT_MOTION_MAX_RADIUS <= RSRT_MOTION_TILE,
              "the neighbour maximum covers one tile around");

// img: sums of fr.total samples; rec: the first-hit records of the same size (2 float4 a pixel).  cl: (colour, l), z, uv: the prepared
// texels; tiles: one record a tile
__global__ __launch_bounds__(RT_MOTION_BLOCK) void rt_motion_prepare_kernel(rsrt_motion_frame fr, const float4 *img, const float4 *rec, float4 *cl, float *z,
                                                                            float2 *uv, rsrt_motion_vel *tiles)
{
    __shared__ unsigned long long wave_max[RT_MOTION_BLOCK / 64];
    const int tid = (int)threadIdx.x, x = (int)blockIdx.x * RT_MOTION_TILE + tid % RT_MOTION_TILE, y = (int)blockIdx.y * RT_MOTION_TILE + tid / RT_MOTION_TILE;
    const bool inside = x < (int)fr.width && y < (int)fr.height;
    rsrt_motion_texel t = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    unsigned long long key = 0ull; // (a texel outside the frame: below every texel inside)
    if (inside) {
        const size_t i = (size_t)y * (size_t)fr.width + (size_t)x;
        const float4 s = img[i];
        const float sum[3] = {s.x, s.y, s.z};
        float a[8];
        dn_aov(rec, i, a);
        t = rsrt_motion_prepare(&fr, x, y, sum, a);
        cl[i] = make_float4(t.r, t.g, t.b, t.l);
        z[i] = t.z;
        uv[i] = make_float2(t.ux, t.uy);
        key = ((unsigned long long)rsrt_tp_bits(t.l) << 32) | (unsigned long long)(RT_MOTION_BLOCK - 1 - tid);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(key >> 32), m, 64), lo = (unsigned)__shfl_xor((int)(key & 0xffffffffull), m, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other > key ? other : key;
    }
    if ((tid & 63) == 0) wave_max[tid >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RT_MOTION_BLOCK / 64; k++) key = wave_max[k] > key ? wave_max[k] : key;
    if (tid == RT_MOTION_BLOCK - 1 - (int)(key & 0xffffffffull)) { // the winner (inside the frame: the tile's first texel always is)
        rsrt_motion_vel m = {0.0f, 0.0f, 0.0f};
        if (t.l > 0.0f) { m.ux = t.ux; m.uy = t.uy; m.l = t.l; }
        tiles[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

// cl, z, out: w x h; tiles: gridDim.x x gridDim.y records; taps in 2 .. 32; dynamic LDS: (16 + 2 R)^2 (sizeof(float4) + sizeof(float)) for
// the call's max_radius R, which bounds every record's l
__global__ __launch_bounds__(RT_MOTION_BLOCK) void rt_motion_gather_kernel(const float4 *cl, const float *z, const rsrt_motion_vel *tiles, int w, int h, int taps,
                                                                           int R, float4 *out)
{
    extern __shared__ __attribute__((aligned(16))) float4 rt_motion_lds[];
    const int tid = (int)threadIdx.x, bx = (int)blockIdx.x * RT_MOTION_TILE, by = (int)blockIdx.y * RT_MOTION_TILE;
    const int lx = tid % RT_MOTION_TILE, ly = tid / RT_MOTION_TILE, x = bx + lx, y = by + ly;
    const bool inside = x < w && y < h;
    const rsrt_motion_vel n = rsrt_motion_neighbour_max(tiles, (int)gridDim.x, (int)gridDim.y, (int)blockIdx.x, (int)blockIdx.y);
    if (n.l < 0.5f) { // the whole workgroup: a copy
        if (inside) {
            const float4 c = cl[(size_t)y * (size_t)w + (size_t)x];
            out[(size_t)y * (size_t)w + (size_t)x] = make_float4(c.x, c.y, c.z, 1.0f);
        }
        return;
    }
    int B = rsrt_motion_ceil(n.l);
    B = B < R ? B : R; // (l <= R already: the prepare step clamps)
    const int sw = RT_MOTION_TILE + 2 * B, nst = sw * sw, gx0 = bx - B, gy0 = by - B;
    float4 *const s = rt_motion_lds;                       // the staged texels: s[ty * sw + tx] is the texel (gx0 + tx, gy0 + ty)
    float *const sz = reinterpret_cast<float *>(s + nst);  // ... and their depths
    float4 c[RT_MOTION_LOADS];
    float d[RT_MOTION_LOADS];
#pragma unroll
    for (int k = 0; k < RT_MOTION_LOADS; k++) {
        const int i = k * RT_MOTION_BLOCK + tid;
        if (i < nst) {
            const int gx = gx0 + i % sw, gy = gy0 + i / sw;
            const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
            const size_t g = in ? (size_t)gy * (size_t)w + (size_t)gx : 0;
            c[k] = in ? cl[g] : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
            d[k] = in ? z[g] : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < RT_MOTION_LOADS; k++) {
        const int i = k * RT_MOTION_BLOCK + tid;
        if (i < nst) {
            s[i] = c[k];
            sz[i] = d[k];
        }
    }
    __syncthreads();
    if (!inside) return;
    const int at = (ly + B) * sw + lx + B;
    const float4 p = s[at];
    const float z_p = sz[at], s_p = rsrt_motion_spread(p.w);
    rsrt_motion_acc acc = RSRT_MOTION_ACC_INIT;
    for (int i = 0; i < taps; i++) {
        int ox, oy;
        float dist;
        rsrt_motion_tap_at(&n, i, taps, &ox, &oy, &dist);
        ox = ox < -B ? -B : (ox > B ? B : ox); // (never taken: |o_i| <= ceil(nl), rsrt_motion.h; keeps a read inside the staged window whatever the record holds)
        oy = oy < -B ? -B : (oy > B ? B : oy);
        const int j = at + oy * sw + ox;
        const float4 q = s[j];
        if (q.w < 0.0f) continue; // outside the frame
        rsrt_motion_tap(&acc, s_p, z_p, dist, q.x, q.y, q.z, q.w, sz[j]);
    }
    float o[4];
    rsrt_motion_resolve(&acc, taps, p.x, p.y, p.z, o);
    out[(size_t)y * (size_t)w + (size_t)x] = make_float4(o[0], o[1], o[2], o[3]);
}

namespace {

// the first-hit records `source` is blurred by: dof_records' for the four images, and for the lens image the ones it was built from
rsrt_status motion_records(rsrt_context *ctx, const char *what, uint32_t source, const PixelBuffer **rec)
{
    if (source == IMAGE_MOTION) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the motion image is not a source of its own pass", what);
    if (source > IMAGE_FOG) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: unknown source %u", what, source);
    if (source != IMAGE_LENS) return dof_records(ctx, what, source, rec);
    if (!ctx->df_last.img || !ctx->df_rec) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no lens image (rsrt_dof first)", what);
    if (!ctx->df_rec->p) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no %s any more (the lens image was built from it)", what, ctx->df_rec->name);
    *rec = ctx->df_rec;
    return RSRT_OK;
}

// cl (float4), the library's output (float4), uv (float2), z (float) of n pixels, in one allocation
constexpr size_t kMotionBytesPerPixel = 2u * sizeof(float4) + sizeof(float2) + sizeof(float);
float4 *motion_cl(rsrt_context *ctx) { return static_cast<float4 *>(ctx->mt_buf.p); }
float4 *motion_own_out(rsrt_context *ctx) { return motion_cl(ctx) + ctx->mt_buf.pixels(); }
float2 *motion_uv(rsrt_context *ctx) { return reinterpret_cast<float2 *>(motion_cl(ctx) + 2u * ctx->mt_buf.pixels()); }
float *motion_z(rsrt_context *ctx) { return reinterpret_cast<float *>(motion_uv(ctx) + ctx->mt_buf.pixels()); }

rsrt_status motion_image(rsrt_context *ctx, const char *what)
{
    rsrt_status st = whole_frame(ctx, what);
    if (st) return st;
    if (!ctx->mt_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "no motion image (rsrt_motion_blur first)");
    return RSRT_OK;
}

} // namespace

extern "C" {

rsrt_status rsrt_motion_blur(rsrt_context *ctx, uint32_t source, uint32_t sample_total, const rsrt_camera *camera, const rsrt_camera *previous,
                             const rsrt_motion_params *params, void *device_out_rgba32f, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = whole_frame(ctx, "motion_blur");
    if (st) return st;
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: camera is NULL");
    if (!previous) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: previous is NULL");
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: params is NULL");
    if (!rsrt_motion_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: want shutter finite and in [0, 1], max_radius in 1..%d, taps even and in 2..%u, flags 0",
                    RSRT_MOTION_MAX_RADIUS, RSRT_MOTION_MAX_TAPS);
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: sample_total must be > 0");
    if ((uintptr_t)device_out_rgba32f % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: output pointer must be 16-byte aligned");
    const PixelBuffer *rec = nullptr;
    if ((st = motion_records(ctx, "motion_blur", source, &rec))) return st;
    ImageView v;
    if ((st = resolve_image(ctx, "motion_blur", "motion_blur: ", source, sample_total, false, &v))) return st;
    if (rec->w != v.w || rec->h != v.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: %s is %ux%u, the source %ux%u", rec->name, rec->w, rec->h, v.w, v.h);
    if (v.w > 0x3fffffffu || v.h > 0x3fffffffu) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_blur: source too large");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const uint32_t tx = (v.w + RT_MOTION_TILE - 1u) / RT_MOTION_TILE, ty = (v.h + RT_MOTION_TILE - 1u) / RT_MOTION_TILE;
    if (!ctx->mt_buf.is(v.w, v.h)) ctx->mt_last = ImageView{}; // (the allocation that held the motion image, or its velocities, goes)
    if ((st = ensure_sized(ctx, ctx->mt_buf, v.w, v.h, kMotionBytesPerPixel))) return st;
    if ((st = ensure_sized(ctx, ctx->mt_tiles, tx, ty, sizeof(rsrt_motion_vel)))) return st;
    if ((st = begin_work(ctx, stream))) return st;
    ctx->mt_last = ImageView{}; // (a failed launch leaves no motion image)
    float cur[13], prev[13];
    dof_camera(camera, cur);
    dof_camera(previous, prev);
    rsrt_motion_frame fr;
    memset(&fr, 0, sizeof fr);
    rsrt_motion_frame_init(&fr, cur, prev, v.w, v.h, v.total, params);
    float4 *const out = device_out_rgba32f ? static_cast<float4 *>(device_out_rgba32f) : motion_own_out(ctx);
    rsrt_motion_vel *const tiles = static_cast<rsrt_motion_vel *>(ctx->mt_tiles.p);
    rt_motion_prepare_kernel<<<dim3(tx, ty), dim3(RT_MOTION_BLOCK), 0, stream>>>(fr, v.img, rec->p, motion_cl(ctx), motion_z(ctx), motion_uv(ctx), tiles);
    const int R = (int)params->max_radius;
    const size_t lds = (size_t)(RT_MOTION_TILE + 2 * R) * (size_t)(RT_MOTION_TILE + 2 * R) * (sizeof(float4) + sizeof(float));
    rt_motion_gather_kernel<<<dim3(tx, ty), dim3(RT_MOTION_BLOCK), lds, stream>>>(motion_cl(ctx), motion_z(ctx), tiles, (int)v.w, (int)v.h, (int)params->taps, R, out);
    HIP_TRY(ctx, hipGetLastError());
    ctx->mt_last = ImageView{out, v.w, v.h, 1.0f};
    return end_work(ctx, stream);
}

rsrt_status rsrt_motion_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = motion_image(ctx, "motion_download");
    if (st) return st;
    if (host_rgba || n_floats) {
        if ((st = download_floats(ctx, "motion_download", ctx->mt_last.img, ctx->mt_last.pixels() * 4u, host_rgba, n_floats))) return st;
    }
    if (width) *width = ctx->mt_last.w;
    if (height) *height = ctx->mt_last.h;
    return RSRT_OK;
}

rsrt_status rsrt_motion_velocity_download(rsrt_context *ctx, float *host_uvl, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = motion_image(ctx, "motion_velocity_download");
    if (st) return st;
    const size_t n = ctx->mt_last.pixels();
    if (!host_uvl || n_floats != n * 3u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "motion_velocity_download: expected %zu floats", n * 3u);
    std::vector<float> cl(n * 4u), uv(n * 2u);
    if ((st = download_floats(ctx, "motion_velocity_download", motion_cl(ctx), cl.size(), cl.data(), cl.size()))) return st;
    if ((st = download_floats(ctx, "motion_velocity_download", motion_uv(ctx), uv.size(), uv.data(), uv.size()))) return st;
    for (size_t i = 0; i < n; i++) {
        host_uvl[3u * i] = uv[2u * i];
        host_uvl[3u * i + 1u] = uv[2u * i + 1u];
        host_uvl[3u * i + 2u] = cl[4u * i + 3u];
    }
    return RSRT_OK;
}

rsrt_status rsrt_motion_tiles_download(rsrt_context *ctx, float *host_uvl, size_t n_floats, uint32_t *tiles_x, uint32_t *tiles_y)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = motion_image(ctx, "motion_tiles_download");
    if (st) return st;
    if (host_uvl || n_floats) {
        if ((st = download_floats(ctx, "motion_tiles_download", ctx->mt_tiles.p, ctx->mt_tiles.pixels() * 3u, host_uvl, n_floats))) return st;
    }
    if (tiles_x) *tiles_x = ctx->mt_tiles.w;
    if (tiles_y) *tiles_y = ctx->mt_tiles.h;
    return RSRT_OK;
}

rsrt_status rsrt_motion_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "motion_reset"); if (st0) return st0; }
    ctx->mt_last = ImageView{};
    return RSRT_OK;
}

} // extern "C"
