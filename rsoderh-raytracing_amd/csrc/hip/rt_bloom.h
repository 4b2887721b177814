// rt_bloom.h — the bloom pass's kernels, the bloomed display kernel and their C-ABI (include/rsrt.h "bloom").
// Included at the end of rsrt_api.hip.  All arithmetic is include/rsrt_bloom.h's.
//
//  rt_bloom_first_kernel     D_1 from the source image: the prefilter and the first 13-tap downsample in one pass over the source.  A
//                            256-thread workgroup makes a tile of RT_BL_TW x RT_BL_TH outputs.  It loads the (2 TW + 4) x (2 TH + 4)
//                            source texels the tile needs (16 B a lane, rows of 1088 B, all of a lane's loads issued before the first
//                            is used; coordinates clamped here, once), prefilters them into LDS, builds every 2x2 tap once
//                            ((2 TW + 3) x (2 TH + 3) of them, in LDS) and every corner group once ((TW + 1) x (TH + 1), in the LDS the
//                            source texels no longer need); an output then reads four taps for its centre group and four corner
//                            groups.  32 KB of LDS, no scratch memory.
//  rt_bloom_down_kernel      D_k from D_{k-1}, k > 1: the same tile scheme without the prefilter, plain form.
//  rt_bloom_up_kernel        U_k = D_k + up(tent(U_{k+1})), in place over D_k; the tent is not stored.
//  rt_bloom_final_kernel     B = tent(U_1) * (1 / N).
//  rt_display_bloomed_kernel rt_display_exposed_kernel plus the four taps of up(B).
#include "../../../include/rsrt_bloom.h"

#define RT_BL_TW 32
#define RT_BL_TH 8
#define RT_BL_BLOCK (RT_BL_TW * RT_BL_TH)
#define RT_BL_SW (2 * RT_BL_TW + 4)   // source texels of a tile
#define RT_BL_SH (2 * RT_BL_TH + 4)
#define RT_BL_PW (RT_BL_SW - 1)       // 2x2 taps of a tile
#define RT_BL_PH (RT_BL_SH - 1)
#define RT_BL_GW (RT_BL_TW + 1)       // corner groups of a tile
#define RT_BL_GH (RT_BL_TH + 1)
#define RT_BL_LOADS ((RT_BL_SW * RT_BL_SH + RT_BL_BLOCK - 1) / RT_BL_BLOCK) // loads in flight a lane

// src: w x h; dst: ceil(w / 2) x ceil(h / 2).  FIRST: src holds sums of `total` samples and goes through the prefilter.
template <bool FIRST>
__device__ __forceinline__ void rt_bloom_down_tile(const rsrt_bloom_texel *src, int w, int h, float total, float exposure, float threshold, int karis,
                                                   rsrt_bloom_texel *dst, int dw, int dh)
{
    __shared__ rsrt_bloom_rgb s[RT_BL_SW * RT_BL_SH]; // the source texels; later the corner groups
    __shared__ rsrt_bloom_rgb p[RT_BL_PW * RT_BL_PH]; // the taps
    const int tid = (int)threadIdx.x, bx = (int)blockIdx.x * RT_BL_TW, by = (int)blockIdx.y * RT_BL_TH;
    const int sx0 = 2 * bx - 2, sy0 = 2 * by - 2; // s[ty][tx] is the texel (cl(sx0 + tx), cl(sy0 + ty))
    rsrt_bloom_rgb c[RT_BL_LOADS];
#pragma unroll
    for (int k = 0; k < RT_BL_LOADS; k++) {
        const int i = k * RT_BL_BLOCK + tid;
        if (i < RT_BL_SW * RT_BL_SH) c[k] = rsrt_bloom_at(src, w, h, sx0 + i % RT_BL_SW, sy0 + i / RT_BL_SW);
    }
#pragma unroll
    for (int k = 0; k < RT_BL_LOADS; k++) {
        const int i = k * RT_BL_BLOCK + tid;
        if (i < RT_BL_SW * RT_BL_SH) s[i] = FIRST ? rsrt_bloom_prefilter(c[k], total, exposure, threshold) : c[k];
    }
    __syncthreads();
    for (int i = tid; i < RT_BL_PW * RT_BL_PH; i += RT_BL_BLOCK) {
        const int at = (i / RT_BL_PW) * RT_BL_SW + i % RT_BL_PW;
        p[i] = rsrt_bloom_box(s[at], s[at + 1], s[at + RT_BL_SW], s[at + RT_BL_SW + 1]);
    }
    __syncthreads(); // the taps are whole, and nobody reads the source texels any more
    rsrt_bloom_rgb *const g = s;
    for (int i = tid; i < RT_BL_GW * RT_BL_GH; i += RT_BL_BLOCK) {
        const int at = 2 * (i / RT_BL_GW) * RT_BL_PW + 2 * (i % RT_BL_GW);
        g[i] = rsrt_bloom_box(p[at], p[at + 2], p[at + 2 * RT_BL_PW], p[at + 2 * RT_BL_PW + 2]);
    }
    __syncthreads();
    const int lx = tid % RT_BL_TW, ly = tid / RT_BL_TW, x = bx + lx, y = by + ly;
    if (x >= dw || y >= dh) return;
    const int at = (2 * ly + 1) * RT_BL_PW + 2 * lx + 1, ga = ly * RT_BL_GW + lx;
    const rsrt_bloom_rgb gc = rsrt_bloom_box(p[at], p[at + 2], p[at + 2 * RT_BL_PW], p[at + 2 * RT_BL_PW + 2]);
    rsrt_bloom_store(dst, (size_t)y * (size_t)dw + (size_t)x, rsrt_bloom_down(gc, g[ga], g[ga + 1], g[ga + RT_BL_GW], g[ga + RT_BL_GW + 1], karis));
}

__global__ __launch_bounds__(RT_BL_BLOCK) void rt_bloom_first_kernel(const float4 *src, int w, int h, float total, float exposure, float threshold, int karis,
                                                                     rsrt_bloom_texel *dst, int dw, int dh)
{
    rt_bloom_down_tile<true>(reinterpret_cast<const rsrt_bloom_texel *>(src), w, h, total, exposure, threshold, karis, dst, dw, dh);
}

__global__ __launch_bounds__(RT_BL_BLOCK) void rt_bloom_down_kernel(const rsrt_bloom_texel *src, int w, int h, rsrt_bloom_texel *dst, int dw, int dh)
{
    rt_bloom_down_tile<false>(src, w, h, 1.0f, 1.0f, 0.0f, 0, dst, dw, dh);
}

// d (dw x dh, D_k on entry, U_k on return) += up(tent(u)), u = U_{k+1} (w x h)
__global__ __launch_bounds__(RT_BL_BLOCK) void rt_bloom_up_kernel(const rsrt_bloom_texel *u, int w, int h, rsrt_bloom_texel *d, int dw, int dh)
{
    const int x = (int)(blockIdx.x * RT_BL_TW + threadIdx.x % RT_BL_TW), y = (int)(blockIdx.y * RT_BL_TH + threadIdx.x / RT_BL_TW);
    if (x >= dw || y >= dh) return;
    const size_t i = (size_t)y * (size_t)dw + (size_t)x;
    rsrt_bloom_store(d, i, rsrt_bloom_add(rsrt_bloom_load(d, i), rsrt_bloom_up_tent_at(u, w, h, x, y)));
}

// b = tent(u) * scale, both w x h
__global__ __launch_bounds__(RT_BL_BLOCK) void rt_bloom_final_kernel(const rsrt_bloom_texel *u, int w, int h, float scale, rsrt_bloom_texel *b)
{
    const int x = (int)(blockIdx.x * RT_BL_TW + threadIdx.x % RT_BL_TW), y = (int)(blockIdx.y * RT_BL_TH + threadIdx.x / RT_BL_TW);
    if (x >= w || y >= h) return;
    rsrt_bloom_store(b, (size_t)y * (size_t)w + (size_t)x, rsrt_bloom_mul(rsrt_bloom_tent_at(u, w, h, x, y), scale));
}

// img: w x h sums; b: bw x bh
__global__ void rt_display_bloomed_kernel(const float4 *img, int w, int h, float total, float exposure, float intensity, const rsrt_bloom_texel *b, int bw,
                                          int bh, uchar4 *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)w * (size_t)h) return;
    const float4 a = img[i];
    const float sum[3] = {a.x, a.y, a.z};
    unsigned char rgb[3];
    rsrt_display_pixel_bloomed(sum, total, exposure, intensity, rsrt_bloom_up_at(b, bw, bh, (int)(i % (size_t)w), (int)(i / (size_t)w)), rgb);
    out[i] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

namespace {

dim3 bloom_grid(uint32_t w, uint32_t h) { return dim3((w + RT_BL_TW - 1u) / RT_BL_TW, (h + RT_BL_TH - 1u) / RT_BL_TH); }

// texels of the pyramid of a w x h source: B, then D_1 .. D_RSRT_BLOOM_MAX_LEVELS
size_t bloom_texels(uint32_t w, uint32_t h)
{
    size_t n = (size_t)rsrt_bloom_level_size(w, 1) * rsrt_bloom_level_size(h, 1);
    for (uint32_t k = 1; k <= RSRT_BLOOM_MAX_LEVELS; k++) n += (size_t)rsrt_bloom_level_size(w, k) * rsrt_bloom_level_size(h, k);
    return n;
}

rsrt_status bloom_source(rsrt_context *ctx, const char *what, uint32_t source, uint32_t sample_total, float exposure, ImageView *v)
{
    const rsrt_status st = whole_frame(ctx, what);
    if (st) return st;
    if (!rsrt_exposure_finite_positive(exposure)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: exposure must be finite and > 0", what);
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: sample_total must be > 0", what);
    return resolve_image(ctx, what, "", source, sample_total, false, v);
}

// what a pass built for one source is v's too, or "<what>: the bloom image was built for WxH, the source is WxH" (and the grid likewise)
rsrt_status built_for(rsrt_context *ctx, const char *what, const char *piece, const SizedAlloc &a, const ImageView &v)
{
    if (a.is(v.w, v.h)) return RSRT_OK;
    return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the %s was built for %ux%u, the source is %ux%u", what, piece, a.w, a.h, v.w, v.h);
}

// there is a bloom image, and it is v's
rsrt_status bloom_ready(rsrt_context *ctx, const char *what, const ImageView &v)
{
    if (!ctx->bl_have) return fail(ctx, RSRT_ERR_NOT_READY, "no bloom image (rsrt_bloom first)");
    return built_for(ctx, what, "bloom image", ctx->bl_pyr, v);
}

} // namespace

extern "C" {

rsrt_status rsrt_bloom(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_bloom_params *params, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "bloom"); if (st0) return st0; }
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bloom: params is NULL");
    if (!rsrt_bloom_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bloom: want levels in 1..%u, flags RSRT_BLOOM_KARIS or 0, threshold finite and >= 0", RSRT_BLOOM_MAX_LEVELS);
    ImageView v;
    rsrt_status st = bloom_source(ctx, "bloom", source, sample_total, exposure, &v);
    if (st) return st;
    if (v.w > 0x3fffffffu || v.h > 0x3fffffffu) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bloom: source too large");
    const hipStream_t stream = stream_of(ctx, hip_stream);
    const size_t texels = bloom_texels(v.w, v.h), px = v.pixels();
    if (!ctx->bl_pyr.is(v.w, v.h)) ctx->bl_have = false; // (the allocation that held B goes)
    if ((st = ensure_sized(ctx, ctx->bl_pyr, v.w, v.h, (texels * sizeof(rsrt_bloom_texel) + px - 1u) / px))) return st;
    if ((st = begin_work(ctx, stream))) return st;
    ctx->bl_have = false; // (a failed launch leaves no bloom image)
    const uint32_t N = params->levels;
    rsrt_bloom_texel *const B = static_cast<rsrt_bloom_texel *>(ctx->bl_pyr.p);
    rsrt_bloom_texel *D[RSRT_BLOOM_MAX_LEVELS + 1];
    uint32_t lw[RSRT_BLOOM_MAX_LEVELS + 1], lh[RSRT_BLOOM_MAX_LEVELS + 1];
    lw[0] = v.w;
    lh[0] = v.h;
    D[0] = nullptr;
    rsrt_bloom_texel *next = B + (size_t)rsrt_bloom_level_size(v.w, 1) * rsrt_bloom_level_size(v.h, 1);
    for (uint32_t k = 1; k <= N; k++) {
        lw[k] = rsrt_bloom_level_size(v.w, k);
        lh[k] = rsrt_bloom_level_size(v.h, k);
        D[k] = next;
        next += (size_t)lw[k] * lh[k];
    }
    rt_bloom_first_kernel<<<bloom_grid(lw[1], lh[1]), dim3(RT_BL_BLOCK), 0, stream>>>(v.img, (int)v.w, (int)v.h, v.total, exposure, params->threshold,
                                                                                     (int)(params->flags & RSRT_BLOOM_KARIS), D[1], (int)lw[1], (int)lh[1]);
    for (uint32_t k = 2; k <= N; k++)
        rt_bloom_down_kernel<<<bloom_grid(lw[k], lh[k]), dim3(RT_BL_BLOCK), 0, stream>>>(D[k - 1], (int)lw[k - 1], (int)lh[k - 1], D[k], (int)lw[k], (int)lh[k]);
    for (uint32_t k = N - 1; k >= 1; k--)
        rt_bloom_up_kernel<<<bloom_grid(lw[k], lh[k]), dim3(RT_BL_BLOCK), 0, stream>>>(D[k + 1], (int)lw[k + 1], (int)lh[k + 1], D[k], (int)lw[k], (int)lh[k]);
    rt_bloom_final_kernel<<<bloom_grid(lw[1], lh[1]), dim3(RT_BL_BLOCK), 0, stream>>>(D[1], (int)lw[1], (int)lh[1], 1.0f / (float)N, B);
    HIP_TRY(ctx, hipGetLastError());
    ctx->bl_have = true;
    return end_work(ctx, stream);
}

rsrt_status rsrt_bloom_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "bloom_download"); if (st0) return st0; }
    if (!ctx->bl_have) return fail(ctx, RSRT_ERR_NOT_READY, "no bloom image (rsrt_bloom first)");
    const uint32_t bw = rsrt_bloom_level_size(ctx->bl_pyr.w, 1), bh = rsrt_bloom_level_size(ctx->bl_pyr.h, 1);
    const size_t n = (size_t)bw * bh;
    if (host_rgba || n_floats) {
        const rsrt_status st = download_floats(ctx, "bloom_download", ctx->bl_pyr.p, n * 4u, host_rgba, n_floats);
        if (st) return st;
        for (size_t i = 0; i < n; i++) host_rgba[4 * i + 3] = 1.0f;
    }
    if (width) *width = bw;
    if (height) *height = bh;
    return RSRT_OK;
}

rsrt_status rsrt_bloom_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    { rsrt_status st0 = whole_frame(ctx, "bloom_reset"); if (st0) return st0; }
    ctx->bl_have = false;
    return RSRT_OK;
}

rsrt_status rsrt_display_bloomed_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, float intensity, uint8_t *host_rgba8,
                                       size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ImageView v;
    rsrt_status st = bloom_source(ctx, "display_bloomed_srgb8", source, sample_total, exposure, &v);
    if (st) return st;
    const size_t n = v.pixels();
    if (!rsrt_bloom_finite_nonneg(intensity)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_bloomed_srgb8: intensity must be finite and >= 0");
    if (!host_rgba8 || n_bytes != n * 4) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_bloomed_srgb8: expected %zu bytes", n * 4);
    if ((st = bloom_ready(ctx, "display_bloomed_srgb8", v))) return st; // (at intensity 0 too)
    const uint32_t bw = rsrt_bloom_level_size(v.w, 1), bh = rsrt_bloom_level_size(v.h, 1);
    return read_back(ctx, host_rgba8, n * sizeof(uchar4), 0, [&](void *tmp) {
        rt_display_bloomed_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(v.img, (int)v.w, (int)v.h, v.total, exposure, intensity,
                                                                                                  static_cast<const rsrt_bloom_texel *>(ctx->bl_pyr.p), (int)bw, (int)bh,
                                                                                                  static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
