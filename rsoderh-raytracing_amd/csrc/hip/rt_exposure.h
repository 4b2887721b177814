// rt_exposure.h — the auto-exposure meter's kernel, the exposed display kernel and their C-ABI (include/rsrt.h "auto-exposure";
// DESIGN.md §15).  Included at the end of rsrt_api.hip.
//
//  rt_exposure_hist_kernel     a 256-thread workgroup walks trips of 2048 consecutive pixels of a float4 image (16 B a lane, coalesced;
//                              the eight loads of a trip are issued before the first is used).  A pixel's word — its bin, or 256 for a
//                              skipped pixel (include/rsrt_exposure.h) — is counted in the WAVE's own 257-word histogram in LDS with an
//                              integer add whose result is not used.  A wave whose 64 pixels share a word (sky, a wall: the common
//                              case, and 64 adds on one LDS address) finds that out with readfirstlane + ballot and lets lane 0 add
//                              64.  After one __syncthreads the workgroup sums its four histograms and adds every non-zero word to
//                              the histogram in global memory with one integer atomic; at most one workgroup a CU is launched,
//                              because the time of that hand-on grows with the number of workgroups.  Integers only:
//                              the result does not depend on the order of anything.  No scratch memory, 4112 B of LDS.
//                              The context holds TWO histograms, each 2 KB aligned: a call adds into the one that is zero and its
//                              workgroup 0 zeroes the other — the result of the call before, which the new call supersedes — for
//                              the call after.  So a meter call is one launch, with no memset in front of it.
//  rt_display_exposed_kernel   rt_display_kernel with rsrt_display_pixel_exposed.
// The host side of such a meter (a HistMeter in the context) is meter_launch, meter_download and meter_reset over a MeterShape; the
// white-balance meter (rt_colour.h) is the second one.
#include "../../../include/rsrt_exposure.h"

#define RT_EX_BLOCK 256u
#define RT_EX_WAVES (RT_EX_BLOCK / RT_WAVE)
#define RT_EX_AHEAD 8u              // loads in flight a lane
#define RT_EX_NONE 0xffffffffu      // a lane past the image's end
#define RT_EX_STRIDE 512u           // words from one histogram to the other: each starts a 2 KB line of its own (a histogram that
                                    // starts 4 B into a 128-byte line takes 4 us longer to add into)

// hist: zero before the launch; next: zeroed here for the call after this one
__global__ __launch_bounds__(RT_EX_BLOCK) void rt_exposure_hist_kernel(const float4 *img, size_t n, float total, uint32_t *hist, uint32_t *next)
{
    __shared__ uint32_t h[RT_EX_WAVES][RSRT_EXPOSURE_WORDS];
    if (blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < RSRT_EXPOSURE_WORDS; w += RT_EX_BLOCK) next[w] = 0u;
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1u);
    uint32_t *const mine = h[threadIdx.x / RT_WAVE];
    for (uint32_t i = threadIdx.x; i < RT_EX_WAVES * RSRT_EXPOSURE_WORDS; i += RT_EX_BLOCK) (&h[0][0])[i] = 0u;
    __syncthreads();
    const size_t trip = (size_t)RT_EX_BLOCK * RT_EX_AHEAD;
    for (size_t base = (size_t)blockIdx.x * trip; base < n; base += (size_t)gridDim.x * trip) { // (base is the workgroup's: no lane leaves early)
        float4 c[RT_EX_AHEAD];
        bool in[RT_EX_AHEAD];
#pragma unroll
        for (uint32_t k = 0; k < RT_EX_AHEAD; k++) {
            const size_t p = base + (size_t)k * RT_EX_BLOCK + threadIdx.x;
            in[k] = p < n;
            if (in[k]) c[k] = img[p];
        }
#pragma unroll
        for (uint32_t k = 0; k < RT_EX_AHEAD; k++) {
            uint32_t word = RT_EX_NONE;
            if (in[k]) {
                const float sum[3] = {c[k].x, c[k].y, c[k].z};
                word = rsrt_exposure_word(rsrt_exposure_luminance(sum, total));
            }
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
            if (__ballot(word == first) == ~0ull) { // all 64 lanes are here, and they agree
                if (first != RT_EX_NONE && lane == 0u) atomicAdd(&mine[first], (uint32_t)RT_WAVE);
            } else if (word != RT_EX_NONE) {
                atomicAdd(&mine[word], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < RSRT_EXPOSURE_WORDS; w += RT_EX_BLOCK) {
        uint32_t s = 0u;
#pragma unroll
        for (uint32_t v = 0; v < RT_EX_WAVES; v++) s += h[v][w];
        if (s) atomicAdd(&hist[w], s);
    }
}

__global__ void rt_display_exposed_kernel(const float4 *img, size_t n, float total, float exposure, uchar4 *out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = img[i];
    const float sum[3] = {a.x, a.y, a.z};
    unsigned char rgb[3];
    rsrt_display_pixel_exposed(sum, total, exposure, rgb);
    out[i] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

namespace {

// the image a metering or an exposed display means; `what` names the caller in the error texts
rsrt_status exposure_source(rsrt_context *ctx, const char *what, uint32_t source, uint32_t sample_total, ImageView *v)
{
    const rsrt_status st = whole_frame(ctx, what);
    if (st) return st;
    if (source == IMAGE_MEAN && sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: sample_total must be > 0", what);
    return resolve_image(ctx, what, "", source, sample_total, false, v);
}

// what differs between two ping-pong histogram meters: the kernel adds an image's `words` words into `hist`, which is zero, and zeroes
// `next`, workgroups of `block` threads walking trips of block * ahead pixels; the two histograms lie `stride` words apart
struct MeterShape {
    uint32_t words, stride, block, ahead;
    void (*kernel)(const float4 *img, size_t n, float total, uint32_t *hist, uint32_t *next);
};
const MeterShape kExposureMeter = {RSRT_EXPOSURE_WORDS, RT_EX_STRIDE, RT_EX_BLOCK, RT_EX_AHEAD, rt_exposure_hist_kernel};

// the histogram of v into the one of m's two that is zero: one launch, at most one workgroup a CU
rsrt_status meter_launch(rsrt_context *ctx, HistMeter &m, const MeterShape &s, const ImageView &v, hipStream_t stream)
{
    rsrt_status st;
    const size_t n = v.pixels();
    if (!m.hist || m.dirty) { // both histograms zero: once, and after a launch that failed
        { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
        if (!m.hist) HIP_TRY(ctx, hipMalloc(&m.hist, 2u * s.stride * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemset(m.hist, 0, 2u * s.stride * sizeof(uint32_t)));
        HIP_TRY(ctx, hipDeviceSynchronize()); // (the memset is enqueued on the null stream, which the kernel's stream does not wait for)
        m.cur = 0;
        m.dirty = m.have = false;
    }
    if ((st = begin_work(ctx, stream))) return st;
    const size_t trip = (size_t)s.block * s.ahead, want = (n + trip - 1u) / trip;
    uint32_t *const now = m.hist + (m.cur ^ 1u) * s.stride, *const old = m.hist + m.cur * s.stride;
    m.have = false; // (a failed launch leaves no histogram, and neither buffer known to be zero)
    m.dirty = true;
    s.kernel<<<dim3((unsigned)(want < (size_t)ctx->cus ? want : (size_t)ctx->cus)), dim3(s.block), 0, stream>>>(v.img, n, v.total, now, old);
    HIP_TRY(ctx, hipGetLastError());
    m.cur ^= 1u;
    m.dirty = false;
    m.have = true;
    return end_work(ctx, stream);
}

// m's last histogram (there is one) into host_hist, or into a buffer of its own where that is NULL; then result(the words)
template <class Result>
rsrt_status meter_download(rsrt_context *ctx, const HistMeter &m, const MeterShape &s, uint32_t *host_hist, Result result)
{
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    std::vector<uint32_t> own;
    if (!host_hist) {
        own.resize(s.words);
        host_hist = own.data();
    }
    HIP_TRY(ctx, hipMemcpy(host_hist, m.hist + m.cur * s.stride, s.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    result(host_hist);
    return RSRT_OK;
}

rsrt_status meter_reset(rsrt_context *ctx, HistMeter &m, const char *what)
{
    { rsrt_status st0 = whole_frame(ctx, what); if (st0) return st0; }
    m.have = false;
    return RSRT_OK;
}

} // namespace

extern "C" {

rsrt_status rsrt_exposure_meter(rsrt_context *ctx, uint32_t source, uint32_t sample_total, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ImageView v;
    const rsrt_status st = exposure_source(ctx, "exposure_meter", source, sample_total, &v);
    return st ? st : meter_launch(ctx, ctx->ex, kExposureMeter, v, stream_of(ctx, hip_stream));
}

rsrt_status rsrt_exposure_download(rsrt_context *ctx, const rsrt_exposure_params *params, uint32_t *host_hist, size_t n_words, rsrt_exposure_result *out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "exposure_download"); if (st0) return st0; }
    if (!params) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "exposure_download: params is NULL");
    if (params->flags != 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "exposure_download: flags must be 0");
    if (!rsrt_exposure_params_ok(params))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "exposure_download: want low_permille < high_permille <= 1000, key and 0 < min_exposure <= max_exposure finite and > 0, "
                                                     "blend in [0, 1], previous_exposure 0 or finite and > 0");
    if (host_hist && n_words != RSRT_EXPOSURE_WORDS) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "exposure_download: expected %u words", RSRT_EXPOSURE_WORDS);
    if (!ctx->ex.have) return fail(ctx, RSRT_ERR_NOT_READY, "no exposure histogram (rsrt_exposure_meter first)");
    return meter_download(ctx, ctx->ex, kExposureMeter, host_hist, [&](const uint32_t *hist) {
        if (out) rsrt_exposure_from_histogram(hist, params, out);
    });
}

rsrt_status rsrt_exposure_reset(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    return meter_reset(ctx, ctx->ex, "exposure_reset");
}

rsrt_status rsrt_display_exposed_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ImageView v;
    rsrt_status st = exposure_source(ctx, "display_exposed_srgb8", source, sample_total, &v);
    if (st) return st;
    const size_t n = v.pixels();
    if (!rsrt_exposure_finite_positive(exposure)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_exposed_srgb8: exposure must be finite and > 0");
    if (!host_rgba8 || n_bytes != n * 4) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_exposed_srgb8: expected %zu bytes", n * 4);
    return read_back(ctx, host_rgba8, n * sizeof(uchar4), 0, [&](void *tmp) {
        rt_display_exposed_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(v.img, n, v.total, exposure, static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}

} // extern "C"
