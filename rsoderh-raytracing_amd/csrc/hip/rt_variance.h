// rt_variance.h — the variance-guided filter and the firefly clamp (rsrt_denoise with RSRT_DENOISE_VARIANCE / RSRT_DENOISE_CLAMP;
// include/rsrt.h "denoiser").  Included at the end of rsrt_api.hip, after rt_temporal.h.  rsrt_denoise runs
// rt_dn_prepare_kernel as for the fixed filter, then:
//
//  rt_sv_variance_kernel  the clamp (3 x 3 luminance of the prepared input) and the variance (the pixel's moment record, or the 7 x 7
//                         spatial estimate from the packed features and the moments: the temporal pass's records, or the input's own
//                         luminance).  Writes (r, v) into the float4 ping-pong buffer.  64 x 4 workgroups like rt_dn_level_kernel.
//  rt_sv_level_kernel     one variance-guided level: the 3 x 3 blur of v, then 25 taps of step 2^i that read the same 24 bytes a tap
//                         as rt_dn_level_kernel (v rides in the alpha the fixed filter leaves at 1), and write (r', v').
// The per-pixel arithmetic is include/rsrt_variance.h.
#include "../../../include/rsrt_variance.h"

// TEMPORAL: moment records from mom (the temporal pass's), otherwise (l, l l, 1, 1) from the input itself
template <bool TEMPORAL>
__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_sv_variance_kernel(const float4 *src, const ushort4 *feat, const float4 *mom, float4 *dst,
                                                                             uint32_t w, uint32_t h, int clamp, int variance, float sigma_n,
                                                                             float sigma_z)
{
    const int x = (int)(blockIdx.x * RT_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RT_DN_BY + threadIdx.y);
    if (x >= (int)w || y >= (int)h) return;
    const size_t p = (size_t)y * w + (size_t)x;
    const float4 c = src[p];
    float r[3] = {c.x, c.y, c.z};
    const float l = rsrt_sv_lum(r);
    if (clamp) {
        float lmax = 0.0f;
        int have = 0;
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= (int)h) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= (int)w) continue;
                const float4 cq = src[(size_t)qy * w + (size_t)qx];
                const float rq[3] = {cq.x, cq.y, cq.z};
                const float lq = rsrt_sv_lum(rq);
                lmax = lq > lmax ? lq : lmax;
                have = 1;
            }
        }
        rsrt_sv_clamp(r, lmax, have);
    }
    float v = 0.0f;
    if (variance) {
        float m[4];
        if (TEMPORAL) {
            const float4 mp = mom[p];
            m[0] = mp.x; m[1] = mp.y; m[2] = mp.z; m[3] = mp.w;
        } else {
            m[0] = l; m[1] = l * l; m[2] = 1.0f; m[3] = 1.0f;
        }
        float sp[3] = {0.0f, 0.0f, 0.0f};
        if (!rsrt_sv_temporal_enough(m)) {
            const ushort4 g = feat[p];
            const float fp[4] = {dn_f(g.x), dn_f(g.y), dn_f(g.z), dn_f(g.w)};
            const float kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
            for (int dy = -RSRT_SV_RADIUS; dy <= RSRT_SV_RADIUS; dy++) {
                const int qy = y + dy;
                if (qy < 0 || qy >= (int)h) continue;
                for (int dx = -RSRT_SV_RADIUS; dx <= RSRT_SV_RADIUS; dx++) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= (int)w) continue;
                    const size_t q = (size_t)qy * w + (size_t)qx;
                    const ushort4 gq = feat[q];
                    const float fq[4] = {dn_f(gq.x), dn_f(gq.y), dn_f(gq.z), dn_f(gq.w)};
                    float mu1, mu2;
                    if (TEMPORAL) {
                        const float4 mq = mom[q];
                        mu1 = mq.x; mu2 = mq.y;
                    } else {
                        const float4 cq = src[q];
                        const float rq[3] = {cq.x, cq.y, cq.z};
                        mu1 = rsrt_sv_lum(rq);
                        mu2 = mu1 * mu1;
                    }
                    rsrt_sv_spatial_tap(fp, kn, kz, fq, mu1, mu2, sp);
                }
            }
        }
        v = rsrt_sv_variance(m, sp);
    }
    dst[p] = make_float4(r[0], r[1], r[2], v);
}

// one variance-guided level; LAST: remodulate (VARIANCE requires demodulation) and write the output with alpha 1
template <bool LAST>
__global__ __launch_bounds__(RT_DN_BX * RT_DN_BY) void rt_sv_level_kernel(const float4 *src, const ushort4 *feat, const float4 *aov, float4 *dst,
                                                                          uint32_t w, uint32_t h, uint32_t level, float sigma_l, float sigma_n,
                                                                          float sigma_z, float aov_total)
{
    const int x = (int)(blockIdx.x * RT_DN_BX + threadIdx.x), y = (int)(blockIdx.y * RT_DN_BY + threadIdx.y);
    if (x >= (int)w || y >= (int)h) return;
    const size_t p = (size_t)y * w + (size_t)x;
    const float4 c = src[p];
    const ushort4 g = feat[p];
    const float rp[3] = {c.x, c.y, c.z}, fp[4] = {dn_f(g.x), dn_f(g.y), dn_f(g.z), dn_f(g.w)};
    float gs = 0.0f, gk = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)w) continue;
            const float k = rsrt_sv_binomial(dx) * rsrt_sv_binomial(dy);
            gs = gs + k * src[(size_t)qy * w + (size_t)qx].w;
            gk = gk + k;
        }
    }
    const float kl = rsrt_sv_kl(sigma_l, gs / gk), kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
    const float lp = rsrt_sv_lum(rp);
    const int step = 1 << level;
    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
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
            rsrt_sv_tap(rsrt_dn_b3(dx) * rsrt_dn_b3(dy), lp, fp, kl, kn, kz, rq, cq.w, fq, acc);
        }
    }
    float a[3] = {1.0f, 1.0f, 1.0f}, out[4];
    if (LAST) {
        float r[8];
        dn_aov(aov, p, r);
        rsrt_dn_albedo(r, aov_total, a);
    }
    rsrt_sv_finish(acc, a, LAST, out);
    dst[p] = make_float4(out[0], out[1], out[2], LAST ? 1.0f : out[3]);
}

namespace {

void sv_filter(rsrt_context *ctx, hipStream_t stream, const rsrt_denoise_params &p, bool temporal, float4 *ping, float4 *pong, const ushort4 *feat,
               float4 *out, uint32_t w, uint32_t h, float aov_total)
{
    const dim3 grid((w + RT_DN_BX - 1) / RT_DN_BX, (h + RT_DN_BY - 1) / RT_DN_BY), block(RT_DN_BX, RT_DN_BY);
    const int clamp = (p.flags & RSRT_DENOISE_CLAMP) ? 1 : 0, variance = (p.flags & RSRT_DENOISE_VARIANCE) ? 1 : 0;
    const int demod = (p.flags & RSRT_DENOISE_DEMODULATE) ? 1 : 0;
    if (temporal && variance)
        rt_sv_variance_kernel<true><<<grid, block, 0, stream>>>(ping, feat, temporal_moments(ctx), pong, w, h, clamp, variance, p.sigma_normal, p.sigma_depth);
    else
        rt_sv_variance_kernel<false><<<grid, block, 0, stream>>>(ping, feat, nullptr, pong, w, h, clamp, variance, p.sigma_normal, p.sigma_depth);
    float4 *a = pong, *b = ping; // level i reads a (i even) or b
    const uint32_t L = p.iterations;
    for (uint32_t i = 0; i < L; i++) {
        const float4 *src = (i % 2u == 0u) ? a : b;
        float4 *dst = (i + 1u == L) ? out : ((i % 2u == 0u) ? b : a);
        if (variance) {
            if (i + 1u == L)
                rt_sv_level_kernel<true><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, dst, w, h, i, p.sigma_color, p.sigma_normal, p.sigma_depth, aov_total);
            else
                rt_sv_level_kernel<false><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, dst, w, h, i, p.sigma_color, p.sigma_normal, p.sigma_depth, aov_total);
        } else if (i + 1u == L) {
            rt_dn_level_kernel<true><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, dst, w, h, i, p.sigma_color, p.sigma_normal, p.sigma_depth, aov_total, demod);
        } else {
            rt_dn_level_kernel<false><<<grid, block, 0, stream>>>(src, feat, ctx->aov.p, dst, w, h, i, p.sigma_color, p.sigma_normal, p.sigma_depth, aov_total, demod);
        }
    }
}

} // namespace
