// The variance guidance on the CPU over include/rsrt_variance.h and include/rsrt_temporal.h, the headers the kernels use
// (csrc/hip/rt_variance.h, rt_temporal_moments_kernel) — built by tests/test_variance.py with g++ -ffp-contract=off and compared bit
// for bit with the numpy restatement (tests/variance_ref.py).
#include <cstdint>
#include <vector>

#include "rsrt_temporal.h"
#include "rsrt_tonemap.h" // rsrt_round_to_f16: the binary16 packing of the features
#include "rsrt_variance.h"

namespace {
struct HostPrev {
    const float *col_, *feat_, *mom_;
    void col(unsigned q, float o[4]) const { for (int i = 0; i < 4; i++) o[i] = col_[4 * (size_t)q + i]; }
    void feat(unsigned q, float o[4]) const { for (int i = 0; i < 4; i++) o[i] = feat_[4 * (size_t)q + i]; }
    void mom(unsigned q, float o[4]) const { for (int i = 0; i < 4; i++) o[i] = mom_[4 * (size_t)q + i]; }
};
} // namespace

// one MOMENTS frame: prev_cam NULL = the first one since a reset (or a MOMENTS toggle); cameras as in temporal_host.cpp
extern "C" void sv_moments_frame(const float *sums, const float *aov, uint32_t w, uint32_t h, uint32_t S, uint32_t T, const float *cam,
                                 const float *prev_cam, const float *prev_col, const float *prev_feat, const float *prev_mom, uint32_t max_history,
                                 float tau_z, float tau_n, float *out_col, float *out_feat, float *out_mom, int32_t *codes)
{
    rsrt_tp_frame fr = {};
    rsrt_tp_camera_init(&fr.cur, cam, cam + 3, cam[12]);
    fr.has_prev = prev_cam != nullptr;
    if (prev_cam) rsrt_tp_camera_init(&fr.prev, prev_cam, prev_cam + 3, prev_cam[12]);
    else fr.prev = fr.cur;
    fr.width = w;
    fr.height = h;
    fr.sample_total = (float)S;
    fr.aov_sample_total = (float)T;
    fr.max_history = (float)max_history;
    fr.depth_tolerance = tau_z;
    fr.normal_tolerance = tau_n;
    fr.aspect = (float)w / (float)h;
    fr.identity = fr.has_prev && rsrt_tp_same_camera(&fr.cur, &fr.prev);
    const HostPrev prev{prev_col, prev_feat, prev_mom};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            codes[p] = rsrt_tp_pixel_moments(&fr, prev, (int)x, (int)y, sums + 4 * p, aov + 8 * p, out_col + 4 * p, out_feat + 4 * p, out_mom + 4 * p);
        }
}

// rsrt_denoise with RSRT_DENOISE_VARIANCE (variance) and / or RSRT_DENOISE_CLAMP (clamp), as rt_dn_prepare_kernel, rt_sv_variance_kernel
// and the levels run it; mom: the temporal moment records, or NULL (from the input).  out: w*h*3; v_out (w*h, or NULL): the variance
// before the first level
extern "C" void sv_filter(const float *sums, const float *aov, uint32_t w, uint32_t h, uint32_t sample_total, uint32_t aov_total, uint32_t iterations,
                          float sigma_c, float sigma_n, float sigma_z, int demodulate, int variance, int clamp, const float *mom, float *out,
                          float *v_out)
{
    const size_t n = (size_t)w * h;
    const float S = (float)sample_total, T = (float)aov_total;
    if (iterations == 0) {
        for (size_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) out[3 * i + k] = sums[4 * i + k] / S;
        return;
    }
    std::vector<float> r0(3 * n), f(4 * n), r(4 * n), r2(4 * n);
    for (size_t i = 0; i < n; i++) {
        const float sum[3] = {sums[4 * i], sums[4 * i + 1], sums[4 * i + 2]};
        float fi[4];
        rsrt_dn_prepare(sum, S, aov + 8 * i, T, demodulate, &r0[3 * i]);
        rsrt_dn_features(aov + 8 * i, T, fi);
        for (int k = 0; k < 4; k++) f[4 * i + k] = rsrt_round_to_f16(fi[k]);
    }
    const float kn = rsrt_dn_kn(sigma_n);
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            const size_t p = (size_t)y * w + x;
            float rp[3] = {r0[3 * p], r0[3 * p + 1], r0[3 * p + 2]};
            const float l = rsrt_sv_lum(rp);
            if (clamp) {
                float lmax = 0.0f;
                int have = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int qx = x + dx, qy = y + dy;
                        if ((dx == 0 && dy == 0) || qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                        const float lq = rsrt_sv_lum(&r0[3 * ((size_t)qy * w + qx)]);
                        lmax = lq > lmax ? lq : lmax;
                        have = 1;
                    }
                rsrt_sv_clamp(rp, lmax, have);
            }
            float v = 0.0f;
            if (variance) {
                float m[4] = {l, l * l, 1.0f, 1.0f};
                if (mom)
                    for (int k = 0; k < 4; k++) m[k] = mom[4 * p + k];
                float sp[3] = {0.0f, 0.0f, 0.0f};
                if (!rsrt_sv_temporal_enough(m)) {
                    const float *fp = &f[4 * p];
                    const float kz = rsrt_dn_kz(sigma_z, fp[3]);
                    for (int dy = -RSRT_SV_RADIUS; dy <= RSRT_SV_RADIUS; dy++)
                        for (int dx = -RSRT_SV_RADIUS; dx <= RSRT_SV_RADIUS; dx++) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                            const size_t q = (size_t)qy * w + qx;
                            float mu1, mu2;
                            if (mom) {
                                mu1 = mom[4 * q];
                                mu2 = mom[4 * q + 1];
                            } else {
                                mu1 = rsrt_sv_lum(&r0[3 * q]);
                                mu2 = mu1 * mu1;
                            }
                            rsrt_sv_spatial_tap(fp, kn, kz, &f[4 * q], mu1, mu2, sp);
                        }
                }
                v = rsrt_sv_variance(m, sp);
            }
            for (int k = 0; k < 3; k++) r[4 * p + k] = rp[k];
            r[4 * p + 3] = v;
            if (v_out) v_out[p] = v;
        }
    for (uint32_t lvl = 0; lvl < iterations; lvl++) {
        const bool last = lvl + 1 == iterations;
        const int step = 1 << lvl;
        for (int y = 0; y < (int)h; y++)
            for (int x = 0; x < (int)w; x++) {
                const size_t p = (size_t)y * w + x;
                const float *rp = &r[4 * p], *fp = &f[4 * p];
                const float kz = rsrt_dn_kz(sigma_z, fp[3]);
                float a[3] = {1.0f, 1.0f, 1.0f}, o[4];
                if (last && demodulate) rsrt_dn_albedo(aov + 8 * p, T, a);
                if (variance) {
                    float gs = 0.0f, gk = 0.0f;
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                            const float k = rsrt_sv_binomial(dx) * rsrt_sv_binomial(dy);
                            gs = gs + k * r[4 * ((size_t)qy * w + qx) + 3];
                            gk = gk + k;
                        }
                    const float kl = rsrt_sv_kl(sigma_c, gs / gk), lp = rsrt_sv_lum(rp);
                    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    for (int dy = -2; dy <= 2; dy++)
                        for (int dx = -2; dx <= 2; dx++) {
                            const int qx = x + dx * step, qy = y + dy * step;
                            if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                            const size_t q = (size_t)qy * w + qx;
                            rsrt_sv_tap(rsrt_dn_b3(dx) * rsrt_dn_b3(dy), lp, fp, kl, kn, kz, &r[4 * q], r[4 * q + 3], &f[4 * q], acc);
                        }
                    rsrt_sv_finish(acc, a, last && demodulate, o);
                } else {
                    const float kc = rsrt_dn_kc(sigma_c, lvl);
                    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    for (int dy = -2; dy <= 2; dy++)
                        for (int dx = -2; dx <= 2; dx++) {
                            const int qx = x + dx * step, qy = y + dy * step;
                            if (qx < 0 || qx >= (int)w || qy < 0 || qy >= (int)h) continue;
                            const size_t q = (size_t)qy * w + qx;
                            rsrt_dn_tap(rsrt_dn_b3(dx) * rsrt_dn_b3(dy), rp, fp, kc, kn, kz, &r[4 * q], &f[4 * q], acc);
                        }
                    rsrt_dn_finish(acc, a, last && demodulate, o);
                    o[3] = 0.0f;
                }
                if (last)
                    for (int k = 0; k < 3; k++) out[3 * p + k] = o[k];
                else
                    for (int k = 0; k < 4; k++) r2[4 * p + k] = o[k];
            }
        r.swap(r2);
    }
}

// the header's defaults, for the State's
extern "C" void sv_defaults(float *min_frames, float *eps, float *sigma_l, int *radius)
{
    *min_frames = RSRT_SV_MIN_FRAMES;
    *eps = RSRT_SV_EPS;
    *sigma_l = RSRT_SV_SIGMA_L;
    *radius = RSRT_SV_RADIUS;
}
