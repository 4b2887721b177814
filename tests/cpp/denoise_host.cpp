// The denoiser's passes (csrc/hip/rt_denoise.h: prepare, levels) run on the CPU over include/rsrt_denoise.h, the header the
// kernels use — built by tests/test_denoise.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement.
#include <cstdint>
#include <vector>

#include "rsrt_denoise.h"
#include "rsrt_tonemap.h" // rsrt_round_to_f16: the binary16 packing of the features

extern "C" void dn_filter(const float *sums, const float *aov, uint32_t w, uint32_t h, uint32_t sample_total, uint32_t aov_total, uint32_t iterations,
                          float sigma_c, float sigma_n, float sigma_z, int demodulate, float *out /* w*h*3 */)
{
    const size_t n = (size_t)w * h;
    const float S = (float)sample_total, T = (float)aov_total;
    if (iterations == 0) {
        for (size_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) out[3 * i + k] = sums[4 * i + k] / S;
        return;
    }
    std::vector<float> r(3 * n), r2(3 * n), f(4 * n);
    for (size_t i = 0; i < n; i++) {
        const float sum[3] = {sums[4 * i], sums[4 * i + 1], sums[4 * i + 2]};
        float fi[4];
        rsrt_dn_prepare(sum, S, aov + 8 * i, T, demodulate, &r[3 * i]);
        rsrt_dn_features(aov + 8 * i, T, fi);
        for (int k = 0; k < 4; k++) f[4 * i + k] = rsrt_round_to_f16(fi[k]);
    }
    for (uint32_t lvl = 0; lvl < iterations; lvl++) {
        const bool last = lvl + 1 == iterations;
        const int step = 1 << lvl;
        for (int y = 0; y < (int)h; y++)
            for (int x = 0; x < (int)w; x++) {
                const size_t p = (size_t)y * w + x;
                const float *rp = &r[3 * p], *fp = &f[4 * p];
                const float kc = rsrt_dn_kc(sigma_c, lvl), kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int dy = -2; dy <= 2; dy++) {
                    const int qy = y + dy * step;
                    if (qy < 0 || qy >= (int)h) continue;
                    for (int dx = -2; dx <= 2; dx++) {
                        const int qx = x + dx * step;
                        if (qx < 0 || qx >= (int)w) continue;
                        const size_t q = (size_t)qy * w + qx;
                        rsrt_dn_tap(rsrt_dn_b3(dx) * rsrt_dn_b3(dy), rp, fp, kc, kn, kz, &r[3 * q], &f[4 * q], acc);
                    }
                }
                float a[3] = {1.0f, 1.0f, 1.0f};
                if (last && demodulate) rsrt_dn_albedo(aov + 8 * p, T, a);
                rsrt_dn_finish(acc, a, last && demodulate, last ? &out[3 * p] : &r2[3 * p]);
            }
        r.swap(r2);
    }
}
