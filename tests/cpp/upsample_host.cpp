// The guided upsampling's passes (csrc/hip/rt_upsample.h: the prepare pass, rt_up_kernel) run on the CPU over include/rsrt_upsample.h,
// the header the kernel uses — built by tests/test_upsample.py with g++ -ffp-contract=off and compared bit for bit with the numpy
// restatement (tests/upsample_ref.py).
#include <cstdint>
#include <vector>

#include "rsrt_tonemap.h" // rsrt_round_to_f16: the binary16 packing of the features
#include "rsrt_upsample.h"

// returns the number of output pixels that took the nearest low pixel's value
extern "C" uint32_t up_filter(const float *colour /* w*h*4 */, const float *aov /* w*h*8 */, const float *guide /* W*H*8 */, uint32_t w, uint32_t h,
                              uint32_t W, uint32_t H, uint32_t sample_total, uint32_t aov_total, uint32_t guide_total, float sigma_n, float sigma_z,
                              int demodulate, float *out /* W*H*3 */)
{
    const size_t n = (size_t)w * h;
    const float S = (float)sample_total, T = (float)aov_total, Tg = (float)guide_total;
    std::vector<float> r(3 * n), f(4 * n);
    for (size_t i = 0; i < n; i++) {
        const float sum[3] = {colour[4 * i], colour[4 * i + 1], colour[4 * i + 2]};
        float fi[4];
        rsrt_dn_prepare(sum, S, aov + 8 * i, T, demodulate, &r[3 * i]);
        rsrt_dn_features(aov + 8 * i, T, fi);
        for (int k = 0; k < 4; k++) f[4 * i + k] = rsrt_round_to_f16(fi[k]);
    }
    uint32_t fallbacks = 0;
    for (uint32_t Y = 0; Y < H; Y++)
        for (uint32_t X = 0; X < W; X++) {
            const size_t P = (size_t)Y * W + X;
            float fr[4], fp[4], a[3];
            rsrt_dn_features(guide + 8 * P, Tg, fr);
            rsrt_dn_albedo(guide + 8 * P, Tg, a);
            for (int k = 0; k < 4; k++) fp[k] = rsrt_round_to_f16(fr[k]);
            const float kn = rsrt_dn_kn(sigma_n), kz = rsrt_dn_kz(sigma_z, fp[3]);
            const float u = rsrt_up_coord(X, w, W), v = rsrt_up_coord(Y, h, H);
            const int xn = rsrt_up_nearest(u), yn = rsrt_up_nearest(v);
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int dy = -1; dy <= 1; dy++) {
                const int qy = yn + dy;
                if (qy < 0 || qy >= (int)h) continue;
                const float hy = rsrt_up_tent(qy, v);
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = xn + dx;
                    if (qx < 0 || qx >= (int)w) continue;
                    const size_t q = (size_t)qy * w + qx;
                    rsrt_up_tap(rsrt_up_tent(qx, u) * hy, fp, kn, kz, &r[3 * q], &f[4 * q], acc);
                }
            }
            const size_t nq = (size_t)(yn < (int)h - 1 ? yn : (int)h - 1) * w + (size_t)(xn < (int)w - 1 ? xn : (int)w - 1);
            if (!(acc[3] > 0.0f)) fallbacks++;
            rsrt_up_finish(acc, &r[3 * nq], a, demodulate, &out[3 * P]);
        }
    return fallbacks;
}
