// The fog rebuild's arithmetic (csrc/hip/rt_fog.h, rt_fog_source_kernel and rt_fog_rebuild_kernel) run on the CPU over
// include/rsrt_fog_upsample.h, the header the kernels use — built by tests/test_fog_upsample.py with g++ -ffp-contract=off and compared
// bit for bit with the numpy restatement (tests/fog_upsample_ref.py).  With -DFOGUP_HOST_MAIN it is a stand-alone program (for a
// sanitizer build) that runs every function over a few inputs.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rsrt.h"
#include "rsrt_fog_upsample.h"

static rsrt_fog_constants constants(const rsrt_fog_params *p)
{
    rsrt_fog_constants k;
    rsrt_fog_prepare(p, &k);
    return k;
}

// rec: n_pixels * 4 of fog_total samples; out: n_pixels * 3
extern "C" void fogup_source(const float *rec, float fog_total, size_t n_pixels, float *out)
{
    for (size_t i = 0; i < n_pixels; i++) rsrt_fogup_source(rec + 4 * i, fog_total, out + 3 * i);
}

// g: n_pixels * 8 of record_total samples; out: n_pixels
extern "C" void fogup_tau(const rsrt_fog_params *p, const float *g, float record_total, size_t n_pixels, float *out)
{
    const rsrt_fog_constants k = constants(p);
    for (size_t i = 0; i < n_pixels; i++) out[i] = rsrt_fogup_tau(&k, g + 8 * i, record_total);
}

// one axis: the low coordinate, its nearest low pixel and the three tents of every output pixel; u, xn: out_size; tent: out_size * 3
extern "C" void fogup_axis(uint32_t low_size, uint32_t out_size, float *u, int *xn, float *tent)
{
    for (uint32_t X = 0; X < out_size; X++) {
        u[X] = rsrt_up_coord(X, low_size, out_size);
        xn[X] = rsrt_up_nearest(u[X]);
        for (int d = -1; d <= 1; d++) tent[3 * X + (d + 1)] = rsrt_up_tent(xn[X] + d, u[X]);
    }
}

// taps: n * 3 source terms with weights hs[n], in order, into acc (4, in and out)
extern "C" void fogup_taps(const float *hs, const float *sq, size_t n, float *acc)
{
    for (size_t i = 0; i < n; i++) rsrt_fogup_tap(hs[i], sq + 3 * i, acc);
}

// colour: n * 3; acc: n * 4; tau: n; out: n * 3
extern "C" void fogup_finish(const float *colour, const float *acc, const float *tau, size_t n, float *out)
{
    for (size_t i = 0; i < n; i++) rsrt_fogup_finish(colour + 3 * i, acc + 4 * i, tau[i], out + 3 * i);
}

// The whole call: rec w * h * 4 of fog_total samples, g W * H * 8 of record_total samples, colour W * H * 3 -> out W * H * 4, alpha 1
extern "C" void fogup_rebuild(const rsrt_fog_params *p, const float *rec, float fog_total, uint32_t w, uint32_t h, const float *g, float record_total,
                              const float *colour, uint32_t W, uint32_t H, float *out)
{
    const rsrt_fog_constants k = constants(p);
    std::vector<float> src((size_t)w * h * 4, 0.0f);
    for (size_t i = 0; i < (size_t)w * h; i++) rsrt_fogup_source(rec + 4 * i, fog_total, src.data() + 4 * i);
    for (uint32_t Y = 0; Y < H; Y++)
        for (uint32_t X = 0; X < W; X++) {
            const size_t P = (size_t)Y * W + X;
            rsrt_fogup_pixel(&k, src.data(), w, h, X, Y, W, H, g + 8 * P, record_total, colour + 3 * P, out + 4 * P);
            out[4 * P + 3] = 1.0f;
        }
}

// RSRT_FOGUP_SOURCE_MAX's bits
extern "C" uint32_t fogup_source_max_bits()
{
    const float f = RSRT_FOGUP_SOURCE_MAX;
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return u;
}

#ifdef FOGUP_HOST_MAIN
int main()
{
    rsrt_fog_params p = {RSRT_FOG_DENSITY, {RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO}, RSRT_FOG_ANISOTROPY, {0.0f, 1.0f, 0.0f}, {1.0f, 1.0f, 1.0f},
                         {RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT}, RSRT_FOG_MAX_DISTANCE, RSRT_FOG_STEPS, RSRT_FOG_FLAGS};
    double sum = 0.0;
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {2, 2, 7, 7}, {34, 3, 67, 5}, {5, 4, 5, 4}, {3, 2, 6, 4}};
    for (const auto &s : sizes) {
        const uint32_t w = s[0], h = s[1], W = s[2], H = s[3];
        std::vector<float> rec((size_t)w * h * 4), g((size_t)W * H * 8, 0.0f), colour((size_t)W * H * 3, 0.75f), out((size_t)W * H * 4, 0.0f);
        for (size_t i = 0; i < (size_t)w * h; i++) {
            const float T = (i % 5 == 0) ? 1.0f : 0.25f + 0.5f * (float)(i % 3) / 3.0f; // (some pixels see a clear medium)
            rec[4 * i] = 2.0f * (1.0f - T); rec[4 * i + 1] = 1.0f - T; rec[4 * i + 2] = (i % 7 == 0) ? 3.0e38f : 0.0f; rec[4 * i + 3] = 2.0f * T;
        }
        for (size_t i = 0; i < (size_t)W * H; i++) {
            g[8 * i + 3] = (float)(i % 4); // 0 .. 3 hits of 3 samples
            g[8 * i + 7] = 20.0f * (float)(i % 4) * (float)(i % 5);
        }
        fogup_rebuild(&p, rec.data(), 2.0f, w, h, g.data(), 3.0f, colour.data(), W, H, out.data());
        for (float v : out) sum += v;
        std::vector<float> u(W), tent(3 * (size_t)W), tau((size_t)W * H), src((size_t)w * h * 3);
        std::vector<int> xn(W);
        fogup_axis(w, W, u.data(), xn.data(), tent.data());
        fogup_tau(&p, g.data(), 3.0f, (size_t)W * H, tau.data());
        fogup_source(rec.data(), 2.0f, (size_t)w * h, src.data());
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[3];
        fogup_taps(tent.data(), src.data(), 1, acc);
        fogup_finish(colour.data(), acc, tau.data(), 1, o);
        sum += tent[1] + tau[0] + o[0];
    }
    std::printf("%.9g %08x\n", sum, fogup_source_max_bits());
    return 0;
}
#endif
