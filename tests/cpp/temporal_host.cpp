// The temporal pass (csrc/hip/rt_temporal.h) runs on the CPU over include/rsrt_temporal.h, the header the kernel uses — built by
// tests/test_temporal.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/temporal_ref.py).
#include <cstdint>

#include "rsrt_temporal.h"

namespace {
struct HostPrev {
    const float *col_, *feat_;
    void col(unsigned q, float o[4]) const { for (int i = 0; i < 4; i++) o[i] = col_[4 * (size_t)q + i]; }
    void feat(unsigned q, float o[4]) const { for (int i = 0; i < 4; i++) o[i] = feat_[4 * (size_t)q + i]; }
};

void frame_of(rsrt_tp_frame &fr, const float *cam, const float *prev_cam, uint32_t w, uint32_t h, uint32_t S, uint32_t T, uint32_t max_history,
              float tau_z, float tau_n)
{
    // cam: pos xyz, rot (9, column-major), fov_y
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
}
} // namespace

// one frame: prev_cam NULL = the first one since a reset
extern "C" void tp_frame(const float *sums, const float *aov, uint32_t w, uint32_t h, uint32_t S, uint32_t T, const float *cam, const float *prev_cam,
                         const float *prev_col, const float *prev_feat, uint32_t max_history, float tau_z, float tau_n, float *out_col,
                         float *out_feat, int32_t *codes)
{
    rsrt_tp_frame fr;
    frame_of(fr, cam, prev_cam, w, h, S, T, max_history, tau_z, tau_n);
    const HostPrev prev{prev_col, prev_feat};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            codes[p] = rsrt_tp_pixel(&fr, prev, (int)x, (int)y, sums + 4 * p, aov + 8 * p, out_col + 4 * p, out_feat + 4 * p);
        }
}

// every pixel's centre ray at distance z from the camera, projected back into the same camera: fx, fy (w*h each; NaN when behind)
extern "C" void tp_roundtrip(const float *cam, uint32_t w, uint32_t h, float z, float *fx, float *fy)
{
    rsrt_tp_frame fr;
    frame_of(fr, cam, nullptr, w, h, 1, 1, 1, 0.05f, 0.9f);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            float d[3], e[3];
            rsrt_tp_center_ray(&fr.cur, w, h, fr.aspect, (int)x, (int)y, d);
            for (int i = 0; i < 3; i++) e[i] = z * d[i];
            if (!rsrt_tp_project(&fr.cur, w, h, fr.aspect, e, &fx[p], &fy[p])) fx[p] = fy[p] = __builtin_nanf("");
        }
}

// the header's defaults, for the State's
extern "C" void tp_defaults(uint32_t *max_history, float *tau_z, float *tau_n, float *min_weight)
{
    *max_history = RSRT_TP_MAX_HISTORY;
    *tau_z = RSRT_TP_DEPTH_TOLERANCE;
    *tau_n = RSRT_TP_NORMAL_TOLERANCE;
    *min_weight = RSRT_TP_MIN_WEIGHT;
}
