// The depth-of-field pass (csrc/hip/rt_dof.h) run on the CPU over include/rsrt_dof.h, the header the kernels use — built by
// tests/test_dof.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/dof_ref.py).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rsrt_dof.h"

static void frame_of(rsrt_dof_frame *fr, const float *cam /* pos 3, rot 9 (column-major), fov_y */, int h, int w, float total, const rsrt_dof_params *p)
{
    rsrt_dof_frame_init(fr, cam, cam + 3, cam[12], (unsigned)w, (unsigned)h, total, p);
}

// out: h*w prepared texels (rgb, r); sums h*w*4, rec h*w*8; neither need be aligned
extern "C" void dof_prepare(const float *sums, const float *rec, int h, int w, float total, const float *cam, const rsrt_dof_params *p, float *out)
{
    rsrt_dof_frame fr;
    frame_of(&fr, cam, h, w, total, p);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const rsrt_dof_texel t = rsrt_dof_prepare(&fr, x, y, sums + 4 * i, rec + 8 * i);
            out[4 * i] = t.r; out[4 * i + 1] = t.g; out[4 * i + 2] = t.b; out[4 * i + 3] = t.rad;
        }
}

// out: h*w RGBA texels, alpha 1, as rsrt_dof_download returns the lens image; prep: h*w prepared texels
extern "C" void dof_gather(const float *prep, int h, int w, int max_radius, float *out)
{
    std::vector<rsrt_dof_texel> img((size_t)w * h);
    for (size_t i = 0; i < img.size(); i++) img[i] = rsrt_dof_texel{prep[4 * i], prep[4 * i + 1], prep[4 * i + 2], prep[4 * i + 3]};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) rsrt_dof_pixel(img.data(), w, h, max_radius, x, y, out + 4 * ((size_t)y * w + x));
}

// out: h*w depths along the optical axis (+inf on sky), as rsrt_dof_depth_at returns one
extern "C" void dof_depth(const float *rec, int h, int w, const float *cam, float *out)
{
    const rsrt_dof_params p = {RSRT_DOF_FOCUS_DISTANCE, RSRT_DOF_APERTURE, RSRT_DOF_RADIUS, RSRT_DOF_FLAGS};
    rsrt_dof_frame fr;
    frame_of(&fr, cam, h, w, 1.0f, &p);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) out[(size_t)y * w + x] = rsrt_dof_depth(&fr, x, y, rec + 8 * ((size_t)y * w + x));
}

extern "C" void dof_table(float *out /* 33 * 33 */)
{
    for (int dy = -RSRT_DOF_MAX_RADIUS; dy <= RSRT_DOF_MAX_RADIUS; dy++)
        for (int dx = -RSRT_DOF_MAX_RADIUS; dx <= RSRT_DOF_MAX_RADIUS; dx++)
            out[(dy + RSRT_DOF_MAX_RADIUS) * RSRT_DOF_TABLE_WIDTH + dx + RSRT_DOF_MAX_RADIUS] = rsrt_dof_dist(dx, dy);
}

extern "C" int dof_params_ok(const rsrt_dof_params *p) { return rsrt_dof_params_ok(p); }

extern "C" void dof_defaults(rsrt_dof_params *p) { *p = rsrt_dof_params{RSRT_DOF_FOCUS_DISTANCE, RSRT_DOF_APERTURE, RSRT_DOF_RADIUS, RSRT_DOF_FLAGS}; }

// size of rsrt_dof_params, then the offsets of aperture, max_radius, flags; RSRT_DOF_MAX_RADIUS; RSRT_EXPOSURE_LENS; the table's width
extern "C" void dof_layout(uint32_t *out /* 7 */)
{
    const size_t v[7] = {sizeof(rsrt_dof_params), offsetof(rsrt_dof_params, aperture), offsetof(rsrt_dof_params, max_radius), offsetof(rsrt_dof_params, flags),
                         RSRT_DOF_MAX_RADIUS, RSRT_EXPOSURE_LENS, RSRT_DOF_TABLE_WIDTH};
    for (int i = 0; i < 7; i++) out[i] = (uint32_t)v[i];
}
