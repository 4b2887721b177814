// The auto-exposure meter and the exposed display (csrc/hip/rt_exposure.h) run on the CPU over include/rsrt_exposure.h, the header
// the kernels use — built by tests/test_exposure.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement
// (tests/exposure_ref.py).
#include <cstddef>
#include <cstdint>

#include "rsrt_exposure.h"

// hist: 257 words, zeroed here
extern "C" void exposure_histogram(const float *sums /* n*4 */, size_t n, float total, uint32_t *hist)
{
    for (uint32_t i = 0; i < RSRT_EXPOSURE_WORDS; i++) hist[i] = 0;
    for (size_t p = 0; p < n; p++) hist[rsrt_exposure_word(rsrt_exposure_luminance(sums + 4 * p, total))]++;
}

extern "C" int exposure_params_ok(const rsrt_exposure_params *p) { return rsrt_exposure_params_ok(p); }

extern "C" void exposure_result(const uint32_t *hist, const rsrt_exposure_params *p, rsrt_exposure_result *out) { rsrt_exposure_from_histogram(hist, p, out); }

extern "C" void exposure_defaults(rsrt_exposure_params *p)
{
    *p = rsrt_exposure_params{RSRT_EXPOSURE_LOW_PERMILLE, RSRT_EXPOSURE_HIGH_PERMILLE, RSRT_EXPOSURE_KEY, RSRT_EXPOSURE_MIN, RSRT_EXPOSURE_MAX,
                              RSRT_EXPOSURE_BLEND, RSRT_EXPOSURE_PREVIOUS, 0u};
}

// out: n RGBA8 pixels; exposed = 0: rsrt_display_pixel (the exposure is not looked at)
extern "C" void exposure_display(const float *sums, size_t n, float total, float exposure, int exposed, unsigned char *out)
{
    for (size_t p = 0; p < n; p++) {
        if (exposed) rsrt_display_pixel_exposed(sums + 4 * p, total, exposure, out + 4 * p);
        else rsrt_display_pixel(sums + 4 * p, total, out + 4 * p);
        out[4 * p + 3] = 255;
    }
}

// sizes, then offsets of the fields ctypes lays out: params (size, high_permille, key, blend, previous_exposure, flags), result (size,
// target, average_luminance, metered, skipped)
extern "C" void exposure_layout(uint32_t *out /* 11 */)
{
    const size_t v[11] = {sizeof(rsrt_exposure_params), offsetof(rsrt_exposure_params, high_permille), offsetof(rsrt_exposure_params, key),
                          offsetof(rsrt_exposure_params, blend), offsetof(rsrt_exposure_params, previous_exposure), offsetof(rsrt_exposure_params, flags),
                          sizeof(rsrt_exposure_result), offsetof(rsrt_exposure_result, target), offsetof(rsrt_exposure_result, average_luminance),
                          offsetof(rsrt_exposure_result, metered), offsetof(rsrt_exposure_result, skipped)};
    for (int i = 0; i < 11; i++) out[i] = (uint32_t)v[i];
}
