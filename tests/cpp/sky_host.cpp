// The procedural sky (csrc/hip/rt_sky.h, librsrt_host.so's rsrt_sky_fill) on the CPU over include/rsrt_sky.h, the header both use —
// built by tests/test_sky.py with g++ -ffp-contract=off and compared bit for bit with the numpy restatement (tests/sky_ref.py).  The
// fill here forms every share per texel (rsrt_sky_at), where the library and the kernel form a row's and a column's once.
#include <cstddef>
#include <cstdint>

#include "rsrt_sky.h"

// out: h*w RGBA texels, alpha 0; returns 1 (and writes nothing) for refused parameters
extern "C" int sky_fill(int h, int w, const rsrt_sky_params *p, float *out)
{
    if (!rsrt_sky_params_ok(p)) return 1;
    rsrt_sky_constants k;
    rsrt_sky_prepare(p, (uint32_t)h, &k);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float *o = out + 4 * ((size_t)y * w + x);
            rsrt_sky_at(&k, (uint32_t)x, (uint32_t)y, (uint32_t)w, (uint32_t)h, o);
            o[3] = 0.0f;
        }
    return 0;
}

// the constants as 33 floats in the struct's order
extern "C" void sky_prepare(const rsrt_sky_params *p, int h, float *out /* 33 */)
{
    static_assert(sizeof(rsrt_sky_constants) == 33 * sizeof(float), "rsrt_sky_constants is 33 floats");
    rsrt_sky_constants k;
    rsrt_sky_prepare(p, (uint32_t)h, &k);
    const float *f = reinterpret_cast<const float *>(&k);
    for (int i = 0; i < 33; i++) out[i] = f[i];
}

extern "C" void sky_exp2(const float *t, int n, float *out)
{
    for (int i = 0; i < n; i++) out[i] = rsrt_sky_exp2(t[i]);
}

extern "C" int sky_params_ok(const rsrt_sky_params *p) { return rsrt_sky_params_ok(p); }

extern "C" void sky_defaults(rsrt_sky_params *p)
{
    *p = rsrt_sky_params{RSRT_SKY_SUN_AZIMUTH, RSRT_SKY_SUN_ELEVATION, RSRT_SKY_TURBIDITY, {RSRT_SKY_GROUND_ALBEDO, RSRT_SKY_GROUND_ALBEDO, RSRT_SKY_GROUND_ALBEDO},
                         RSRT_SKY_SCALE, RSRT_SKY_SUN_ILLUMINANCE, RSRT_SKY_SUN_RADIUS, RSRT_SKY_FLAGS};
}

// size of rsrt_sky_params, then the offsets of its fields from sun_elevation on; the size of rsrt_sky_constants
extern "C" void sky_layout(uint32_t *out /* 9 */)
{
    const size_t v[9] = {sizeof(rsrt_sky_params), offsetof(rsrt_sky_params, sun_elevation), offsetof(rsrt_sky_params, turbidity),
                         offsetof(rsrt_sky_params, ground_albedo), offsetof(rsrt_sky_params, scale), offsetof(rsrt_sky_params, sun_illuminance),
                         offsetof(rsrt_sky_params, sun_radius), offsetof(rsrt_sky_params, flags), sizeof(rsrt_sky_constants)};
    for (int i = 0; i < 9; i++) out[i] = (uint32_t)v[i];
}

// the limits and guards the header publishes: min / max elevation, min / max turbidity, max radius
extern "C" void sky_limits(float *out /* 5 */)
{
    const float v[5] = {RSRT_SKY_MIN_ELEVATION, RSRT_SKY_MAX_ELEVATION, RSRT_SKY_MIN_TURBIDITY, RSRT_SKY_MAX_TURBIDITY, RSRT_SKY_MAX_SUN_RADIUS};
    for (int i = 0; i < 5; i++) out[i] = v[i];
}
