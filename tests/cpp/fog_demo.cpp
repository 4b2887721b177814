// Volumetric fog through the C++ State (include/rsrt_state.hpp): render with the AOV pass, the fog records of the same samples in two
// calls, the fog image of the mean, then the lens, the meter, bloom and the bloomed display of the fog image; their checksums (FNV-1a)
// and the exposure's bits to stdout.
//   fog_demo scene.toml w h bounces env_w env_h samples steps density
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rsrt_state.hpp"

static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char *>(data)[i]) * 1099511628211ull;
    return h;
}

static unsigned bits(float f)
{
    unsigned u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: fog_demo scene.toml w h bounces env_w env_h samples steps density\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), samples = (uint32_t)std::atoi(argv[7]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        rsrt_sky_params sky = rsrt::State::sky_defaults();
        sky.sun_azimuth = 2.0f;
        sky.sun_elevation = 0.9f;
        rsrt_fog_params p = rsrt::State::fog_light_from_sky(rsrt::State::fog_defaults(), sky, 512);
        p.steps = (uint32_t)std::atoi(argv[8]);
        p.density = (float)std::atof(argv[9]);
        p.ambient[0] = p.ambient[1] = p.ambient[2] = 0.05f;
        std::printf("light %08x %08x %08x %08x %08x %08x\n", bits(p.light_dir[0]), bits(p.light_dir[1]), bits(p.light_dir[2]), bits(p.light_irradiance[0]),
                    bits(p.light_irradiance[1]), bits(p.light_irradiance[2]));
        state.render_samples(samples, true);
        state.render_fog(1, p);
        if (samples > 1) state.render_fog(samples - 1); // progressive, with the remembered parameters
        const std::vector<float> rec = state.download_fog();
        std::printf("records %u %016llx\n", state.fog_sample_count(), fnv1a(rec.data(), rec.size() * sizeof(float)));
        state.fog();
        const std::vector<float> img = state.fog_download();
        std::printf("fog %zu %016llx\n", img.size(), fnv1a(img.data(), img.size() * sizeof(float)));
        state.depth_of_field(RSRT_EXPOSURE_FOG);
        const std::vector<float> lens = state.dof_download();
        std::printf("lens %016llx\n", fnv1a(lens.data(), lens.size() * sizeof(float)));
        const rsrt_exposure_result r = state.auto_exposure(RSRT_EXPOSURE_FOG);
        std::printf("exposure %08x\n", bits(r.exposure));
        state.bloom(RSRT_EXPOSURE_FOG);
        const std::vector<uint8_t> shown = state.display_bloomed(RSRT_EXPOSURE_FOG);
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        state.fog_reset();
        try {
            state.display_exposed(RSRT_EXPOSURE_FOG);
            std::printf("reset no\n");
        } catch (const rsrt::Error &) {
            std::printf("reset yes\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
