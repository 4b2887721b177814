// The fog rebuild through the C++ State (include/rsrt_state.hpp): render with the AOV pass, fog records of half the size in two calls,
// the fog image of the mean rebuilt from them (fog(source, true)), then the lens and the exposed display of the fog image; their
// checksums (FNV-1a) to stdout.
//   fog_upsample_demo scene.toml w h bounces env_w env_h samples steps density
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

int main(int argc, char **argv)
{
    if (argc != 10) { std::fprintf(stderr, "usage: fog_upsample_demo scene.toml w h bounces env_w env_h samples steps density\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), samples = (uint32_t)std::atoi(argv[7]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        rsrt_fog_params p = rsrt::State::fog_defaults();
        p.light_dir[0] = 0.0f; p.light_dir[1] = 0.6f; p.light_dir[2] = -0.8f;
        p.light_irradiance[0] = 4.0f; p.light_irradiance[1] = 3.0f; p.light_irradiance[2] = 2.0f;
        p.steps = (uint32_t)std::atoi(argv[8]);
        p.density = (float)std::atof(argv[9]);
        p.ambient[0] = p.ambient[1] = p.ambient[2] = 0.05f;
        state.render_samples(samples, true);
        const uint32_t lw = (w + 1u) / 2u, lh = (h + 1u) / 2u;
        state.render_fog(0, 1, p, lw, lh);
        if (samples > 1) state.render_fog(1, samples - 1, state.fog_params(), lw, lh);
        const std::vector<float> rec = state.download_fog();
        std::printf("records %u %zu %016llx\n", state.fog_sample_count(), rec.size(), fnv1a(rec.data(), rec.size() * sizeof(float)));
        try {
            state.fog(); // rsrt_fog_apply goes on refusing records of another size
            std::printf("plain accepted\n");
        } catch (const rsrt::Error &) {
            std::printf("plain refused\n");
        }
        state.fog(RSRT_EXPOSURE_MEAN, true);
        const std::vector<float> img = state.fog_download();
        std::printf("fog %zu %016llx\n", img.size(), fnv1a(img.data(), img.size() * sizeof(float)));
        state.depth_of_field(RSRT_EXPOSURE_FOG);
        const std::vector<float> lens = state.dof_download();
        std::printf("lens %016llx\n", fnv1a(lens.data(), lens.size() * sizeof(float)));
        const std::vector<uint8_t> shown = state.display_exposed(RSRT_EXPOSURE_FOG, 1.5f);
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
