// The finished display through the C++ State (include/rsrt_state.hpp): render, auto_exposure, a baked LUT, then display_finished with
// everything off (the colour display's bytes), with the defaults, and with sharpening, grain, dither and the noise limiter at two seeds;
// their checksums (FNV-1a) to stdout.
//   finish_demo scene.toml w h bounces env_w env_h samples lut_size
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char *>(data)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: finish_demo scene.toml w h bounces env_w env_h samples lut_size\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        state.auto_exposure();
        rsrt_cdl_params cdl = rsrt::State::cdl_defaults();
        cdl.slope[0] = 1.1f;
        cdl.saturation = 1.25f;
        state.colour_lut(cdl, (uint32_t)std::atoi(argv[8]));
        rsrt_finish_params f = rsrt::State::finish_defaults();
        std::printf("defaults %08x %u\n", (unsigned)(f.sharpness * 256.0f) << 16 | (unsigned)(f.grain * 256.0f) << 8 | (unsigned)f.dither, f.flags);
        std::vector<uint8_t> shown = state.display_finished();
        std::printf("default %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        f.sharpness = f.grain = f.dither = 0.0f;
        std::printf("off %s\n", state.display_finished(f) == state.display_colour() ? "yes" : "no");
        f = rsrt_finish_params{1.0f, 0.5f, 1.0f, 7u, RSRT_FINISH_NOISE_AWARE, {0u, 0u, 0u}};
        shown = state.display_finished(f);
        std::printf("seed7 %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        std::printf("again %s\n", state.display_finished(f) == shown ? "yes" : "no");
        f.seed = 8u;
        shown = state.display_finished(f);
        std::printf("seed8 %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
