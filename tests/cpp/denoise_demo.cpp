// The denoiser through the C++ State (include/rsrt_state.hpp): n spp with the AOV pass, the default filter, the result to a file.
//   denoise_demo scene.toml w h spp bounces env_w env_h out.f32
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: denoise_demo scene.toml w h spp bounces env_w env_h out.f32\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[6]), (uint32_t)std::atoi(argv[7]));
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[5]);
        state.render_samples((uint32_t)std::atoi(argv[4]), true);
        const std::vector<float> out = state.denoise();
        const std::vector<uint8_t> disp = state.denoised_display();
        FILE *f = std::fopen(argv[8], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[8]); return 1; }
        std::fclose(f);
        std::printf("denoised %ux%u from %u spp (%u AOV samples), %zu display bytes\n", w, h, state.sample_count(), state.aov_sample_count(), disp.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
