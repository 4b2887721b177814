// Guided upsampling through the C++ State (include/rsrt_state.hpp): n spp traced at the low size, the guide at the output size, the
// default filter and upsample, the result to a file.
//   upsample_demo scene.toml low_w low_h out_w out_h spp bounces env_w env_h out.f32
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) { std::fprintf(stderr, "usage: upsample_demo scene.toml low_w low_h out_w out_h spp bounces env_w env_h out.f32\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        const uint32_t W = (uint32_t)std::atoi(argv[4]), H = (uint32_t)std::atoi(argv[5]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[8]), (uint32_t)std::atoi(argv[9]));
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[7]);
        const std::vector<float> out = state.render_upsampled(W, H, (uint32_t)std::atoi(argv[6]));
        const std::vector<uint8_t> disp = state.upsampled_display();
        FILE *f = std::fopen(argv[10], "wb");
        if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[10]); return 1; }
        std::fclose(f);
        std::printf("upsampled %ux%u -> %ux%u from %u spp (%u AOV, %u guide samples), %zu display bytes\n", w, h, state.guide_width(), state.guide_height(),
                    state.sample_count(), state.aov_sample_count(), state.guide_sample_count(), disp.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
