// Rendering to a noise level through the C++ State (include/rsrt_state.hpp): render_to_noise, its rounds to stdout (floats as hex, so
// that a reader gets their bits), the last round's tile map to a file.
//   noise_demo scene.toml w h bounces env_w env_h threshold min_samples max_samples out.f32
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

int main(int argc, char **argv)
{
    if (argc != 11) { std::fprintf(stderr, "usage: noise_demo scene.toml w h bounces env_w env_h threshold min_samples max_samples out.f32\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        const std::vector<rsrt::State::NoiseRound> rounds =
            state.render_to_noise(std::strtof(argv[7], nullptr), (uint32_t)std::atoi(argv[8]), (uint32_t)std::atoi(argv[9]));
        for (const rsrt::State::NoiseRound &r : rounds) std::printf("round %u %u %a %a %u\n", r.n1, r.n2, (double)r.max_error, (double)r.mean_error, r.tiles_above);
        rsrt_noise_summary s;
        const std::vector<float> tiles = state.noise_download(&s);
        FILE *f = std::fopen(argv[10], "wb");
        if (!f || std::fwrite(tiles.data(), sizeof(float), tiles.size(), f) != tiles.size()) { std::fprintf(stderr, "cannot write %s\n", argv[10]); return 1; }
        std::fclose(f);
        std::printf("total %u tiles %u %u\n", state.sample_count(), s.tiles_x, s.tiles_y);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
