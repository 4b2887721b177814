// The variance guidance through the C++ State (include/rsrt_state.hpp): four MOMENTS frames along a camera path (a turn, a held frame
// of 2 spp, a step and tilt), each frame's moment records, then the variance-guided, clamped filter of the last one, to a file.
//   variance_demo scene.toml w h bounces env_w env_h out.f32
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: variance_demo scene.toml w h bounces env_w env_h out.f32\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        std::vector<float> out;
        const uint32_t spp[4] = {1, 1, 2, 1};
        for (int f = 0; f < 4; f++) {
            rsrt_camera_desc cam = state.camera();
            if (f == 1) cam.yaw += 0.03f;
            if (f == 3) { cam.pos[0] += 0.1f; cam.pitch += 0.02f; }
            state.update(cam);
            state.render_temporal(spp[f], rsrt::State::temporal_defaults(), true);
            const std::vector<float> m = state.download_temporal_moments();
            out.insert(out.end(), m.begin(), m.end());
        }
        rsrt_denoise_params p = rsrt::State::variance_defaults();
        p.flags |= RSRT_DENOISE_TEMPORAL | RSRT_DENOISE_CLAMP;
        const std::vector<float> den = state.denoise(p);
        out.insert(out.end(), den.begin(), den.end());
        FILE *fo = std::fopen(argv[7], "wb");
        if (!fo || std::fwrite(out.data(), sizeof(float), out.size(), fo) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
        std::fclose(fo);
        std::printf("4 MOMENTS frames of %ux%u, %u samples in the last\n", w, h, state.sample_count());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
