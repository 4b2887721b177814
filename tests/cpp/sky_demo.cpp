// The procedural sky through the C++ State (include/rsrt_state.hpp): a synthetic map in slot 0, the device sky in slot 1, its texels
// back from the device and the same sky from the CPU (Environment::sky), a render lit by slot 1, then the sun moved and the texels
// again; their checksums (FNV-1a) to stdout.
//   sky_demo scene.toml w h bounces env_w env_h samples elevation_deg azimuth_deg
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
    if (argc != 10) { std::fprintf(stderr, "usage: sky_demo scene.toml w h bounces env_w env_h samples elevation_deg azimuth_deg\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        const uint32_t ew = (uint32_t)std::atoi(argv[5]), eh = (uint32_t)std::atoi(argv[6]);
        rsrt::Environment synth = rsrt::Environment::synthetic(ew, eh);
        rsrt::State state(scene, {&synth}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        const float rad = RSRT_PIF / 180.0f;
        rsrt_sky_params p = rsrt::State::sky_defaults();
        p.sun_elevation = (float)std::atof(argv[8]) * rad;
        p.sun_azimuth = (float)std::atof(argv[9]) * rad;
        state.environment_sky(1, ew, eh, p);
        uint32_t w = 0, h = 0;
        const std::vector<float> sky = state.environment_download(1, &w, &h);
        std::printf("sky %u %u %016llx\n", w, h, fnv1a(sky.data(), sky.size() * sizeof(float)));
        const rsrt::Environment host = rsrt::Environment::sky(ew, eh, p);
        std::printf("host %016llx\n", fnv1a(host.rgba.data(), host.rgba.size() * sizeof(float)));
        const std::vector<float> kept = state.environment_download(0);
        std::printf("slot0 %s\n", kept.size() == synth.rgba.size() && fnv1a(kept.data(), kept.size() * 4) == fnv1a(synth.rgba.data(), kept.size() * 4) ? "kept" : "changed");
        state.environment_index = 1;
        state.render_samples((uint32_t)std::atoi(argv[7]));
        const std::vector<float> sums = state.download();
        std::printf("render %016llx\n", fnv1a(sums.data(), sums.size() * sizeof(float)));
        p.sun_azimuth += 1.0f; // the sun moves: one more call on the same slot
        state.environment_sky(1, ew, eh, p);
        const std::vector<float> moved = state.environment_download(1);
        std::printf("moved %016llx\n", fnv1a(moved.data(), moved.size() * sizeof(float)));
        p.turbidity = 11.0f;
        try {
            state.environment_sky(1, ew, eh, p);
            std::printf("refused no\n");
        } catch (const rsrt::Error &) {
            std::printf("refused yes\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
