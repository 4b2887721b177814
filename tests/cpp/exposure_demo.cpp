// Auto-exposure through the C++ State (include/rsrt_state.hpp): render, auto_exposure twice (the second adapts from the first),
// the exposed display; the histogram's and the display bytes' checksums (FNV-1a) and the results' bits to stdout.
//   exposure_demo scene.toml w h bounces env_w env_h samples blend
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
    if (argc != 9) { std::fprintf(stderr, "usage: exposure_demo scene.toml w h bounces env_w env_h samples blend\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        const uint32_t samples = (uint32_t)std::atoi(argv[7]);
        const float blend = std::strtof(argv[8], nullptr);
        state.render_samples(samples);
        for (int frame = 0; frame < 2; frame++) {
            const rsrt_exposure_result r = state.auto_exposure(RSRT_EXPOSURE_MEAN, blend);
            std::printf("result %08x %08x %08x %u %u\n", bits(r.exposure), bits(r.target), bits(r.average_luminance), r.metered, r.skipped);
            state.render_samples(samples); // (more samples: another frame to meter)
        }
        const std::vector<uint32_t> hist = state.exposure_download();
        std::printf("hist %zu %016llx\n", hist.size(), fnv1a(hist.data(), hist.size() * sizeof(uint32_t)));
        const std::vector<uint8_t> shown = state.display_exposed();
        std::printf("display %zu %016llx %08x\n", shown.size(), fnv1a(shown.data(), shown.size()), bits(state.exposure()));
        state.exposure_reset();
        try {
            state.display_exposed();
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
