// Local exposure through the C++ State (include/rsrt_state.hpp): render, auto_exposure, local_exposure, the blurred grid, the gains and
// the graded display; their checksums (FNV-1a) and the exposure's bits to stdout.
//   local_demo scene.toml w h bounces env_w env_h samples cell
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
    if (argc != 9) { std::fprintf(stderr, "usage: local_demo scene.toml w h bounces env_w env_h samples cell\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        const rsrt_exposure_result r = state.auto_exposure();
        std::printf("exposure %08x\n", bits(r.exposure));
        state.local_exposure(RSRT_EXPOSURE_MEAN, (uint32_t)std::atoi(argv[8]));
        uint32_t dims[4] = {0, 0, 0, 0};
        const std::vector<uint32_t> grid = state.local_exposure_download(dims);
        std::printf("grid %u %u %u %u %016llx\n", dims[0], dims[1], dims[2], dims[3], fnv1a(grid.data(), grid.size() * sizeof(uint32_t)));
        const std::vector<float> gain = state.local_gain();
        std::printf("gain %zu %016llx\n", gain.size(), fnv1a(gain.data(), gain.size() * sizeof(float)));
        const std::vector<uint8_t> shown = state.display_local();
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        rsrt_local_params flat = rsrt::State::local_defaults();
        flat.shadows = flat.highlights = 0.0f;
        std::printf("strength0 %s\n", state.display_local(RSRT_EXPOSURE_MEAN, 0.0f, flat) == state.display_exposed() ? "yes" : "no");
        state.local_exposure_reset();
        try {
            state.display_local();
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
