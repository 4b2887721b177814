// Bloom through the C++ State (include/rsrt_state.hpp): render, auto_exposure, bloom, the bloom image and the bloomed display;
// their checksums (FNV-1a) and the exposure's bits to stdout.
//   bloom_demo scene.toml w h bounces env_w env_h samples levels
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
    if (argc != 9) { std::fprintf(stderr, "usage: bloom_demo scene.toml w h bounces env_w env_h samples levels\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        const rsrt_exposure_result r = state.auto_exposure();
        std::printf("exposure %08x\n", bits(r.exposure));
        rsrt_bloom_params p = rsrt::State::bloom_defaults();
        p.levels = (uint32_t)std::atoi(argv[8]);
        state.bloom(RSRT_EXPOSURE_MEAN, 0.0f, p);
        uint32_t bw = 0, bh = 0;
        const std::vector<float> b = state.bloom_download(&bw, &bh);
        std::printf("bloom %u %u %016llx\n", bw, bh, fnv1a(b.data(), b.size() * sizeof(float)));
        const std::vector<uint8_t> shown = state.display_bloomed();
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        const std::vector<uint8_t> plain = state.display_bloomed(RSRT_EXPOSURE_MEAN, 0.0f, 0.0f), exposed = state.display_exposed();
        std::printf("intensity0 %s\n", plain == exposed ? "yes" : "no");
        state.bloom_reset();
        try {
            state.display_bloomed();
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
