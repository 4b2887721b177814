// The HDR display through the C++ State (include/rsrt_state.hpp): render, auto_exposure, then display_hdr in both encodings with the
// content light levels, the PQ words again without the levels and with dither; their checksums (FNV-1a) and the levels to stdout.
//   hdr_demo scene.toml w h bounces env_w env_h samples
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char *>(data)[i]) * 1099511628211ull;
    return h;
}

static void show(const char *name, const std::vector<uint8_t> &words, const rsrt_hdr_levels &lv)
{
    std::printf("%s %zu %016llx %u %llu %.9g %.9g\n", name, words.size(), fnv1a(words.data(), words.size()), lv.max_q, (unsigned long long)lv.sum_q, (double)lv.max_cll,
                (double)lv.max_fall);
}

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: hdr_demo scene.toml w h bounces env_w env_h samples\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        state.auto_exposure();
        rsrt_hdr_params p = rsrt::State::hdr_defaults();
        std::printf("defaults %g %g %g %g %u %u %u\n", (double)p.paper_white_nits, (double)p.peak_nits, (double)p.knee, (double)p.dither, p.seed, p.encoding, p.flags);
        rsrt_hdr_levels lv{};
        std::vector<uint8_t> pq = state.display_hdr(p, &lv);
        show("pq10", pq, lv);
        std::printf("without %s\n", state.display_hdr() == pq ? "yes" : "no");
        p.dither = 1.0f;
        p.seed = 7u;
        show("dithered", state.display_hdr(p, &lv), lv);
        p = rsrt::State::hdr_defaults();
        p.encoding = RSRT_HDR_SCRGB16F;
        show("scrgb16f", state.display_hdr(p, &lv), lv);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
