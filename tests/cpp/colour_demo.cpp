// White balance and colour grading through the C++ State (include/rsrt_state.hpp): render, auto_exposure, auto_white_balance (twice:
// the second call blends), a baked LUT, and the colour display with and without it; their checksums (FNV-1a) and the white point's
// bits to stdout.
//   colour_demo scene.toml w h bounces env_w env_h samples lut_size
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
    if (argc != 9) { std::fprintf(stderr, "usage: colour_demo scene.toml w h bounces env_w env_h samples lut_size\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        rsrt::State state(scene, {&env}, (uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]));
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        const rsrt_exposure_result e = state.auto_exposure();
        std::printf("exposure %08x\n", bits(e.exposure));
        rsrt_white_result r = state.auto_white_balance();
        std::printf("white %08x %08x %08x %u\n", bits(r.white[0]), bits(r.white[1]), bits(r.white[2]), r.gated);
        const std::vector<uint32_t> hist = state.white_download();
        std::printf("hist %zu %016llx\n", hist.size(), fnv1a(hist.data(), hist.size() * sizeof(uint32_t)));
        std::vector<uint8_t> shown = state.display_colour();
        std::printf("balanced %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        const float one[3] = {1.0f, 1.0f, 1.0f};
        std::printf("white1 %s\n", state.display_colour(RSRT_EXPOSURE_MEAN, 0.0f, one) == state.display_exposed() ? "yes" : "no");
        rsrt_cdl_params cdl = rsrt::State::cdl_defaults();
        cdl.slope[0] = 1.1f;
        cdl.offset[2] = -0.03f;
        cdl.power[1] = 1.2f;
        cdl.saturation = 1.25f;
        state.colour_lut(cdl, (uint32_t)std::atoi(argv[8]));
        uint32_t n = 0;
        const std::vector<float> lut = state.colour_lut_download(&n);
        std::printf("lut %u %016llx\n", n, fnv1a(lut.data(), lut.size() * sizeof(float)));
        shown = state.display_colour();
        std::printf("graded %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        r = state.auto_white_balance(RSRT_EXPOSURE_MEAN, 0.25f);
        std::printf("blended %08x %08x %08x\n", bits(r.white[0]), bits(r.white[1]), bits(r.white[2]));
        state.white_reset();
        state.colour_lut_reset();
        std::printf("reset %s\n", state.white()[0] == 0.0f && state.display_colour() == state.display_exposed() ? "yes" : "no");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
