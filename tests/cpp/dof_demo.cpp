// Depth of field through the C++ State (include/rsrt_state.hpp): render with the AOV pass, focus_at the centre, depth_of_field, the
// lens image and its radii, then the meter, bloom and the bloomed display of the lens image; their checksums (FNV-1a) and the focus
// distance's and the exposure's bits to stdout.
//   dof_demo scene.toml w h bounces env_w env_h samples max_radius
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
    if (argc != 9) { std::fprintf(stderr, "usage: dof_demo scene.toml w h bounces env_w env_h samples max_radius\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]), true);
        const float z = state.focus_at(w / 2, h / 2);
        std::printf("focus %08x %08x\n", bits(z), bits(state.focus_distance()));
        rsrt_dof_params p = rsrt::State::dof_defaults();
        p.focus_distance = 0.0f; // the remembered one
        p.aperture = 0.05f;
        p.max_radius = (uint32_t)std::atoi(argv[8]);
        state.depth_of_field(RSRT_EXPOSURE_MEAN, p);
        uint32_t lw = 0, lh = 0;
        const std::vector<float> lens = state.dof_download(&lw, &lh);
        std::printf("lens %u %u %016llx\n", lw, lh, fnv1a(lens.data(), lens.size() * sizeof(float)));
        const std::vector<float> coc = state.dof_coc();
        std::printf("coc %zu %016llx\n", coc.size(), fnv1a(coc.data(), coc.size() * sizeof(float)));
        const rsrt_exposure_result r = state.auto_exposure(RSRT_EXPOSURE_LENS);
        std::printf("exposure %08x\n", bits(r.exposure));
        state.bloom(RSRT_EXPOSURE_LENS);
        const std::vector<uint8_t> shown = state.display_bloomed(RSRT_EXPOSURE_LENS);
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        state.dof_reset();
        try {
            state.display_exposed(RSRT_EXPOSURE_LENS);
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
