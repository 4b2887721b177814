// The JPEG pass through the C++ State (include/rsrt_state.hpp): render, auto_exposure, then display_jpeg at the defaults (quality 90,
// 4:2:0), at quality 50 and 4:4:4, and at quality 100, where the State's first guess at the size is too small and it asks again; every
// file's size and checksum (FNV-1a) to stdout, and the default file to disk.
//   jpeg_demo scene.toml w h bounces env_w env_h samples out.jpg
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char *>(data)[i]) * 1099511628211ull;
    return h;
}

static void show(const char *name, const std::vector<uint8_t> &file) { std::printf("%s %zu %016llx\n", name, file.size(), fnv1a(file.data(), file.size())); }

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: jpeg_demo scene.toml w h bounces env_w env_h samples out.jpg\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        state.auto_exposure();
        rsrt_jpeg_params j = rsrt::State::jpeg_defaults();
        std::printf("defaults %u %u %u %u\n", j.quality, j.subsampling, j.flags, j.reserved);
        const std::vector<uint8_t> file = state.display_jpeg();
        show("default", file);
        FILE *f = std::fopen(argv[8], "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size() || std::fclose(f) != 0) throw rsrt::Error("cannot write the file");
        j.quality = 50u;
        j.subsampling = RSRT_JPEG_444;
        show("q50_444", state.display_jpeg(j));
        j = rsrt::State::jpeg_defaults();
        j.quality = 100u;
        show("q100", state.display_jpeg(j));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
