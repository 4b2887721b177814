// The video pass through the C++ State (include/rsrt_state.hpp): render, auto_exposure, then display_video as NV12 at the defaults, as
// a dithered full-range I420 at the centre siting, as 10-bit yuv420p10le and as HDR10 P010 at the top-left siting with the content light
// levels; every frame's size and checksum (FNV-1a) to stdout, and the planar 8-bit frame twice into a YUV4MPEG2 file.
//   video_demo scene.toml w h bounces env_w env_h samples out.y4m
#include <cstdio>
#include <cstdlib>

#include "rsrt_state.hpp"

static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const unsigned char *>(data)[i]) * 1099511628211ull;
    return h;
}

static void show(const char *name, const std::vector<uint8_t> &frame) { std::printf("%s %zu %016llx\n", name, frame.size(), fnv1a(frame.data(), frame.size())); }

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: video_demo scene.toml w h bounces env_w env_h samples out.y4m\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        state.render_samples((uint32_t)std::atoi(argv[7]));
        state.auto_exposure();
        rsrt_video_params v = rsrt::State::video_defaults();
        std::printf("defaults %u %u %u %u %u %g %u %u\n", v.standard, v.depth, v.layout, v.range, v.siting, (double)v.dither, v.seed, v.flags);
        show("nv12", state.display_video());
        v.layout = RSRT_VIDEO_PLANAR;
        v.range = RSRT_VIDEO_FULL;
        v.siting = RSRT_VIDEO_SITING_CENTRE;
        v.dither = 1.0f;
        v.seed = 7u;
        const std::vector<uint8_t> planar = state.display_video(v);
        show("i420", planar);
        for (int append = 0; append < 2; append++)
            if (rsrt_y4m_write(argv[8], append, w, h, 25, 1, &v, planar.data(), planar.size()) != 0) throw rsrt::Error("rsrt_y4m_write failed");
        v = rsrt::State::video_defaults();
        v.depth = 10u;
        v.layout = RSRT_VIDEO_PLANAR;
        show("i420p10", state.display_video(v));
        v.standard = RSRT_VIDEO_HDR10;
        v.layout = RSRT_VIDEO_SEMIPLANAR;
        v.siting = RSRT_VIDEO_SITING_TOPLEFT;
        const rsrt_hdr_params hdr = rsrt::State::hdr_defaults();
        rsrt_hdr_levels lv{};
        show("hdr10", state.display_video(v, &hdr, &lv));
        std::printf("levels %u %llu %.9g %.9g\n", lv.max_q, (unsigned long long)lv.sum_q, (double)lv.max_cll, (double)lv.max_fall);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
