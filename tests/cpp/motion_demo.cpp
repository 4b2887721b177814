// Camera motion blur through the C++ State (include/rsrt_state.hpp): render with the AOV pass, motion_blur with no previous camera (the
// source itself), turn the camera and render again, motion_blur after the remembered camera, the motion image, its velocities and
// tile maxima, then the meter, bloom and the bloomed display of the motion image; their checksums (FNV-1a) and the exposure's bits to
// stdout.
//   motion_demo scene.toml w h bounces env_w env_h samples max_radius yaw_step
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
    if (argc != 10) { std::fprintf(stderr, "usage: motion_demo scene.toml w h bounces env_w env_h samples max_radius yaw_step\n"); return 2; }
    try {
        rsrt::Scene scene(argv[1]);
        rsrt::Environment env = rsrt::Environment::synthetic((uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]), samples = (uint32_t)std::atoi(argv[7]);
        rsrt::State state(scene, {&env}, w, h);
        state.max_bounces = (uint32_t)std::atoi(argv[4]);
        rsrt_motion_params p = rsrt::State::motion_defaults();
        p.max_radius = (uint32_t)std::atoi(argv[8]);
        state.render_samples(samples, true);
        state.motion_blur(RSRT_EXPOSURE_MEAN, nullptr, p); // no camera remembered yet: the source itself
        const std::vector<float> still = state.motion_download();
        std::printf("still %016llx\n", fnv1a(still.data(), still.size() * sizeof(float)));
        rsrt_camera_desc cam = state.camera();
        cam.yaw += (float)std::atof(argv[9]);
        state.update(cam); // (the next render starts clean: the camera is part of the scene hash)
        state.render_samples(samples, true);
        state.motion_blur(RSRT_EXPOSURE_MEAN, nullptr, p); // after the camera of the call before
        uint32_t mw = 0, mh = 0, tx = 0, ty = 0;
        const std::vector<float> img = state.motion_download(&mw, &mh);
        std::printf("motion %u %u %016llx\n", mw, mh, fnv1a(img.data(), img.size() * sizeof(float)));
        const std::vector<float> vel = state.motion_velocity();
        std::printf("velocity %zu %016llx\n", vel.size(), fnv1a(vel.data(), vel.size() * sizeof(float)));
        const std::vector<float> tiles = state.motion_tiles(&tx, &ty);
        std::printf("tiles %u %u %016llx\n", tx, ty, fnv1a(tiles.data(), tiles.size() * sizeof(float)));
        const rsrt_exposure_result r = state.auto_exposure(RSRT_EXPOSURE_MOTION);
        std::printf("exposure %08x\n", bits(r.exposure));
        state.bloom(RSRT_EXPOSURE_MOTION);
        const std::vector<uint8_t> shown = state.display_bloomed(RSRT_EXPOSURE_MOTION);
        std::printf("display %zu %016llx\n", shown.size(), fnv1a(shown.data(), shown.size()));
        state.motion_reset();
        try {
            state.display_exposed(RSRT_EXPOSURE_MOTION);
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
