// rsrt_state.hpp — header-only C++17 mirror of the reference's `State` (src/state.rs:29-834) over the
// C-ABI of rsrt.h / rsrt_host.h.  What `State::new / resize / update / render` do with wgpu, this does
// with librsrt: same progressive semantics (scene-hash reset, sample_count += 1 per frame,
// src/state.rs:775-794), plus the batched render the C-ABI adds.  Errors become rsrt::Error (the
// reference's anyhow::Error / unwrap at init).
#pragma once
#include <array>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rsrt.h"
#include "rsrt_bloom.h"
#include "rsrt_colour.h"
#include "rsrt_finish.h"
#include "rsrt_hdr.h"
#include "rsrt_jpeg.h"
#include "rsrt_video.h"
#include "rsrt_dof.h"
#include "rsrt_motion.h"
#include "rsrt_exposure.h"
#include "rsrt_fog.h"
#include "rsrt_host.h"
#include "rsrt_local.h"
#include "rsrt_sky.h"

namespace rsrt {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Scene::load_toml (src/scene.rs:235) + the uploads State::new derives from it
class Scene {
public:
    explicit Scene(const std::string &toml_path)
    {
        char err[2048] = {0};
        if (rsrt_scene_load_toml(toml_path.c_str(), &s_, err, sizeof err) != 0) throw Error(err);
        rsrt_scene_get_counts(s_, &counts_);
        rsrt_scene_get_camera(s_, &camera_);
    }
    ~Scene() { rsrt_scene_free(s_); }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;
    const rsrt_scene *handle() const { return s_; }
    const rsrt_scene_counts &counts() const { return counts_; }
    const rsrt_camera_desc &camera() const { return camera_; }

private:
    rsrt_scene *s_ = nullptr;
    rsrt_scene_counts counts_{};
    rsrt_camera_desc camera_{};
};

// one HDRI + its alias table (EnvironmentMaps::new, src/environments.rs:19-64)
struct Environment {
    uint32_t width = 0, height = 0;
    std::vector<float> rgba;
    std::vector<rsrt_alias_entry> alias;

    static Environment synthetic(uint32_t w, uint32_t h)
    {
        Environment e;
        e.width = w; e.height = h;
        e.rgba.resize((size_t)w * h * 4);
        if (rsrt_synth_environment(w, h, e.rgba.data()) != 0) throw Error("rsrt_synth_environment failed");
        e.build_alias();
        return e;
    }
    // the procedural daylight sky (rsrt_sky.h) on the CPU with the host alias table: what State::environment_sky builds on the device
    static Environment sky(uint32_t w, uint32_t h, const rsrt_sky_params &p)
    {
        Environment e;
        e.width = w; e.height = h;
        e.rgba.resize((size_t)w * h * 4);
        if (rsrt_sky_fill(w, h, &p, e.rgba.data()) != 0) throw Error("rsrt_sky_fill refused the size or the parameters");
        e.build_alias();
        return e;
    }
    static Environment from_hdr(const std::string &path)
    {
        Environment e;
        float *rgb = nullptr;
        char err[512] = {0};
        if (rsrt_load_hdr(path.c_str(), &e.width, &e.height, &rgb, err, sizeof err) != 0) throw Error(err);
        e.rgba.assign((size_t)e.width * e.height * 4, 0.0f);
        for (size_t i = 0; i < (size_t)e.width * e.height; i++) std::memcpy(&e.rgba[4 * i], &rgb[3 * i], 12);
        rsrt_free(rgb);
        e.build_alias();
        return e;
    }

private:
    void build_alias()
    {
        std::vector<float> rgb((size_t)width * height * 3);
        for (size_t i = 0; i < (size_t)width * height; i++) std::memcpy(&rgb[3 * i], &rgba[4 * i], 12);
        alias.resize((size_t)width * height);
        if (rsrt_alias_table_build(width, height, rgb.data(), alias.data(), nullptr) != 0) throw Error("rsrt_alias_table_build failed");
    }
};

class State {
public:
    // State::new (src/state.rs:60-649) over a LIST of devices of one node (rsrt_multi_*): device i renders the tiles
    // t % n == i, the frame is reduced onto devices[0] by RCCL inside librsrt whenever it is asked for.  {0} = one GPU.
    State(const Scene &scene, const std::vector<const Environment *> &environments, uint32_t width, uint32_t height,
          const std::vector<int> &devices = {0})
    {
        if (rsrt_multi_create(devices.data(), (uint32_t)devices.size(), &m_) != RSRT_OK) throw Error(rsrt_multi_last_error(nullptr));
        try {
            const rsrt_scene *s = scene.handle();
            const rsrt_scene_counts &c = scene.counts();
            check(rsrt_multi_upload_scene(m_, rsrt_scene_materials(s), c.n_materials, rsrt_scene_spheres(s), c.n_spheres, rsrt_scene_planes(s),
                                          c.n_planes, rsrt_scene_vertices(s), c.n_vertices, rsrt_scene_normals(s), c.n_normals,
                                          rsrt_scene_triangles(s), c.n_triangles, rsrt_scene_primitives(s), c.n_primitives, rsrt_scene_bvh_nodes(s),
                                          c.n_bvh_nodes));
            for (size_t i = 0; i < environments.size(); i++) {
                check(rsrt_multi_upload_environment(m_, (uint32_t)i, environments[i]->width, environments[i]->height, environments[i]->rgba.data(),
                                                    environments[i]->alias.data()));
                remember_environment((uint32_t)i, environments[i]->width, environments[i]->height);
            }
            camera_ = scene.camera();
            resize(width, height);
        } catch (...) {
            rsrt_multi_destroy(m_);
            throw;
        }
    }
    ~State() { rsrt_multi_destroy(m_); }
    State(const State &) = delete;
    State &operator=(const State &) = delete;

    uint32_t max_bounces = 10;      // MAX_BOUNCES (shader.wgsl:232)
    uint32_t environment_index = 0; // src/state.rs:638
    uint32_t flags = 0;

    // State::resize (src/state.rs:651-666)
    void resize(uint32_t width, uint32_t height)
    {
        check(rsrt_multi_resize(m_, width, height));
        width_ = width; height_ = height;
        have_hash_ = false;
    }
    // State::update (src/state.rs:722-758): the controller's result
    void update(const rsrt_camera_desc &camera) { camera_ = camera; }
    const rsrt_camera_desc &camera() const { return camera_; }
    uint32_t sample_count() const { return sample_count_; }
    uint32_t device_count() const { return rsrt_multi_size(m_); }

    // State::render (src/state.rs:760-833): one more sample per pixel; restart when the scene hash changed
    void render() { render_samples(1); }
    // aov = true: the denoiser's AOV pass over the same samples too (one device only, see render_aov)
    void render_samples(uint32_t n, bool aov = false)
    {
        const size_t h = scene_hash();
        if (!have_hash_ || h != last_hash_) { // src/state.rs:778-786
            last_hash_ = h; have_hash_ = true;
            check(rsrt_multi_clear(m_));
            sample_count_ = 0;
            if (have_aov_) clear_aov();
            if (guide_width_) clear_guide();
        }
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        check(rsrt_multi_render(m_, &cam, width_, height_, sample_count_, n, max_bounces, environment_index, flags));
        if (aov) render_aov(sample_count_, n);
        sample_count_ += n;
    }

    // -- the denoiser (rsrt.h "denoiser"): whole frame, so a State over one device -------------------------
    // rsrt_aov_render of samples [sample_begin, sample_begin + n) into device 0's AOV buffer (raw: no hash check)
    void render_aov(uint32_t sample_begin, uint32_t n)
    {
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        check_ctx(rsrt_aov_render(context(0), &cam, width_, height_, sample_begin, n, 0, nullptr));
        have_aov_ = true;
        aov_sample_count_ += n;
    }
    void clear_aov()
    {
        check_ctx(rsrt_aov_clear(context(0)));
        aov_sample_count_ = 0;
    }
    uint32_t aov_sample_count() const { return aov_sample_count_; }
    std::vector<float> download_aov() // W*H*8: albedo sum xyz, hits, normal sum xyz, distance sum
    {
        std::vector<float> out((size_t)width_ * height_ * 8);
        check_ctx(rsrt_aov_download(context(0), out.data(), out.size()));
        return out;
    }
    static rsrt_denoise_params denoise_defaults() { return rsrt_denoise_params{5u, RSRT_DENOISE_DEMODULATE, 2.0f, 0.5f, 0.3f}; }
    // the variance-guided filter (rsrt.h RSRT_DENOISE_VARIANCE): sigma_color is sigma_l, 4.0 (RSRT_SV_SIGMA_L); add RSRT_DENOISE_CLAMP for
    // the firefly clamp and RSRT_DENOISE_TEMPORAL (after render_temporal(n, p, true)) for the temporal moments
    static rsrt_denoise_params variance_defaults() { return rsrt_denoise_params{5u, RSRT_DENOISE_DEMODULATE | RSRT_DENOISE_VARIANCE, 4.0f, 0.5f, 0.3f}; }
    // rsrt_denoise of the mean of sample_count() samples, guided by aov_sample_count() AOV samples: W*H*4 f32 (alpha 1)
    std::vector<float> denoise(const rsrt_denoise_params &p = denoise_defaults())
    {
        check_ctx(rsrt_denoise(context(0), sample_count_, aov_sample_count_, &p, nullptr, nullptr));
        std::vector<float> out((size_t)width_ * height_ * 4);
        check_ctx(rsrt_denoised_download(context(0), out.data(), out.size()));
        return out;
    }
    // -- guided upsampling (rsrt.h "guided upsampling"): one device, like the denoiser -----------------------------
    // The State's own size is the LOW size the paths are traced at; the guide has the output's.  The caller picks a low size of the
    // output's aspect (ceil(W / 2) x ceil(H / 2) for half size).  The guide wants as many samples as the low frame.
    // rsrt_guide_render of samples [sample_begin, sample_begin + n) for a frame of width x height into device 0's guide (raw: no hash check)
    void render_guide(uint32_t width, uint32_t height, uint32_t sample_begin, uint32_t n)
    {
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        check_ctx(rsrt_guide_render(context(0), &cam, width, height, sample_begin, n, 0, nullptr));
        guide_width_ = width; guide_height_ = height;
        guide_sample_count_ += n;
    }
    void clear_guide()
    {
        check_ctx(rsrt_guide_clear(context(0)));
        guide_sample_count_ = 0;
    }
    uint32_t guide_sample_count() const { return guide_sample_count_; }
    uint32_t guide_width() const { return guide_width_; }
    uint32_t guide_height() const { return guide_height_; }
    std::vector<float> download_guide() // W*H*8 of the guide's size: albedo sum xyz, hits, normal sum xyz, distance sum
    {
        std::vector<float> out((size_t)guide_width_ * guide_height_ * 8);
        check_ctx(rsrt_guide_download(context(0), out.data(), out.size()));
        return out;
    }
    static rsrt_upsample_params upsample_defaults() { return rsrt_upsample_params{RSRT_UPSAMPLE_DEMODULATE, 0.5f, 0.3f}; }
    // rsrt_upsample of the low frame to the guide's size: W*H*4 f32 (alpha 1).  The low colour is the mean of sample_count() samples, or
    // with RSRT_UPSAMPLE_DENOISED / RSRT_UPSAMPLE_TEMPORAL in p.flags the last denoise() output / the last render_temporal frame's colour.
    std::vector<float> upsample(const rsrt_upsample_params &p = upsample_defaults())
    {
        check_ctx(rsrt_upsample(context(0), sample_count_, aov_sample_count_, guide_sample_count_, &p, nullptr, nullptr));
        std::vector<float> out((size_t)guide_width_ * guide_height_ * 4);
        check_ctx(rsrt_upsampled_download(context(0), out.data(), out.size()));
        return out;
    }
    std::vector<uint8_t> upsampled_display() // the last upsample() through the display pass
    {
        std::vector<uint8_t> out((size_t)guide_width_ * guide_height_ * 4);
        check_ctx(rsrt_upsampled_display_srgb8(context(0), out.data(), out.size()));
        return out;
    }
    // one progressive step of a picture of out_width x out_height traced at the State's own (low) size: render_samples(n, true), the
    // guide over the same samples at the output size (a changed camera / environment cleared it with the accumulator; another size
    // starts it anew), denoise() and the upsample of its output — or of the mean with denoise = false
    std::vector<float> render_upsampled(uint32_t out_width, uint32_t out_height, uint32_t n = 1, bool denoise = true)
    {
        const uint32_t begin = (have_hash_ && scene_hash() == last_hash_) ? sample_count_ : 0u;
        render_samples(n, true);
        if (guide_width_ != out_width || guide_height_ != out_height) guide_sample_count_ = 0; // a guide of another size is allocated zeroed
        render_guide(out_width, out_height, begin, n);
        rsrt_upsample_params p = upsample_defaults();
        if (denoise) {
            const rsrt_denoise_params d = denoise_defaults();
            check_ctx(rsrt_denoise(context(0), sample_count_, aov_sample_count_, &d, nullptr, nullptr));
            p.flags |= RSRT_UPSAMPLE_DENOISED;
        }
        return upsample(p);
    }
    // -- the noise estimate (rsrt.h "noise estimate"): one device, like the denoiser -------------------------------
    struct NoiseRound { uint32_t n1, n2; float max_error, mean_error; uint32_t tiles_above; };
    static rsrt_noise_params noise_defaults() { return rsrt_noise_params{16u, 16u, 0.0f, 0u}; }
    void noise_snapshot() { check_ctx(rsrt_noise_snapshot(context(0), sample_count_, nullptr)); } // a copy of the sum of sample_count() samples
    // rsrt_noise_estimate of the accumulator against the last noise_snapshot(): the tile map, tiles_y rows of tiles_x; *summary when given
    std::vector<float> noise_estimate(const rsrt_noise_params &p = noise_defaults(), rsrt_noise_summary *summary = nullptr)
    {
        check_ctx(rsrt_noise_estimate(context(0), sample_count_, &p, nullptr));
        return noise_download(summary);
    }
    std::vector<float> noise_download(rsrt_noise_summary *summary = nullptr) // the last noise_estimate()
    {
        rsrt_noise_summary s;
        check_ctx(rsrt_noise_download(context(0), nullptr, 0, &s));
        std::vector<float> tiles((size_t)s.tiles_x * s.tiles_y);
        check_ctx(rsrt_noise_download(context(0), tiles.data(), tiles.size(), &s));
        if (summary) *summary = s;
        return tiles;
    }
    void noise_reset() { check_ctx(rsrt_noise_reset(context(0))); }
    // renders until the largest tile error is at most `threshold` or max_samples are in: clears and renders min_samples, then per round
    // snapshots at n samples, renders up to min(2 n, max_samples) and estimates.  Returns the rounds; sample_count() is the total.  The
    // accumulator is what render_samples(total) leaves from a clear, bit for bit.  exposure: 0 compares the errors with `threshold`
    // itself; E > 0, or kAutoExposure (metered once with blend 1 after the min_samples render, and remembered), compares them with
    // threshold / sqrt(E) in f32: the threshold is then in displayed units.
    static constexpr float kAutoExposure = -1.0f;
    std::vector<NoiseRound> render_to_noise(float threshold, uint32_t min_samples = 8, uint32_t max_samples = 1024, uint32_t tile_w = 16,
                                            uint32_t tile_h = 16, float exposure = 0.0f)
    {
        if (min_samples < 1 || max_samples <= min_samples) throw Error("render_to_noise: 1 <= min_samples < max_samples");
        have_hash_ = false; // start from a clear, whatever was rendered before
        render_samples(min_samples);
        if (exposure != 0.0f) {
            if (exposure == kAutoExposure) {
                exposure_ = 0.0f;
                exposure = auto_exposure().exposure;
            }
            threshold = threshold / rsrt_sqrtf(exposure);
        }
        std::vector<NoiseRound> rounds;
        for (;;) {
            const uint32_t n1 = sample_count_;
            noise_snapshot();
            render_samples((2u * n1 < max_samples ? 2u * n1 : max_samples) - n1);
            rsrt_noise_summary s;
            noise_estimate(rsrt_noise_params{tile_w, tile_h, threshold, 0u}, &s);
            rounds.push_back(NoiseRound{n1, sample_count_, s.max_error, s.mean_error, s.tiles_above});
            if (s.max_error <= threshold || sample_count_ >= max_samples) return rounds;
        }
    }
    // -- auto-exposure (rsrt.h "auto-exposure"): one device, like the denoiser ---------------------------------------
    static rsrt_exposure_params exposure_defaults()
    {
        return rsrt_exposure_params{RSRT_EXPOSURE_LOW_PERMILLE, RSRT_EXPOSURE_HIGH_PERMILLE, RSRT_EXPOSURE_KEY, RSRT_EXPOSURE_MIN, RSRT_EXPOSURE_MAX,
                                    RSRT_EXPOSURE_BLEND, RSRT_EXPOSURE_PREVIOUS, 0u};
    }
    // the luminance histogram of `source` (RSRT_EXPOSURE_MEAN: the accumulator over sample_count() samples), built on the device
    void exposure_meter(uint32_t source = RSRT_EXPOSURE_MEAN) { check_ctx(rsrt_exposure_meter(context(0), source, sample_count_, nullptr)); }
    // the last exposure_meter(): its 257 words (256 bins, the skipped pixels) and, when given, the exposure of it under p
    std::vector<uint32_t> exposure_download(const rsrt_exposure_params &p = exposure_defaults(), rsrt_exposure_result *result = nullptr)
    {
        std::vector<uint32_t> hist(RSRT_EXPOSURE_WORDS);
        check_ctx(rsrt_exposure_download(context(0), &p, hist.data(), hist.size(), result));
        return hist;
    }
    // meters `source`, downloads with the remembered exposure as previous_exposure and remembers the new one: the first call takes the
    // target, later ones move a fraction `blend` of the way to it
    rsrt_exposure_result auto_exposure(uint32_t source = RSRT_EXPOSURE_MEAN, float blend = 1.0f, rsrt_exposure_params p = exposure_defaults())
    {
        exposure_meter(source);
        p.blend = blend;
        p.previous_exposure = exposure_;
        rsrt_exposure_result r;
        exposure_download(p, &r);
        exposure_ = r.exposure;
        return r;
    }
    float exposure() const { return exposure_; } // the remembered exposure (0: none)
    void exposure_reset() // forgets the remembered exposure and drops the histogram
    {
        exposure_ = 0.0f;
        check_ctx(rsrt_exposure_reset(context(0)));
    }
    // `source` through the display pass at `exposure` (0: the remembered one); of the source's own size
    std::vector<uint8_t> display_exposed(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f)
    {
        if (exposure == 0.0f) {
            if (exposure_ == 0.0f) throw Error("display_exposed: no remembered exposure (auto_exposure first): RSRT_ERR_NOT_READY");
            exposure = exposure_;
        }
        return displayed(rsrt_display_exposed_srgb8, source, exposure);
    }
    // -- bloom (rsrt.h "bloom"): one device, like the denoiser -----------------------------------------------------
    static rsrt_bloom_params bloom_defaults() { return rsrt_bloom_params{RSRT_BLOOM_LEVELS, RSRT_BLOOM_FLAGS, RSRT_BLOOM_THRESHOLD, 0.0f}; }
    // the bloom image of `source` at `exposure` (0: the remembered one, else 1), built on the device
    void bloom(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const rsrt_bloom_params &p = bloom_defaults())
    {
        check_ctx(rsrt_bloom(context(0), source, sample_count_, exposure_or_one(exposure), &p, nullptr));
    }
    // the last bloom(): RGBA32F, alpha 1, ceil(width / 2) x ceil(height / 2) of its source; the size where asked for
    std::vector<float> bloom_download(uint32_t *width = nullptr, uint32_t *height = nullptr)
    {
        uint32_t w = 0, h = 0;
        check_ctx(rsrt_bloom_download(context(0), nullptr, 0, &w, &h));
        std::vector<float> out((size_t)w * h * 4);
        check_ctx(rsrt_bloom_download(context(0), out.data(), out.size(), width, height));
        return out;
    }
    void bloom_reset() { check_ctx(rsrt_bloom_reset(context(0))); } // drops the bloom image
    // `source` through the display pass at `exposure` (0: the remembered one, else 1 — what bloom() took) with `intensity` times the
    // doubled bloom image added before the tone map; of the source's own size
    std::vector<uint8_t> display_bloomed(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, float intensity = RSRT_BLOOM_INTENSITY)
    {
        return displayed(rsrt_display_bloomed_srgb8, source, exposure_or_one(exposure), intensity);
    }
    // -- local exposure (rsrt.h "local exposure"): one device, like the denoiser --------------------------------------
    static rsrt_local_params local_defaults()
    {
        return rsrt_local_params{RSRT_LOCAL_SHADOWS, RSRT_LOCAL_HIGHLIGHTS, RSRT_LOCAL_KEY, RSRT_LOCAL_MAX_STOPS, 0u, 0u};
    }
    // the blurred bilateral grid of `source` (unexposed), built on the device in cells of `cell` pixels
    void local_exposure(uint32_t source = RSRT_EXPOSURE_MEAN, uint32_t cell = RSRT_LOCAL_CELL)
    {
        check_ctx(rsrt_local_exposure(context(0), source, sample_count_, cell, nullptr));
    }
    // the last local_exposure(): z-major, then y, then x, two words a cell (count, sum of q); gx, gy, gz, cell where asked for
    std::vector<uint32_t> local_exposure_download(uint32_t dims_out[4] = nullptr)
    {
        uint32_t dims[4] = {0, 0, 0, 0};
        check_ctx(rsrt_local_exposure_download(context(0), nullptr, 0, dims));
        std::vector<uint32_t> out((size_t)dims[0] * dims[1] * dims[2] * 2);
        check_ctx(rsrt_local_exposure_download(context(0), out.data(), out.size(), dims_out));
        return out;
    }
    void local_exposure_reset() { check_ctx(rsrt_local_exposure_reset(context(0))); } // drops the grid
    // the gain display_local() multiplies every pixel of `source` by at `exposure` (0: the remembered one, else 1)
    std::vector<float> local_gain(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const rsrt_local_params &p = local_defaults())
    {
        std::vector<float> out(source_pixels(source));
        check_ctx(rsrt_local_gain_download(context(0), source, sample_count_, exposure_or_one(exposure), &p, out.data(), out.size()));
        return out;
    }
    // `source` through the display pass at `exposure` (0: the remembered one, else 1) with the local gain of the last local_exposure()
    // and, with bloom_intensity > 0, the last bloom() added before it; of the source's own size
    std::vector<uint8_t> display_local(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const rsrt_local_params &p = local_defaults(),
                                       float bloom_intensity = 0.0f)
    {
        return displayed(rsrt_display_local_srgb8, source, exposure_or_one(exposure), &p, bloom_intensity);
    }
    // -- white balance and colour grading (rsrt.h "white balance and colour grading"): one device, like the denoiser ----
    static rsrt_white_params white_defaults()
    {
        return rsrt_white_params{RSRT_WHITE_GATE, RSRT_WHITE_ITERATIONS, RSRT_WHITE_MIN_PERMILLE, RSRT_WHITE_STRENGTH, RSRT_WHITE_MAX_STOPS, RSRT_WHITE_BLEND,
                                 {0.0f, 0.0f, 0.0f}, 0u};
    }
    static rsrt_cdl_params cdl_defaults()
    {
        return rsrt_cdl_params{{RSRT_CDL_SLOPE, RSRT_CDL_SLOPE, RSRT_CDL_SLOPE}, {RSRT_CDL_OFFSET, RSRT_CDL_OFFSET, RSRT_CDL_OFFSET},
                               {RSRT_CDL_POWER, RSRT_CDL_POWER, RSRT_CDL_POWER}, RSRT_CDL_SATURATION, 0u, 0u};
    }
    // the chroma histogram of `source` (RSRT_EXPOSURE_MEAN: the accumulator over sample_count() samples), built on the device
    void white_meter(uint32_t source = RSRT_EXPOSURE_MEAN) { check_ctx(rsrt_white_meter(context(0), source, sample_count_, nullptr)); }
    // the last white_meter(): its 4097 words (64 x 64 bins, the skipped pixels) and, when given, the white point of it under p
    std::vector<uint32_t> white_download(const rsrt_white_params &p = white_defaults(), rsrt_white_result *result = nullptr)
    {
        std::vector<uint32_t> hist(RSRT_WHITE_WORDS);
        check_ctx(rsrt_white_download(context(0), &p, hist.data(), hist.size(), result));
        return hist;
    }
    // meters `source`, downloads with the remembered white point as `previous` and remembers the new one: the first call takes the
    // target, later ones move a fraction `blend` of the way to it
    rsrt_white_result auto_white_balance(uint32_t source = RSRT_EXPOSURE_MEAN, float blend = 1.0f, rsrt_white_params p = white_defaults())
    {
        white_meter(source);
        p.blend = blend;
        for (int i = 0; i < 3; i++) p.previous[i] = white_[i];
        rsrt_white_result r;
        white_download(p, &r);
        for (int i = 0; i < 3; i++) white_[i] = r.white[i];
        return r;
    }
    std::array<float, 3> white() const { return white_; } // the remembered white point (all 0: none)
    void white_reset() // forgets the remembered white point and drops the histogram
    {
        white_ = {0.0f, 0.0f, 0.0f};
        check_ctx(rsrt_white_reset(context(0)));
    }
    // bakes the CDL into a size^3 LUT on the device
    void colour_lut(const rsrt_cdl_params &cdl = cdl_defaults(), uint32_t size = RSRT_COLOUR_LUT_SIZE)
    {
        check_ctx(rsrt_colour_lut_build(context(0), size, &cdl, nullptr));
    }
    // a LUT from the host: 3 * n^3 floats, red fastest, encoded rgb in [0, 1]
    void colour_lut_upload(uint32_t n, const std::vector<float> &rgb) { check_ctx(rsrt_colour_lut_upload(context(0), n, rgb.data(), rgb.size())); }
    std::vector<float> colour_lut_download(uint32_t *n_out = nullptr)
    {
        uint32_t n = 0;
        check_ctx(rsrt_colour_lut_download(context(0), nullptr, 0, &n));
        std::vector<float> out((size_t)n * n * n * 3);
        check_ctx(rsrt_colour_lut_download(context(0), out.data(), out.size(), n_out));
        return out;
    }
    void colour_lut_reset() { check_ctx(rsrt_colour_lut_reset(context(0))); } // drops the LUT
    // `source` through the colour display at `exposure` (0: the remembered one, else 1): `white` (NULL: the remembered white point, else
    // 1) before the tone map, the LUT behind it at lut_strength (negative: 1 with a LUT, 0 without); local: NULL for no local grade,
    // else the last local_exposure()'s gain under it; with bloom_intensity > 0 the last bloom() is added.  Of the source's own size
    std::vector<uint8_t> display_colour(uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const float *white = nullptr, float lut_strength = -1.0f,
                                        const rsrt_local_params *local = nullptr, float bloom_intensity = 0.0f)
    {
        const rsrt_colour_params c = colour_params(white, lut_strength);
        return displayed(rsrt_display_colour_srgb8, source, exposure_or_one(exposure), local, bloom_intensity, &c);
    }
    // -- finished display (rsrt.h "finished display"): one device, like the denoiser --------------------------------------
    static rsrt_finish_params finish_defaults()
    {
        return rsrt_finish_params{RSRT_FINISH_SHARPNESS, RSRT_FINISH_GRAIN, RSRT_FINISH_DITHER, RSRT_FINISH_SEED, RSRT_FINISH_FLAGS, {0u, 0u, 0u}};
    }
    // display_colour (whose arguments source .. bloom_intensity are) with the sharpener, the film grain and the dithered quantiser of
    // `finish` behind the LUT; finish.seed seeds the noise: a frame index for grain that moves, the same seed for the same bytes
    std::vector<uint8_t> display_finished(const rsrt_finish_params &finish = finish_defaults(), uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f,
                                          const float *white = nullptr, float lut_strength = -1.0f, const rsrt_local_params *local = nullptr,
                                          float bloom_intensity = 0.0f)
    {
        const rsrt_colour_params c = colour_params(white, lut_strength);
        return displayed(rsrt_display_finished_srgb8, source, exposure_or_one(exposure), local, bloom_intensity, &c, &finish);
    }
    // -- HDR display (rsrt.h "HDR display"): one device, like the denoiser -------------------------------------------------
    static rsrt_hdr_params hdr_defaults()
    {
        return rsrt_hdr_params{RSRT_HDR_PAPER_WHITE, RSRT_HDR_PEAK, RSRT_HDR_KNEE, RSRT_HDR_DITHER, RSRT_HDR_SEED, RSRT_HDR_ENCODING, RSRT_HDR_FLAGS, 0u};
    }
    // display_colour's chain up to its tone map (whose arguments source .. bloom_intensity are; there is no LUT here) under hdr.peak_nits
    // and encoded as hdr.encoding says: the bytes of one uint32 a pixel (RSRT_HDR_PQ10) or of four binary16 a pixel (RSRT_HDR_SCRGB16F).
    // levels: NULL, or where the frame's content light levels go
    std::vector<uint8_t> display_hdr(const rsrt_hdr_params &hdr = hdr_defaults(), rsrt_hdr_levels *levels = nullptr, uint32_t source = RSRT_EXPOSURE_MEAN,
                                     float exposure = 0.0f, const float *white = nullptr, const rsrt_local_params *local = nullptr, float bloom_intensity = 0.0f)
    {
        const rsrt_colour_params c = colour_params(white, 0.0f);
        std::vector<uint8_t> out(source_pixels(source) * (hdr.encoding == RSRT_HDR_SCRGB16F ? 8u : 4u));
        check_ctx(rsrt_display_hdr(context(0), source, sample_count_, exposure_or_one(exposure), local, bloom_intensity, &c, &hdr, out.data(), out.size(), levels));
        return out;
    }
    // -- video output (rsrt.h "video output"): one device, like the denoiser ----------------------------------------------
    static rsrt_video_params video_defaults()
    {
        return rsrt_video_params{RSRT_VIDEO_DEFAULT_STANDARD, RSRT_VIDEO_DEFAULT_DEPTH, RSRT_VIDEO_DEFAULT_LAYOUT, RSRT_VIDEO_DEFAULT_RANGE, RSRT_VIDEO_DEFAULT_SITING,
                                 RSRT_VIDEO_DEFAULT_DITHER, RSRT_VIDEO_DEFAULT_SEED, RSRT_VIDEO_DEFAULT_FLAGS};
    }
    // display_colour's chain with its LUT (video.standard RSRT_VIDEO_BT709: hdr NULL) or display_hdr's (RSRT_VIDEO_HDR10: hdr given, no LUT) as
    // a Y'CbCr 4:2:0 frame: the bytes rsrt_video_planes lays out for the source's size.  levels: NULL, or (RSRT_VIDEO_HDR10) where the frame's
    // content light levels go.  lut_strength < 0: 1 with a LUT, 0 without or with hdr
    std::vector<uint8_t> display_video(const rsrt_video_params &video = video_defaults(), const rsrt_hdr_params *hdr = nullptr, rsrt_hdr_levels *levels = nullptr,
                                       uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const float *white = nullptr, float lut_strength = -1.0f,
                                       const rsrt_local_params *local = nullptr, float bloom_intensity = 0.0f)
    {
        const rsrt_colour_params c = colour_params(white, hdr && lut_strength < 0.0f ? 0.0f : lut_strength);
        uint32_t w = 0, h = 0;
        source_size(source, &w, &h);
        std::vector<uint8_t> out(rsrt_video_planes(w, h, &video, nullptr));
        check_ctx(rsrt_display_video(context(0), source, sample_count_, exposure_or_one(exposure), local, bloom_intensity, &c, hdr, &video, out.data(), out.size(), levels));
        return out;
    }
    // -- JPEG output (rsrt.h "JPEG output"): one device, like the denoiser -------------------------------------------------
    static rsrt_jpeg_params jpeg_defaults()
    {
        return rsrt_jpeg_params{RSRT_JPEG_DEFAULT_QUALITY, RSRT_JPEG_DEFAULT_SUBSAMPLING, RSRT_JPEG_DEFAULT_FLAGS, RSRT_JPEG_DEFAULT_RESERVED};
    }
    // display_colour's chain with its LUT as a complete baseline JPEG file, coded on the device.  The buffer is sized from a guess, an eighth of
    // the worst case, and the call is made once more with the size the library asks for.  lut_strength < 0: 1 with a LUT, 0 without
    std::vector<uint8_t> display_jpeg(const rsrt_jpeg_params &jpeg = jpeg_defaults(), uint32_t source = RSRT_EXPOSURE_MEAN, float exposure = 0.0f, const float *white = nullptr,
                                      float lut_strength = -1.0f, const rsrt_local_params *local = nullptr, float bloom_intensity = 0.0f)
    {
        const rsrt_colour_params c = colour_params(white, lut_strength);
        uint32_t w = 0, h = 0;
        source_size(source, &w, &h);
        const size_t limit = rsrt_jpeg_max_bytes(w, h, jpeg.subsampling);
        std::vector<uint8_t> out(limit ? RSRT_JPEG_HEADER_BYTES + 2u + limit / 8u : 1u);
        size_t n = 0;
        rsrt_status st = rsrt_display_jpeg(context(0), source, sample_count_, exposure_or_one(exposure), local, bloom_intensity, &c, &jpeg, out.data(), out.size(), &n);
        if (st != RSRT_OK && n > out.size() && n <= limit) { // (refused for the room alone: n is the size needed)
            out.resize(n);
            st = rsrt_display_jpeg(context(0), source, sample_count_, exposure_or_one(exposure), local, bloom_intensity, &c, &jpeg, out.data(), out.size(), &n);
        }
        check_ctx(st);
        out.resize(n);
        return out;
    }
    // -- depth of field (rsrt.h "depth of field"): one device, like the denoiser ----------------------------------------
    static rsrt_dof_params dof_defaults() { return rsrt_dof_params{RSRT_DOF_FOCUS_DISTANCE, RSRT_DOF_APERTURE, RSRT_DOF_RADIUS, RSRT_DOF_FLAGS}; }
    // the lens image of `source` (RSRT_EXPOSURE_MEAN .. _UPSAMPLED) seen through the state's camera, built on the device; a
    // focus_distance of 0 in p means the one focus_at() remembered, else the default.  The later passes take it as RSRT_EXPOSURE_LENS.
    void depth_of_field(uint32_t source = RSRT_EXPOSURE_MEAN, rsrt_dof_params p = rsrt_dof_params{0.0f, RSRT_DOF_APERTURE, RSRT_DOF_RADIUS, RSRT_DOF_FLAGS})
    {
        if (p.focus_distance == 0.0f) p.focus_distance = focus_distance_ != 0.0f ? focus_distance_ : RSRT_DOF_FOCUS_DISTANCE;
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        check_ctx(rsrt_dof(context(0), source, sample_count_, &cam, &p, nullptr, nullptr));
    }
    // the last depth_of_field(): RGBA32F, alpha 1, of its source's size; the size where asked for
    std::vector<float> dof_download(uint32_t *width = nullptr, uint32_t *height = nullptr)
    {
        std::vector<float> out(source_pixels(RSRT_EXPOSURE_LENS) * 4);
        check_ctx(rsrt_dof_download(context(0), out.data(), out.size(), width, height));
        return out;
    }
    std::vector<float> dof_coc() // the signed blur radii of the last depth_of_field(), in pixels (negative: near field)
    {
        std::vector<float> out(source_pixels(RSRT_EXPOSURE_LENS));
        check_ctx(rsrt_dof_coc_download(context(0), out.data(), out.size()));
        return out;
    }
    // autofocus: the depth along the optical axis at pixel (x, y) of `source`'s records, remembered as the focus distance of later
    // depth_of_field() calls; a sky pixel returns +inf and leaves the focus as it was
    float focus_at(uint32_t x, uint32_t y, uint32_t source = RSRT_EXPOSURE_MEAN)
    {
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        float z = 0.0f;
        check_ctx(rsrt_dof_depth_at(context(0), source, &cam, x, y, &z));
        if (rsrt_dof_finite(z) && z > 0.0f) focus_distance_ = z;
        return z;
    }
    float focus_distance() const { return focus_distance_; } // the remembered focus distance (0: none)
    void dof_reset() { check_ctx(rsrt_dof_reset(context(0))); } // drops the lens image
    // -- camera motion blur (rsrt.h "camera motion blur"): one device, like the denoiser -----------------------------------
    static rsrt_motion_params motion_defaults() { return rsrt_motion_params{RSRT_MOTION_SHUTTER, RSRT_MOTION_RADIUS, RSRT_MOTION_TAPS, RSRT_MOTION_FLAGS}; }
    // the motion image of `source` (RSRT_EXPOSURE_MEAN .. _LENS) seen through the state's camera after `previous`, the camera one frame
    // earlier, built on the device.  previous NULL: the camera of this state's last motion_blur(); on the first call, or after
    // motion_reset(), the current camera, and the output is the source.  Every call remembers its camera afterwards (the library keeps
    // none).  The later passes take the result as RSRT_EXPOSURE_MOTION.
    void motion_blur(uint32_t source = RSRT_EXPOSURE_MEAN, const rsrt_camera_desc *previous = nullptr, rsrt_motion_params p = motion_defaults())
    {
        rsrt_camera cam, prev;
        rsrt_camera_uniform(&camera_, &cam);
        rsrt_camera_uniform(previous ? previous : (have_motion_camera_ ? &motion_camera_ : &camera_), &prev);
        check_ctx(rsrt_motion_blur(context(0), source, sample_count_, &cam, &prev, &p, nullptr, nullptr));
        motion_camera_ = camera_;
        have_motion_camera_ = true;
    }
    // the last motion_blur(): RGBA32F, alpha 1, of its source's size; the size where asked for
    std::vector<float> motion_download(uint32_t *width = nullptr, uint32_t *height = nullptr)
    {
        std::vector<float> out(source_pixels(RSRT_EXPOSURE_MOTION) * 4);
        check_ctx(rsrt_motion_download(context(0), out.data(), out.size(), width, height));
        return out;
    }
    std::vector<float> motion_velocity() // the velocities of the last motion_blur(), in pixels: ux, uy, l a pixel
    {
        std::vector<float> out(source_pixels(RSRT_EXPOSURE_MOTION) * 3);
        check_ctx(rsrt_motion_velocity_download(context(0), out.data(), out.size()));
        return out;
    }
    // every 16 x 16 tile's own maximum of the last motion_blur(): ux, uy, l a tile, rows of *tiles_x
    std::vector<float> motion_tiles(uint32_t *tiles_x = nullptr, uint32_t *tiles_y = nullptr)
    {
        uint32_t tx = 0, ty = 0;
        check_ctx(rsrt_motion_tiles_download(context(0), nullptr, 0, &tx, &ty));
        std::vector<float> out((size_t)tx * ty * 3);
        check_ctx(rsrt_motion_tiles_download(context(0), out.data(), out.size(), tiles_x, tiles_y));
        return out;
    }
    void motion_reset() // drops the motion image and forgets the remembered camera
    {
        have_motion_camera_ = false;
        check_ctx(rsrt_motion_reset(context(0)));
    }
    // -- volumetric fog (rsrt.h "volumetric fog", rsrt_fog.h): one device, like the denoiser -------------------------------------
    // RSRT_FOG_*; the light has no default: straight up at irradiance 1 here, fog_light_from_sky() gives a sky's sun
    static rsrt_fog_params fog_defaults()
    {
        return rsrt_fog_params{RSRT_FOG_DENSITY, {RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO, RSRT_FOG_ALBEDO}, RSRT_FOG_ANISOTROPY, {0.0f, 1.0f, 0.0f}, {1.0f, 1.0f, 1.0f},
                               {RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT, RSRT_FOG_AMBIENT}, RSRT_FOG_MAX_DISTANCE, RSRT_FOG_STEPS, RSRT_FOG_FLAGS};
    }
    // p with the sun of the procedural sky of `sky` on a map of env_height rows as its light (rsrt_fog_light_from_sky)
    static rsrt_fog_params fog_light_from_sky(rsrt_fog_params p, const rsrt_sky_params &sky, uint32_t env_height = 1024)
    {
        if (!rsrt_sky_params_ok(&sky) || env_height == 0) throw Error("fog_light_from_sky: parameters rsrt_sky_params_ok does not accept, or a zero height");
        rsrt_fog_light_from_sky(&sky, env_height, p.light_dir, p.light_irradiance);
        return p;
    }
    // adds the fog of samples [sample_begin, sample_begin + n) of the state's camera and size to the fog records; raw, like render_aov:
    // fog_sample_count() grows by n and the state keeps p.  clear_fog() before a new camera or other parameters
    void render_fog(uint32_t sample_begin, uint32_t n, const rsrt_fog_params &p) { render_fog(sample_begin, n, p, width_, height_); }
    // ... to records of a size of their own: the guide's for the fog of the upsampled image, or half the source's for fog(source, true)
    void render_fog(uint32_t sample_begin, uint32_t n, const rsrt_fog_params &p, uint32_t width, uint32_t height)
    {
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        if (fog_width_ != width || fog_height_ != height) fog_sample_count_ = 0; // records of another size are allocated zeroed
        check_ctx(rsrt_fog_render(context(0), &cam, width, height, sample_begin, n, &p, nullptr));
        fog_width_ = width;
        fog_height_ = height;
        fog_params_ = p;
        fog_sample_count_ += n;
    }
    void render_fog(uint32_t n, const rsrt_fog_params &p) { render_fog(fog_sample_count_, n, p); } // progressive: from fog_sample_count()
    void render_fog(uint32_t n = 1) { render_fog(fog_sample_count_, n, fog_params_); }               // ... with the parameters of the call before
    void clear_fog()
    {
        check_ctx(rsrt_fog_clear(context(0)));
        fog_sample_count_ = 0;
    }
    std::vector<float> download_fog() // the records, W*H*4: inscatter sum rgb, transmittance sum
    {
        std::vector<float> out((size_t)fog_width_ * fog_height_ * 4);
        check_ctx(rsrt_fog_download(context(0), out.data(), out.size()));
        return out;
    }
    uint32_t fog_sample_count() const { return fog_sample_count_; }
    const rsrt_fog_params &fog_params() const { return fog_params_; } // what the records were rendered with
    // the fog image of `source` (RSRT_EXPOSURE_MEAN .. _UPSAMPLED) and the fog records, built on the device.  The later passes —
    // depth_of_field, motion_blur, the meters, bloom, local exposure, the displays — take it as RSRT_EXPOSURE_FOG.
    // upsample: the records are smaller than the source (rsrt_fog_apply_upsampled); the fog image is rebuilt from them, the source's
    // first-hit records (the guide for RSRT_EXPOSURE_UPSAMPLED, the AOV buffer otherwise) and fog_params().
    void fog(uint32_t source = RSRT_EXPOSURE_MEAN, bool upsample = false)
    {
        const size_t n = source_pixels(source);
        if (upsample)
            check_ctx(rsrt_fog_apply_upsampled(context(0), source, sample_count_, fog_sample_count_,
                                               source == RSRT_EXPOSURE_UPSAMPLED ? guide_sample_count_ : aov_sample_count_, &fog_params_, nullptr, nullptr));
        else
            check_ctx(rsrt_fog_apply(context(0), source, sample_count_, fog_sample_count_, nullptr, nullptr));
        fog_pixels_ = n;
    }
    std::vector<float> fog_download() // the last fog(): RGBA32F, alpha 1, of its source's size
    {
        std::vector<float> out(source_pixels(RSRT_EXPOSURE_FOG) * 4);
        check_ctx(rsrt_fog_image_download(context(0), out.data(), out.size()));
        return out;
    }
    void fog_reset() // drops the records and the fog image
    {
        check_ctx(rsrt_fog_reset(context(0)));
        fog_sample_count_ = fog_width_ = fog_height_ = 0;
        fog_pixels_ = 0;
    }
    // -- the procedural sky (rsrt.h rsrt_environment_sky, rsrt_sky.h) -----------------------------------------------------------
    static rsrt_sky_params sky_defaults()
    {
        return rsrt_sky_params{RSRT_SKY_SUN_AZIMUTH, RSRT_SKY_SUN_ELEVATION, RSRT_SKY_TURBIDITY, {RSRT_SKY_GROUND_ALBEDO, RSRT_SKY_GROUND_ALBEDO, RSRT_SKY_GROUND_ALBEDO},
                               RSRT_SKY_SCALE, RSRT_SKY_SUN_ILLUMINANCE, RSRT_SKY_SUN_RADIUS, RSRT_SKY_FLAGS};
    }
    // fills environment `slot` with the sky of p and builds its alias table, on every device of the State (each makes the same bits);
    // replaces what the slot held and, like an upload, drops the temporal history
    void environment_sky(uint32_t slot, uint32_t width = 2048, uint32_t height = 1024, const rsrt_sky_params &p = sky_defaults())
    {
        for (uint32_t i = 0; i < device_count(); i++)
            if (rsrt_environment_sky(context(i), slot, width, height, &p) != RSRT_OK) throw Error(rsrt_last_error(context(i)));
        remember_environment(slot, width, height);
    }
    // the texels of environment `slot` (a sky or an upload), width * height * 4 f32 with alpha 0, from device 0; the size where asked for
    std::vector<float> environment_download(uint32_t slot, uint32_t *width = nullptr, uint32_t *height = nullptr)
    {
        const uint32_t w = slot < env_sizes_.size() ? env_sizes_[slot].first : 0u, h = slot < env_sizes_.size() ? env_sizes_[slot].second : 0u;
        std::vector<float> out((size_t)w * h * 4);
        check_ctx(rsrt_environment_download(context(0), slot, out.data(), out.size()));
        if (width) *width = w;
        if (height) *height = h;
        return out;
    }
    // -- the temporal pass (rsrt.h "temporal pass"): one device, like the denoiser ---------------------------------
    static rsrt_temporal_params temporal_defaults() { return rsrt_temporal_params{32u, 0.05f, 0.9f}; }
    // one displayed frame: clear the accumulator and the AOV buffer, render samples [k, k + n) of the current camera with the AOV pass
    // (k only grows until temporal_reset: fresh random numbers every frame) and blend them with the reprojected history.  Resets the
    // history first when environment_index, max_bounces, flags or the size changed; afterwards sample_count() = aov_sample_count() = n
    // and a later render_samples starts clean.  denoise() with RSRT_DENOISE_TEMPORAL in the flags filters the result.  moments: keep the
    // luminance moments too (RSRT_TEMPORAL_MOMENTS, download_temporal_moments); toggling it resets the history.
    void render_temporal(uint32_t n = 1, const rsrt_temporal_params &p = temporal_defaults(), bool moments = false)
    {
        const uint32_t key[6] = {environment_index, max_bounces, flags, width_, height_, moments ? 1u : 0u};
        if (!have_temporal_key_ || std::memcmp(key, temporal_key_, sizeof key) != 0) {
            temporal_reset();
            std::memcpy(temporal_key_, key, sizeof key);
            have_temporal_key_ = true;
        }
        check(rsrt_multi_clear(m_));
        if (have_aov_) clear_aov();
        const uint32_t k = temporal_sample_count_;
        rsrt_camera cam;
        rsrt_camera_uniform(&camera_, &cam);
        check(rsrt_multi_render(m_, &cam, width_, height_, k, n, max_bounces, environment_index, flags));
        render_aov(k, n);
        check_ctx(rsrt_temporal_accumulate_ex(context(0), &cam, n, n, &p, moments ? RSRT_TEMPORAL_MOMENTS : 0u, nullptr));
        temporal_sample_count_ = k + n;
        sample_count_ = n;
        have_hash_ = false;
    }
    void temporal_reset() // the next render_temporal is a first frame, from sample 0
    {
        check_ctx(rsrt_temporal_reset(context(0)));
        temporal_sample_count_ = 0;
    }
    std::vector<float> download_temporal() // W*H*4: colour, sample weight
    {
        std::vector<float> out((size_t)width_ * height_ * 4);
        check_ctx(rsrt_temporal_download(context(0), out.data(), out.size()));
        return out;
    }
    std::vector<float> download_temporal_moments() // W*H*4: mu1, mu2, frames, scale (the last frame must have carried moments)
    {
        std::vector<float> out((size_t)width_ * height_ * 4);
        check_ctx(rsrt_temporal_moments_download(context(0), out.data(), out.size()));
        return out;
    }
    std::vector<uint8_t> denoised_display() // the last denoise() through the display pass
    {
        std::vector<uint8_t> out((size_t)width_ * height_ * 4);
        check_ctx(rsrt_denoised_display_srgb8(context(0), out.data(), out.size()));
        return out;
    }
    std::vector<float> download() // cumulative_light_texture, all devices' tiles
    {
        std::vector<float> out((size_t)width_ * height_ * 4);
        check(rsrt_multi_download(m_, out.data(), out.size()));
        return out;
    }
    std::vector<uint8_t> display() // what the window shows (hdr.wgsl + sRGB surface)
    {
        std::vector<uint8_t> out((size_t)width_ * height_ * 4);
        check(rsrt_multi_display_srgb8(m_, sample_count_, out.data(), out.size()));
        return out;
    }
    // scene.dev_index 2 / 3 (shader.wgsl:1314-1338): out_texture (RGBA binary16) as `main` leaves it for the developer views — 3: the HDRI
    // under the frame; 2: twenty draws of the alias table per pixel added onto `out_texture` (the previous frame's; zeros when empty)
    std::vector<uint16_t> debug_view(uint32_t dev_index, std::vector<uint16_t> out_texture = {})
    {
        out_texture.resize((size_t)width_ * height_ * 4, 0);
        const rsrt_status st = rsrt_debug_view_f16(context(0), dev_index, environment_index, sample_count_, out_texture.data(), out_texture.size());
        if (st != RSRT_OK) throw Error(rsrt_last_error(context(0)));
        return out_texture;
    }
    rsrt_stats stats()
    {
        rsrt_stats s;
        check(rsrt_multi_get_stats(m_, &s));
        return s;
    }
    // rsrt_selftest_sincos on the first device: {mismatches (must be 0), inputs checked (2^32), 0, first failing pattern or UINT64_MAX}
    std::array<uint64_t, 4> selftest_sincos()
    {
        std::array<uint64_t, 4> out{};
        check_ctx(rsrt_selftest_sincos(context(0), out.data()));
        return out;
    }
    rsrt_context *context(uint32_t i = 0) { return rsrt_multi_context(m_, i); }

private:
    void check(rsrt_status st)
    {
        if (st != RSRT_OK) throw Error(rsrt_multi_last_error(m_));
    }
    void check_ctx(rsrt_status st)
    {
        if (st != RSRT_OK) throw Error(rsrt_last_error(context(0)));
    }
    size_t scene_hash() const // SceneState: camera bits + environment index (src/scene.rs:255-262, src/camera.rs:92-100)
    {
        std::string bytes(reinterpret_cast<const char *>(&camera_), sizeof camera_);
        bytes.append(reinterpret_cast<const char *>(&environment_index), sizeof environment_index);
        return std::hash<std::string>()(bytes);
    }
    void remember_environment(uint32_t slot, uint32_t width, uint32_t height)
    {
        if (env_sizes_.size() <= slot) env_sizes_.resize(slot + 1, {0u, 0u});
        env_sizes_[slot] = {width, height};
    }
    std::vector<std::pair<uint32_t, uint32_t>> env_sizes_; // slot -> the size of what the constructor or environment_sky put there
    rsrt_multi *m_ = nullptr;
    rsrt_camera_desc camera_{};
    uint32_t width_ = 0, height_ = 0, sample_count_ = 0, aov_sample_count_ = 0;
    bool have_aov_ = false;
    uint32_t guide_width_ = 0, guide_height_ = 0, guide_sample_count_ = 0;
    uint32_t temporal_sample_count_ = 0, temporal_key_[6] = {0, 0, 0, 0, 0, 0};
    bool have_temporal_key_ = false;
    size_t last_hash_ = 0;
    bool have_hash_ = false;
    float exposure_ = 0.0f; // the last auto_exposure() (0: none since exposure_reset)
    std::array<float, 3> white_ = {0.0f, 0.0f, 0.0f}; // the last auto_white_balance() (all 0: none since white_reset)
    float exposure_or_one(float exposure) const { return exposure != 0.0f ? exposure : (exposure_ != 0.0f ? exposure_ : 1.0f); }
    float focus_distance_ = 0.0f; // the last focus_at() that hit a surface (0: none)
    rsrt_camera_desc motion_camera_{}; // the camera of the last motion_blur()
    bool have_motion_camera_ = false;
    uint32_t fog_sample_count_ = 0, fog_width_ = 0, fog_height_ = 0; // samples in the fog records and their size
    rsrt_fog_params fog_params_ = fog_defaults();                    // what the last render_fog took
    size_t fog_pixels_ = 0;                                          // the pixels of the last fog() image (0: none)
    // the pixels of `source`: the guide's for RSRT_EXPOSURE_UPSAMPLED, what the library holds for RSRT_EXPOSURE_LENS and _MOTION, else the state's own
    size_t source_pixels(uint32_t source)
    {
        if (source == RSRT_EXPOSURE_FOG && fog_pixels_) return fog_pixels_; // (the size of the source the last fog() composed)
        if (source == RSRT_EXPOSURE_MOTION) {
            uint32_t w = 0, h = 0;
            check_ctx(rsrt_motion_download(context(0), nullptr, 0, &w, &h));
            return (size_t)w * h;
        }
        if (source == RSRT_EXPOSURE_LENS) {
            uint32_t w = 0, h = 0;
            check_ctx(rsrt_dof_download(context(0), nullptr, 0, &w, &h));
            return (size_t)w * h;
        }
        const bool up = source == RSRT_EXPOSURE_UPSAMPLED;
        return (size_t)(up ? guide_width_ : width_) * (up ? guide_height_ : height_);
    }
    // ... and its width and height (a fogged image is of the guide's size when that is the size the last fog() composed, else of the state's own)
    void source_size(uint32_t source, uint32_t *w, uint32_t *h)
    {
        if (source == RSRT_EXPOSURE_MOTION) {
            check_ctx(rsrt_motion_download(context(0), nullptr, 0, w, h));
            return;
        }
        if (source == RSRT_EXPOSURE_LENS) {
            check_ctx(rsrt_dof_download(context(0), nullptr, 0, w, h));
            return;
        }
        const size_t own = (size_t)width_ * height_, guide = (size_t)guide_width_ * guide_height_;
        const bool up = source == RSRT_EXPOSURE_UPSAMPLED || (source == RSRT_EXPOSURE_FOG && fog_pixels_ == guide && guide != own);
        *w = up ? guide_width_ : width_;
        *h = up ? guide_height_ : height_;
    }
    // a display into a vector: display(context, source, sample_count, args..., bytes, their number), RGBA8 of the source's own size
    template <class Display, class... Args>
    std::vector<uint8_t> displayed(Display display, uint32_t source, Args... args)
    {
        std::vector<uint8_t> out(source_pixels(source) * 4);
        check_ctx(display(context(0), source, sample_count_, args..., out.data(), out.size()));
        return out;
    }
    // the colour displays' parameters: `white` (NULL: the remembered white point, else 1) and lut_strength (negative: 1 with a LUT, 0 without)
    rsrt_colour_params colour_params(const float *white, float lut_strength)
    {
        const bool remembered = white_[0] != 0.0f;
        rsrt_colour_params c{{1.0f, 1.0f, 1.0f}, lut_strength, 0u, {0u, 0u, 0u}};
        for (int i = 0; i < 3; i++) c.white[i] = white ? white[i] : (remembered ? white_[i] : 1.0f);
        if (lut_strength < 0.0f) c.lut_strength = rsrt_colour_lut_download(context(0), nullptr, 0, nullptr) == RSRT_OK ? RSRT_COLOUR_LUT_STRENGTH : 0.0f;
        return c;
    }
};

} // namespace rsrt
