/*
 * rsrt_host.h — C-ABI of the host-side preprocessing (librsrt_host.so, CPU only).
 *
 * The reference does this work in Rust before it uploads anything;
 * a Rust host that keeps its own Scene/BVH/alias code does not need this library at all — it
 * passes its buffers straight to rsrt.h.  It exists so that a C/C++/Python host can produce
 * the SAME buffers: each function restates one reference function in C++ with the same f32
 * operation order.
 *
 *   rsrt_scene_load_toml     Scene::load_toml            src/scene.rs:233-441, src/mesh.rs:29-113
 *   rsrt_build_bvh           build_bvh                   src/bvh.rs:13-337
 *   rsrt_plane_to_uniform    Plane::to_uniform           src/scene.rs:190-201
 *   rsrt_camera_uniform      CameraUniform::new          src/camera.rs:26-28, :111-119
 *   rsrt_alias_table_build   AliasTable::build_by_luminance  src/environments.rs:96-187
 *   rsrt_load_hdr            image::load_from_memory(..).into_rgb32f() for Radiance .hdr  src/state.rs:119-132
 *   rsrt_camera_(de)serialize Camera::serialize / deserialize (--state)  src/camera.rs:30-89
 *   rsrt_display_srgb8_host  hdr.wgsl aces_tone_map + sRGB surface write  src/shaders/hdr.wgsl:3-22
 *   rsrt_write_png/_pfm      image output (the reference only presents to a window)
 *   rsrt_y4m_write           video output: the frames of rsrt_display_video as a YUV4MPEG2 sequence
 *   rsrt_synth_environment   stand-in for the two HDRIs the checkout lacks (state.rs:119-122;
 *                            .MISSING_LARGE_BLOBS) — deterministic formula, DESIGN.md §env
 *   rsrt_sky_fill            the procedural daylight sky of include/rsrt_sky.h on the CPU (no reference counterpart;
 *                            rsrt_environment_sky in rsrt.h fills a slot with the same bits on the device), DESIGN.md §19
 */
#ifndef RSRT_HOST_H
#define RSRT_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "rsrt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsrt_scene rsrt_scene;

typedef struct rsrt_scene_counts {
    uint32_t n_materials, n_spheres, n_planes, n_vertices, n_normals, n_triangles, n_primitives, n_bvh_nodes;
    uint32_t bvh_depth;
} rsrt_scene_counts;

/* Camera as the scene file / --state describe it (src/camera.rs:14-21); angles in radians. */
typedef struct rsrt_camera_desc {
    float pos[3];
    float yaw, pitch, fov_y;
} rsrt_camera_desc;

/* Scene::load_toml + PackedMeshes::pack_meshes + build_bvh.  On failure returns non-zero and
 * writes the reference's error text (src/scene.rs:236-249, :334-351, :413-427) into err. */
int rsrt_scene_load_toml(const char *path, rsrt_scene **out, char *err, size_t err_len);
void rsrt_scene_free(rsrt_scene *scene);
void rsrt_scene_get_counts(const rsrt_scene *scene, rsrt_scene_counts *out);
const rsrt_material *rsrt_scene_materials(const rsrt_scene *scene);
const rsrt_sphere *rsrt_scene_spheres(const rsrt_scene *scene);
const rsrt_plane_desc *rsrt_scene_plane_descs(const rsrt_scene *scene);
const rsrt_plane *rsrt_scene_planes(const rsrt_scene *scene);
const rsrt_vec3 *rsrt_scene_vertices(const rsrt_scene *scene);
const rsrt_vec3 *rsrt_scene_normals(const rsrt_scene *scene);
const rsrt_triangle *rsrt_scene_triangles(const rsrt_scene *scene);
const rsrt_primitive_info *rsrt_scene_primitives(const rsrt_scene *scene);
const rsrt_bvh_node *rsrt_scene_bvh_nodes(const rsrt_scene *scene);
void rsrt_scene_get_camera(const rsrt_scene *scene, rsrt_camera_desc *out);

/* build_bvh.  primitives_out: n_spheres+n_planes+n_triangles entries; nodes_out: room for
 * 2*that-1.  Returns 0 and the node count / tree depth; non-zero for an empty scene
 * (the reference asserts, src/bvh.rs:222). */
int rsrt_build_bvh(const rsrt_sphere *spheres, uint32_t n_spheres, const rsrt_plane_desc *planes, uint32_t n_planes,
                   const rsrt_vec3 *vertices, uint32_t n_vertices, const rsrt_triangle *triangles, uint32_t n_triangles,
                   rsrt_primitive_info *primitives_out, rsrt_bvh_node *nodes_out, uint32_t *n_nodes_out,
                   uint32_t *depth_out);

void rsrt_plane_to_uniform(const rsrt_plane_desc *in, rsrt_plane *out);
void rsrt_camera_uniform(const rsrt_camera_desc *in, rsrt_camera *out);

/* rgb: width*height*3 f32 (image::Rgb32FImage), rows top to bottom. out: width*height entries. */
int rsrt_alias_table_build(uint32_t width, uint32_t height, const float *rgb, rsrt_alias_entry *out, uint32_t *leftover_out);

/* Deterministic synthetic equirectangular sky (gradient + sun lobe); rgba_out: w*h*4, alpha 0. */
int rsrt_synth_environment(uint32_t width, uint32_t height, float *rgba_out);

/* The daylight sky of include/rsrt_sky.h (Preetham's, with a sun disc) as an equirectangular map; rgba_out: w*h*4, alpha 0.  Returns
 * non-zero for NULL arguments, a zero size or parameters rsrt_sky_params_ok refuses, and then writes nothing.
 * Rust: pub fn rsrt_sky_fill(width: u32, height: u32, params: *const RsrtSkyParams, rgba_out: *mut f32) -> i32; */
int rsrt_sky_fill(uint32_t width, uint32_t height, const rsrt_sky_params *params, float *rgba_out);
/* The sun of that sky on a map of env_height rows as the fog pass's light (rsrt_fog_light_from_sky, include/rsrt_fog.h): dir_out and
 * irradiance_out receive 3 floats each, rsrt_fog_params' light_dir and light_irradiance.  Returns non-zero for NULL arguments, a zero
 * height or parameters rsrt_sky_params_ok refuses, and then writes nothing.
 * Rust: pub fn rsrt_fog_sky_light(env_height: u32, params: *const RsrtSkyParams, dir_out: *mut f32, irradiance_out: *mut f32) -> i32; */
int rsrt_fog_sky_light(uint32_t env_height, const rsrt_sky_params *params, float *dir_out, float *irradiance_out);

/* Radiance RGBE (.hdr): rgb_out = malloc'ed width*height*3 f32, rows top to bottom; free with rsrt_free.
 * value = mantissa * 2^(e-136), (0,0,0) when e == 0 — the `image` 0.25 hdr decoder's rule. */
int rsrt_load_hdr(const char *path, uint32_t *width, uint32_t *height, float **rgb_out, char *err, size_t err_len);
void rsrt_free(void *p);

/* 24 bytes [pos.xyz, yaw, pitch, fov_y] little-endian f32 <-> standard base64 (32 chars + NUL).
 * Deserialize errors carry the reference's text ("Couldn't deserialize camera: binary data (N bytes) not 24 bytes"). */
void rsrt_camera_serialize(const rsrt_camera_desc *cam, char out[33]);
int rsrt_camera_deserialize(const char *encoded, rsrt_camera_desc *out, char *err, size_t err_len);

/* Display transform on the CPU (same inline code as the HIP kernel behind rsrt_display_srgb8). */
void rsrt_display_srgb8_host(const float *sum_rgba, size_t n_pixels, uint32_t sample_total, uint8_t *out_rgba8);

/* Image files: 8-bit RGBA PNG (stored deflate), 32-bit float PFM from a buffer with `stride_floats` per pixel. */
int rsrt_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgba8);
int rsrt_write_pfm(const char *path, uint32_t width, uint32_t height, const float *rgb, uint32_t stride_floats);
/* A frame of rsrt_display_video (include/rsrt.h "video output") into a YUV4MPEG2 file, the uncompressed sequence every encoder and player
 * reads.  append 0: the file is created and gets the stream header first — W, H, F fps_num:fps_den, Ip, A1:1, the colour space tag
 * (8 bits: C420mpeg2 for RSRT_VIDEO_SITING_LEFT, C420jpeg for RSRT_VIDEO_SITING_CENTRE; RSRT_VIDEO_SITING_TOPLEFT has no tag of its own
 * and gets the closest, C420mpeg2, which agrees along x; 10 bits: C420p10, the one 10-bit 4:2:0 tag there is, which names no siting),
 * XCOLORRANGE=LIMITED or FULL, and the comment fields XRSRT_SITING=LEFT | CENTRE | TOPLEFT and XRSRT_STANDARD=BT709 | HDR10, which say
 * what the tag cannot — ; append 1: the file must exist, and the caller keeps size, rate and video the same.  Then "FRAME" and the three
 * planes of planar_frame, n_bytes = rsrt_video_planes(width, height, video, ..).  video->layout must be RSRT_VIDEO_PLANAR: the format has
 * no interleaved chroma.  0: written; 1: an argument is refused; 2: the file cannot be opened; 3: a write failed. */
struct rsrt_video_params;
int rsrt_y4m_write(const char *path, int append, uint32_t width, uint32_t height, uint32_t fps_num, uint32_t fps_den, const struct rsrt_video_params *video,
                   const void *planar_frame, size_t n_bytes);

/* JPEG output (include/rsrt.h "JPEG output") on the CPU: the whole of include/rsrt_jpeg.h, sequential — the reference the device's file is
 * held to byte for byte.  sdr_rgb: display-referred linear RGB, 3 floats a pixel, rows top to bottom (what rsrt_finish_sdr gives: any
 * float is legal).  out receives the file when capacity suffices; *n_bytes_out is its size either way (rsrt_jpeg_max_bytes always
 * suffices; out may be NULL with capacity 0 to ask).  0: written; 1: an argument is refused (NULL, params rsrt_jpeg_params_ok refuses, a
 * size rsrt_jpeg_size_ok refuses: a side of 0 or above 65535, a worst case of 2^32 bits, the device's own limit) and nothing is written; 2: capacity is too small, *n_bytes_out says what is needed, out is untouched.
 * Rust: pub fn rsrt_jpeg_encode_host(sdr_rgb: *const f32, width: u32, height: u32, jpeg: *const RsrtJpegParams, out: *mut c_void,
 *                                    capacity: usize, n_bytes_out: *mut usize) -> i32; */
struct rsrt_jpeg_params;
int rsrt_jpeg_encode_host(const float *sdr_rgb, uint32_t width, uint32_t height, const struct rsrt_jpeg_params *jpeg, void *out, size_t capacity,
                          size_t *n_bytes_out);
/* Steps 1 to 5 alone: the quantised coefficients, int16 in zigzag order, 64 a block, blocks in scan order;
 * n_values = 64 * rsrt_jpeg_blocks(width, height, subsampling).  0 or 1 as above. */
int rsrt_jpeg_coefficients_host(const float *sdr_rgb, uint32_t width, uint32_t height, const struct rsrt_jpeg_params *jpeg, int16_t *coefs_out, size_t n_values);
/* The sequential entropy coder and the file alone, from coefficients in that layout; 1 also for another n_values and a value outside
 * [-1023, 1023] (a DC: [-1024, 1023]).  What rsrt_jpeg_encode_coefficients computes on the device. */
int rsrt_jpeg_from_coefficients(const int16_t *coefs, size_t n_values, uint32_t width, uint32_t height, const struct rsrt_jpeg_params *jpeg, void *out,
                                size_t capacity, size_t *n_bytes_out);
/* n_frames JPEG files of one size as one Motion-JPEG RIFF AVI 1.0 file, in one call: hdrl (avih; one strl: strh vids / MJPG, strf a
 * BITMAPINFOHEADER with biCompression MJPG, 24 bits), movi with one 00dc chunk a frame, padded to even, and idx1 with every frame a key
 * frame.  Stateless like rsrt_y4m_write: compressed frames are small enough to keep until the last is there.  0: written; 1: refused
 * (NULL, n_frames 0, a NULL or empty frame, a size or rate of 0, a file that would reach 2 GiB); 2: the file cannot be opened; 3: a
 * write failed.
 * Rust: pub fn rsrt_avi_mjpeg_write(path: *const c_char, frames: *const *const c_void, sizes: *const usize, n_frames: usize,
 *                                   width: u32, height: u32, fps_num: u32, fps_den: u32) -> i32; */
int rsrt_avi_mjpeg_write(const char *path, const void *const *frames, const size_t *sizes, size_t n_frames, uint32_t width, uint32_t height, uint32_t fps_num,
                         uint32_t fps_den);

#ifdef __cplusplus
}
#endif
#endif /* RSRT_HOST_H */
