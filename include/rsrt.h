/*
 * rsrt.h — C-ABI of the MI355X path-tracing integrator (librsrt.so).
 *
 * Drop-in boundary.  The reference has no FFI: its integrator is the WGSL compute shader
 * src/shaders/shader.wgsl (entry `main` :1305, `trace_ray` :1213) reached through three wgpu
 * bind groups that `State::new` builds (src/state.rs:60-649) and `State::render` dispatches
 * once per displayed frame (src/state.rs:760-833).  The entry points below are that bind-group
 * contract restated as plain C calls — what a Rust `extern "C"` block in src/state.rs would
 * bind (INTEGRATION.md shows the stub):
 *
 *   bind group 2 (scene storage buffers, state.rs:394-458)        -> rsrt_upload_scene
 *   bind group 0 bindings 2-5 (sampler, HDRIs, metadata, alias)   -> rsrt_upload_environment
 *   bind group 1 (camera/resolution/sample_count/env index)       -> arguments of rsrt_render
 *   bind group 0 binding 1 (cumulative_light_texture, RGBA32F sum) -> the accumulator
 *   bind group 0 binding 0 (out_texture, RGBA16F mean)             -> rsrt_resolve_mean_f16
 *   compute_pass.dispatch_workgroups (state.rs:808-824)            -> rsrt_render
 *   encoder.clear_texture(cumulative) on scene-hash change (:778-786) -> rsrt_accumulator_clear
 *
 * Semantics that differ from the reference on purpose:
 *   - one rsrt_render call may add MANY samples (the reference adds exactly one per frame);
 *     sample k of pixel p always uses the reference's RNG seed (pixel_index, k)
 *     (shader.wgsl:1309-1312), so any split over calls / tiles / GPUs gives the same image;
 *   - max_bounces is a run-time argument (the reference's constant is 10, shader.wgsl:232);
 *   - dev_index 1 (normal render) is rsrt_render; the developer views 2 / 3 (shader.wgsl:1314-1338) are rsrt_debug_view_f16.
 *
 * Threading: a context is used from one thread at a time, like `State`.  All functions return
 * an rsrt_status (0 = ok) and never throw/abort across the boundary; rsrt_last_error() gives
 * the message.  No CPU fallback exists: without a gfx950 device rsrt_context_create fails.
 */
#ifndef RSRT_H
#define RSRT_H

#include <stddef.h>
#include <stdint.h>

#include "rsrt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rsrt_status {
    RSRT_OK = 0,
    RSRT_ERR_INVALID_ARGUMENT = 1,
    RSRT_ERR_NO_DEVICE = 2,
    RSRT_ERR_HIP = 3,
    RSRT_ERR_NOT_READY = 4, /* scene or environment not uploaded / accumulator missing */
    RSRT_ERR_OUT_OF_MEMORY = 5,
    RSRT_ERR_COMM = 6 /* RCCL missing or a collective failed (multi-GPU only) */
} rsrt_status;

typedef struct rsrt_context rsrt_context;

/* flags of rsrt_render */
enum {
    /* Default (0): exactly the primitives the reference's unpruned walk tests are tested
     * (shader.wgsl:469-564), and of equal distances the one it visits first wins; only the NEE
     * shadow query, of which the shader reads nothing but `.did_hit` (:1249), stops at its
     * first hit.  That is exactly result-preserving.
     *
     * REFERENCE_TRAVERSAL: also run the shadow query to the end, as the shader literally does. */
    RSRT_FLAG_REFERENCE_TRAVERSAL = 1u,
    /* PRUNE: skip nodes whose slab entry lies beyond the current best hit.  NOT exactly
     * result-preserving: the slab entry t and a primitive's own t are rounded differently, and a
     * primitive a hair closer than the current best can sit in a skipped node.  Measured on
     * house.toml 1920x1080 x 256 spp: 2 of 5.3e8 paths change (per-channel RMSE 4e-7).  Opt-in;
     * honoured by the tree-walk traversals only (scenes of up to 64 primitives are not walked). */
    RSRT_FLAG_PRUNE = 2u
};

/* Counters of the work submitted since the previous rsrt_get_stats call (and cumulative since
 * context creation).  Times are HIP-event times on the stream the kernels were launched on. */
typedef struct rsrt_stats {
    uint64_t paths;        /* camera paths started */
    uint64_t ext_rays;     /* calls of cast_ray (shader.wgsl:1221) */
    uint64_t shadow_rays;  /* NEE queries actually issued (shader.wgsl:1246-1250) */
    double kernel_ms;      /* HIP-event time of the integrator kernel(s) on the launch stream */
    uint64_t total_paths, total_ext_rays, total_shadow_rays;
    double total_kernel_ms;
    uint32_t launches;     /* kernel launches since the previous rsrt_get_stats */
    uint32_t _pad;
    double trace_kernel_ms;   /* part of kernel_ms spent in the path-tracing kernel (rt_render_pool_kernel) */
    double resolve_kernel_ms; /* part spent in the ordered sample resolve (rt_resolve_kernel) */
    double reduce_ms;         /* HIP-event time of rsrt_comm_reduce calls (the RCCL reduce of the accumulators) */
    uint64_t traversal_steps; /* box tests + primitive tests of the BVH walks (0 where the flat small-scene loop runs:
                                 its work per ray is fixed by the scene); what RSRT_FLAG_PRUNE reduces */
} rsrt_stats;

/* -- context: State::new's device acquisition (state.rs:60-98) ------------------------------ */
rsrt_status rsrt_context_create(int device_index, rsrt_context **out);
void rsrt_context_destroy(rsrt_context *ctx);
/* Message of the last failing call on ctx; with ctx == NULL, of the last failing
 * rsrt_context_create or rsrt_scene_image_build on this thread. Never NULL. */
const char *rsrt_last_error(const rsrt_context *ctx);

/* -- scene: bind group 2, the eight storage buffers (state.rs:394-458) -----------------------
 * Arrays are in the layouts of rsrt_types.h; the library copies and re-lays them out for the
 * device, the caller keeps ownership.  Any array may be empty (pointer ignored when count 0)
 * except bvh_nodes.  Indices are validated; an out-of-range index is RSRT_ERR_INVALID_ARGUMENT.
 * A context may be given a new scene at any time: the next render, probe or AOV pass uses it.  Every call, a refused one
 * included, drops the temporal history first thing (rsrt_temporal_download is RSRT_ERR_NOT_READY until the next temporal frame).
 * A REFUSED call: every array, every index and the tree's shape are checked before the scene is touched, so a call refused for
 * any of them leaves the previous scene in place (it still renders, the same image and ray counts) and the accumulator as it was.
 * One refusal comes later: a valid tree deeper than the traversal stack holds (more than 128 levels: "bvh depth ... exceeds the
 * supported traversal stack", RSRT_ERR_INVALID_ARGUMENT) is found after the previous scene has been freed.  The context then has
 * NO scene: rsrt_render, rsrt_cast_rays and rsrt_aov_render return RSRT_ERR_NOT_READY until the next successful upload; the
 * accumulator is untouched. */
rsrt_status rsrt_upload_scene(rsrt_context *ctx,
                              const rsrt_material *materials, uint32_t n_materials,
                              const rsrt_sphere *spheres, uint32_t n_spheres,
                              const rsrt_plane *planes, uint32_t n_planes,
                              const rsrt_vec3 *vertices, uint32_t n_vertices,
                              const rsrt_vec3 *normals, uint32_t n_normals,
                              const rsrt_triangle *triangles, uint32_t n_triangles,
                              const rsrt_primitive_info *primitives, uint32_t n_primitives,
                              const rsrt_bvh_node *bvh_nodes, uint32_t n_bvh_nodes);

/* -- environment: bind group 0 bindings 3-5 (state.rs:119-132, environments.rs:19-64) --------
 * slot = index into the reference's binding_array / `environments` array.  rgba: width*height*4
 * f32, rows top to bottom, alpha ignored (texture.rs:112-115 writes 0).  alias: width*height
 * entries as AliasTable::build_by_luminance produces (rsrt_host.h has that builder), or NULL to have the
 * library build the table on the device (rsrt_environment_build_alias below).
 * Slots are 0 .. 63 and need not be filled in order: a slot below the highest one may stay empty, and rendering with an empty slot
 * is RSRT_ERR_NOT_READY (nothing is launched, the accumulator is not touched).  Uploading to a filled slot replaces it, whatever
 * the two sizes.  Every call, a refused one included, drops the temporal history first thing.  A REFUSED call (NULL data, a zero
 * size, slot > 63, an alias_index out of range: all RSRT_ERR_INVALID_ARGUMENT) leaves every slot, the one it named included, as it
 * was: what rendered before renders the same afterwards. */
rsrt_status rsrt_upload_environment(rsrt_context *ctx, uint32_t slot, uint32_t width, uint32_t height,
                                    const float *rgba, const rsrt_alias_entry *alias);
/* AliasTable::build_by_luminance (src/environments.rs:96-187) ON THE DEVICE, for the texels already uploaded in `slot`
 * (SURVEY.md §8 f3): the same bits as the host builder rsrt_alias_table_build (rsrt_host.h) — the sequential f32 sum and
 * the LIFO Vose pairing are kept sequential, one wave runs them (csrc/hip/rt_alias_device.h).  Replaces the slot's
 * table; host_out (may be NULL) receives the width*height entries, leftover_out (may be NULL) the count of entries
 * that kept the default {1, self, 1/N}.  rsrt_upload_environment with alias == NULL uploads the texels and calls this. */
rsrt_status rsrt_environment_build_alias(rsrt_context *ctx, uint32_t slot, rsrt_alias_entry *host_out, size_t n_entries,
                                         uint32_t *leftover_out);
/* A procedural daylight sky written straight into `slot`, ON THE DEVICE: Preetham's analytic sky with a sun disc (the model, its
 * parameters' defaults and every bit of its arithmetic are published in include/rsrt_sky.h; rsrt_sky_params is in rsrt_types.h).
 * One kernel fills the width x height texels (alpha 0, as uploaded maps have), the device builder above makes the alias table;
 * neither texels nor table cross the bus.  The texels equal rsrt_sky_fill's (rsrt_host.h) bit for bit, so the slot renders exactly
 * as if they and the host builder's table had been uploaded.  The contract is rsrt_upload_environment's: slots 0 .. 63, a filled
 * slot is replaced whatever the two sizes, every call — a refused one included — drops the temporal history first thing, the
 * accumulator is never touched, and a REFUSED call (NULL params, params rsrt_sky_params_ok refuses: a non-finite field, sun_elevation
 * outside 1 .. 90 degrees, turbidity outside 2 .. 10, a negative ground_albedo, scale, sun_illuminance or sun_radius, sun_radius >
 * 0.1, flags not 0; a zero size; more than 2^31 - 1 texels; slot > 63: all RSRT_ERR_INVALID_ARGUMENT) leaves every slot as it was.
 * Moving the sun is one more call with another sun_azimuth / sun_elevation.
 * Rust: pub fn rsrt_environment_sky(ctx: *mut RsrtContext, slot: u32, width: u32, height: u32, params: *const RsrtSkyParams) -> i32; */
rsrt_status rsrt_environment_sky(rsrt_context *ctx, uint32_t slot, uint32_t width, uint32_t height, const rsrt_sky_params *params);
/* Waits and copies the texels of `slot` to the host, width*height*4 f32, for a sky and an uploaded map alike: the colours as they
 * went in, alpha 0 (the alpha an upload carried is ignored, see above).  RSRT_ERR_NOT_READY for an empty slot,
 * RSRT_ERR_INVALID_ARGUMENT for NULL or another n_floats.
 * Rust: pub fn rsrt_environment_download(ctx: *mut RsrtContext, slot: u32, host_rgba: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_environment_download(rsrt_context *ctx, uint32_t slot, float *host_rgba, size_t n_floats);

/* build_bvh (src/bvh.rs:13-337) ON THE DEVICE (csrc/hip/rt_bvh_device.h): the arguments and outputs of the host
 * builder rsrt_build_bvh (rsrt_host.h) — host arrays in, host arrays out: primitives_out holds n_spheres + n_planes + n_triangles
 * entries, nodes_out room for twice that — and the same bits in both: level-parallel binned SAH with integer bucket counts,
 * min / max bounds, the host's f32 cost expression, and the reference's unstable two-pointer partition reproduced as its
 * closed-form permutation.  build_ms_out (may be NULL): device time of the build, uploads and downloads excluded.  A split that
 * leaves one side empty (the reference's median fallback, unreachable for finite input) is RSRT_ERR_INVALID_ARGUMENT: use the
 * host builder then. */
rsrt_status rsrt_build_bvh_device(rsrt_context *ctx, const rsrt_sphere *spheres, uint32_t n_spheres, const rsrt_plane_desc *planes, uint32_t n_planes,
                                  const rsrt_vec3 *vertices, uint32_t n_vertices, const rsrt_triangle *triangles, uint32_t n_triangles,
                                  rsrt_primitive_info *primitives_out, rsrt_bvh_node *nodes_out, uint32_t *n_nodes_out, uint32_t *depth_out,
                                  double *build_ms_out);

/* -- multi-GPU framebuffer ownership (no reference counterpart) ---------------
 * The frame is cut into tile_w x tile_h pixel tiles; this context renders tile (tx, ty) iff (tx + ty * skew) % world_size ==
 * rank — interleaved in x, each tile row shifted by `skew` (the smallest odd number >= 3 coprime to world_size: 3 for 2, 4, 8
 * GPUs) against the row above, so that a rank's tiles form a lattice whatever the frame width (t % world_size would give every
 * rank fixed column stripes whenever the tiles per row are a multiple of world_size) — and leaves every other pixel of the
 * accumulator untouched.  Default: rank 0 of 1 (whole frame).  A tile is any tile_w x tile_h whose pixel count is a multiple of 64
 * and at most 4096 (64 x 1, 1 x 64 and 128 x 32 included); it may be larger than the frame.  The partition holds from the next
 * render on, whatever the size.  A REFUSED call (rank >= world_size, an empty tile, a pixel count that is no multiple of 64 or is
 * above 4096: RSRT_ERR_INVALID_ARGUMENT) leaves the previous partition in force. */
rsrt_status rsrt_set_partition(rsrt_context *ctx, uint32_t rank, uint32_t world_size, uint32_t tile_w, uint32_t tile_h);

/* Pure host arithmetic of that partition (no GPU needed): the rank that renders pixel (x, y) (UINT32_MAX for bad
 * arguments), and a width*height byte mask (1 = rendered by `rank`; mask may be NULL) with the pixel count. */
uint32_t rsrt_partition_owner(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t world_size, uint32_t x, uint32_t y);
rsrt_status rsrt_partition_mask(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t world_size,
                                uint8_t *mask, uint64_t *owned_pixels);
/* The compact tile buffer the exchange step moves: every rank owns *n_tile_slots = tiles_y * ceil(tiles_x / world_size) tile
 * slots — the same number for all ranks — of tile_w * tile_h RGBA32F pixels each, row-major inside the tile.  tiles_xy (may be
 * NULL): 2 words per slot, the tile's (tx, ty), or UINT32_MAX twice for a padding slot (a slot beyond the right edge of the
 * frame; it holds zeros). */
rsrt_status rsrt_partition_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t world_size,
                                 uint32_t *tiles_xy, uint32_t *n_tile_slots);

/* -- multi-GPU, form 1: one process (or thread) per GPU ----------------------------------------
 * The one exchange step of the path — the sum of the ranks' W*H*4 accumulators onto a root, once per frame — runs on RCCL
 * over xGMI INSIDE the library (librccl is dlopen'ed on first use; a single-GPU caller never needs it).  Every pixel has
 * exactly one owner, so that sum is a GATHER: each rank packs its tiles into the compact buffer above (1 / world of the
 * frame), the root receives world - 1 of them point to point (grouped ncclSend / ncclRecv) and scatters them into the frame;
 * nothing is added, and the N-GPU frame equals the 1-GPU frame bit for bit.  (RSRT_COMM_MODE=reduce in the environment when the
 * context is created, or rsrt_comm_set_mode(ctx, 1): the dense ncclReduce(sum, f32) of the full accumulators instead — the
 * fallback until the gather has run on a multi-GPU box; bench.py switches to it by itself if the gathered frame is not the 1-GPU frame.)
 *   rank 0:      rsrt_comm_unique_id(&id); hand the 128 bytes to the other ranks (file, socket, MPI, a torch store ...)
 *   every rank:  rsrt_comm_init(ctx, rank, world, &id)   -- creates the communicator (collective call) and sets the tile
 *                                                            partition (rank, world, current tile size)
 *   per frame:   rsrt_accumulator_clear; rsrt_render ...; rsrt_comm_reduce(ctx, root, recv, stream)
 * rsrt_comm_reduce is asynchronous on `hip_stream` (NULL = the context's stream) and ordered after the context's
 * earlier work.  recv_device_rgba32f (root only, ignored elsewhere): where the full frame goes; NULL = in place, i.e.
 * the root's accumulator becomes the full frame (clear it before rendering further samples); a progressive caller
 * passes a separate W*H*4 f32 device buffer so that its accumulator keeps holding only its own tiles.
 * Without rsrt_comm_init the world is one rank and the reduce is a (device) copy or nothing.
 * N > 1 over RCCL is unverified on hardware so far. */
#define RSRT_UNIQUE_ID_BYTES 128
typedef struct rsrt_unique_id { char bytes[RSRT_UNIQUE_ID_BYTES]; } rsrt_unique_id;
int rsrt_comm_available(void); /* 1: librccl could be loaded (a dlopen, nothing else: safe to ask on every rank BEFORE the collective rsrt_comm_init) */
rsrt_status rsrt_comm_unique_id(rsrt_unique_id *out); /* error text: rsrt_last_error(NULL) */
rsrt_status rsrt_comm_init(rsrt_context *ctx, uint32_t rank, uint32_t world_size, const rsrt_unique_id *id);
rsrt_status rsrt_comm_reduce(rsrt_context *ctx, uint32_t root, void *recv_device_rgba32f, void *hip_stream);
rsrt_status rsrt_comm_set_mode(rsrt_context *ctx, uint32_t dense_reduce); /* 0 (default; RSRT_COMM_MODE unset): gather of compact tile buffers, 1 (RSRT_COMM_MODE=reduce):
                                                                             * dense ncclReduce(sum) of the full accumulators; every rank the same, between frames */
rsrt_status rsrt_comm_destroy(rsrt_context *ctx); /* also done by rsrt_context_destroy */

/* -- multi-GPU, form 2: one caller, a list of devices -----------------------
 * What the reference's single-threaded `State` (src/state.rs:60-98 device acquisition, :760-833 render) would bind:
 * one handle over 1/2/4/8 GPUs of the node.  Inside: one rsrt_context per device (rsrt_multi_context gives access,
 * e.g. for per-device stats), ncclCommInitAll for a list of two or more, device i renders the tiles of rank i, and the frame
 * is gathered onto devices[0] (one RCCL group per frame, into a frame buffer, so the per-device accumulators stay progressive) whenever
 * it is asked for.  Calls mirror the single-device ones; errors: rsrt_multi_last_error (NULL handle: of the last
 * failing rsrt_multi_create on this thread). */
typedef struct rsrt_multi rsrt_multi;
rsrt_status rsrt_multi_create(const int *devices, uint32_t n_devices, rsrt_multi **out);
void rsrt_multi_destroy(rsrt_multi *m);
const char *rsrt_multi_last_error(const rsrt_multi *m);
uint32_t rsrt_multi_size(const rsrt_multi *m);
rsrt_context *rsrt_multi_context(rsrt_multi *m, uint32_t i);
/* 1: the frame is gathered by RCCL; 0: by peer copies of the compact tile buffers onto devices[0] — a list of one device (no
 * exchange at all), librccl could not be loaded or its communicators did not come up, or the list names one device twice,
 * which is accepted only with RSRT_MULTI_ALLOW_SAME_DEVICE=1 (a rehearsal of N devices on one GPU). */
int rsrt_multi_uses_rccl(const rsrt_multi *m);
rsrt_status rsrt_multi_upload_scene(rsrt_multi *m,
                                    const rsrt_material *materials, uint32_t n_materials,
                                    const rsrt_sphere *spheres, uint32_t n_spheres,
                                    const rsrt_plane *planes, uint32_t n_planes,
                                    const rsrt_vec3 *vertices, uint32_t n_vertices,
                                    const rsrt_vec3 *normals, uint32_t n_normals,
                                    const rsrt_triangle *triangles, uint32_t n_triangles,
                                    const rsrt_primitive_info *primitives, uint32_t n_primitives,
                                    const rsrt_bvh_node *bvh_nodes, uint32_t n_bvh_nodes);
rsrt_status rsrt_multi_upload_environment(rsrt_multi *m, uint32_t slot, uint32_t width, uint32_t height,
                                          const float *rgba, const rsrt_alias_entry *alias);
rsrt_status rsrt_multi_resize(rsrt_multi *m, uint32_t width, uint32_t height);
rsrt_status rsrt_multi_clear(rsrt_multi *m);
rsrt_status rsrt_multi_render(rsrt_multi *m, const rsrt_camera *camera, uint32_t width, uint32_t height,
                              uint32_t sample_begin, uint32_t sample_count, uint32_t max_bounces,
                              uint32_t environment_index, uint32_t flags);
rsrt_status rsrt_multi_synchronize(rsrt_multi *m);
rsrt_status rsrt_multi_download(rsrt_multi *m, float *host_rgba, size_t n_floats);           /* reduce, then copy */
rsrt_status rsrt_multi_display_srgb8(rsrt_multi *m, uint32_t sample_total, uint8_t *host_rgba8, size_t n_bytes);
rsrt_status rsrt_multi_get_stats(rsrt_multi *m, rsrt_stats *out); /* counters summed, times = max over devices */

/* -- accumulator: cumulative_light_texture (hdr.rs:217-223) ----------------------------------
 * Library-owned W*H RGBA32F sum on the device, (re)allocated and zeroed when the resolution
 * changes (State::resize).  rsrt_accumulator_bind lets the caller own it instead (a device
 * pointer of width*height*4 floats, e.g. a torch tensor that a RCCL reduce will read); pass NULL
 * to go back to the internal one (it was given up at the bind: the context then has no accumulator
 * until the next resize or render).  Any change of the accumulator's size, to none included, drops
 * what was derived from the old one: the denoised image, the temporal history and moments, the
 * noise snapshot and estimate. */
rsrt_status rsrt_accumulator_resize(rsrt_context *ctx, uint32_t width, uint32_t height);
rsrt_status rsrt_accumulator_bind(rsrt_context *ctx, void *device_rgba32f, uint32_t width, uint32_t height);
rsrt_status rsrt_accumulator_clear(rsrt_context *ctx);
rsrt_status rsrt_accumulator_download(rsrt_context *ctx, float *host_rgba, size_t n_floats);
/* out_texture: mean = sum / sample_total rounded to binary16 (shader.wgsl:1369-1372) */
rsrt_status rsrt_resolve_mean_f16(rsrt_context *ctx, uint32_t sample_total, uint16_t *host_rgba16f, size_t n_halfs);

/* The reference's developer views — what `main` writes to out_texture instead of a render when `dev_index` (bind group 1 binding 3; key
 * bindings src/camera.rs:283) is 2 or 3, shader.wgsl:1314-1338 — for the bound accumulator's width x height, as RGBA binary16:
 *   3  the HDRI: texel (x, y) of environment `environment_index`, saturated, alpha 0 (zeros outside the map); the buffer's contents going in
 *      are ignored;
 *   2  draws of the alias table: every pixel draws 20 texel indices (seeded by its pixel index and `sample_count`, like a render's pixel) and
 *      each draw adds 0.1 / 20 to THAT texel's position in out_texture — read, add in f32, store as binary16, alpha 0.  host_rgba16f_inout holds
 *      out_texture as the previous frame left it and receives the new one.  The shader's invocations race on the texture (which draws survive
 *      is up to the GPU); this call returns the frame in which every draw lands.
 * The accumulator is not touched. */
rsrt_status rsrt_debug_view_f16(rsrt_context *ctx, uint32_t dev_index, uint32_t environment_index, uint32_t sample_count,
                                uint16_t *host_rgba16f_inout, size_t n_halfs);

/* The display pass (src/shaders/hdr.wgsl `fs_main`, src/hdr.rs:162-200): mean through binary16 ->
 * ACES fit (negatives -> magenta) -> sRGB 8-bit, as the *Srgb surface stores it.  RGBA8, alpha 255.
 * Arithmetic published in include/rsrt_tonemap.h. */
rsrt_status rsrt_display_srgb8(rsrt_context *ctx, uint32_t sample_total, uint8_t *host_rgba8, size_t n_bytes);

/* -- render: State::render's compute pass (state.rs:808-824), batched over samples -----------
 * Adds samples [sample_begin, sample_begin + sample_count) of every owned pixel into the
 * accumulator (alpha := 1), in increasing sample order per pixel, on `hip_stream`
 * (a hipStream_t, NULL = the context's own stream).  Asynchronous; rsrt_synchronize or
 * rsrt_accumulator_download/rsrt_get_stats wait for it. */
rsrt_status rsrt_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height,
                        uint32_t sample_begin, uint32_t sample_count, uint32_t max_bounces,
                        uint32_t environment_index, uint32_t flags, void *hip_stream);
rsrt_status rsrt_synchronize(rsrt_context *ctx);
rsrt_status rsrt_get_stats(rsrt_context *ctx, rsrt_stats *out);

/* -- denoiser: first-hit AOV buffers and an edge-aware a-trous filter (no reference counterpart) --
 * The reference shows a 1-16 spp image (one sample per displayed frame); these passes turn such an image into a usable picture.
 * Whole frame only: a context with a partition of world_size > 1 gets RSRT_ERR_INVALID_ARGUMENT.  Nothing here touches the
 * accumulator or what rsrt_render computes.
 *
 * AOV pass.  For every pixel and every sample k in [sample_begin, sample_begin + sample_count) it casts the camera ray that
 * rsrt_render casts for (pixel, k) — seed (pixel_index, k), unit-disc jitter — takes that ray's closest hit as rsrt_cast_rays
 * mode 0 does (BVH, then the brute-force fallback) and adds, in increasing k and in f32, to the pixel's 8-float record:
 *   [0..2] the hit material's color, [3] 1 (hits), [4..6] the hit normal (flipped towards the ray, as the shader uses it),
 *   [7] the hit distance.  A miss adds nothing, so split calls give the bits of one call.
 * The record buffer is width*height*8 f32 on the device: library-owned, sized to the accumulator (allocated and zeroed on
 * first use or when the size changes), or caller-owned through rsrt_aov_bind (16-byte aligned; NULL goes back to the
 * library's).  flags must be 0. */
rsrt_status rsrt_aov_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                            uint32_t sample_count, uint32_t flags, void *hip_stream);
rsrt_status rsrt_aov_bind(rsrt_context *ctx, void *device_f32x8, uint32_t width, uint32_t height);
rsrt_status rsrt_aov_clear(rsrt_context *ctx);
rsrt_status rsrt_aov_download(rsrt_context *ctx, float *host_f32x8, size_t n_floats);

/* Filter pass: an edge-aware a-trous wavelet filter (Dammertz et al. 2010) of the mean sum / sample_total, guided by the AOV
 * records of aov_sample_total samples.  The arithmetic is published in include/rsrt_denoise.h: demodulation by the mean
 * first-hit albedo, `iterations` levels of the 5x5 B3 spline with step 2^i and rational colour / normal / relative-depth weights,
 * remodulation.  Defaults (what a zero-initialised caller should fill in; the Python and C++ State use them):
 *   iterations 5 (0..8; 0 returns the mean exactly), sigma_color 2.0, sigma_normal 0.5, sigma_depth 0.3
 *   (each in [1e-6, 1e6]), flags RSRT_DENOISE_DEMODULATE. */
enum { RSRT_DENOISE_DEMODULATE = 1u };
typedef struct rsrt_denoise_params {
    uint32_t iterations;
    uint32_t flags;
    float sigma_color;  /* of the demodulated colour; level i uses sigma_color / 2^i (under RSRT_DENOISE_VARIANCE: sigma_l, below) */
    float sigma_normal; /* of the mean normal */
    float sigma_depth;  /* of the mean distance, relative to the centre pixel's */
} rsrt_denoise_params;
/* Writes W*H RGBA32F (alpha 1) to device_out_rgba32f (a device buffer of the accumulator's size, 16-byte aligned) or, when it is
 * NULL, to a library-owned buffer.  Scratch (two W*H float4 ping-pong buffers and the packed features) is allocated on first
 * use and freed on resize and destroy.  RSRT_ERR_NOT_READY: no accumulator or no AOV buffer; RSRT_ERR_INVALID_ARGUMENT: a bad
 * parameter, sample_total or aov_sample_total 0, an AOV buffer of another size than the accumulator, world_size > 1.
 * Asynchronous on hip_stream (NULL = the context's stream). */
rsrt_status rsrt_denoise(rsrt_context *ctx, uint32_t sample_total, uint32_t aov_sample_total, const rsrt_denoise_params *params,
                         void *device_out_rgba32f, void *hip_stream);
/* the last rsrt_denoise output (wherever it was written), to the host: W*H*4 floats */
rsrt_status rsrt_denoised_download(rsrt_context *ctx, float *host_rgba, size_t n_floats);
/* ... through the display pass: rsrt_display_pixel(denoised, 1.0f) per pixel (include/rsrt_tonemap.h), RGBA8, alpha 255 */
rsrt_status rsrt_denoised_display_srgb8(rsrt_context *ctx, uint8_t *host_rgba8, size_t n_bytes);

/* -- temporal pass: sample history kept across camera moves (no reference counterpart) ---------------------------------------------
 * An interactive caller shows one new frame of a few samples per display refresh and moves the camera between frames.  This pass
 * reprojects the previous frames' per-pixel history into the current camera, rejects it where the surface changed (plane-distance and
 * normal tests against the AOV records' mean first hit) and blends the rest with the new frame, weighted by sample count: the colour
 * of up to max_history earlier samples at no extra ray cost.  The arithmetic is published in include/rsrt_temporal.h (defaults there:
 * max_history 32, depth_tolerance 0.05, normal_tolerance 0.9).  Whole frame only, like the denoiser.
 *
 * rsrt_temporal_accumulate takes the current frame from the accumulator (sum of sample_total samples) and the AOV buffer (records of
 * aov_sample_total samples), both of the same size, seen through `camera`.  It writes W*H float4 (colour, sample weight) into a
 * library-owned history (two history and two feature buffers, 64 B a pixel, allocated on first use and freed on resize and destroy)
 * and remembers the camera for the next call.  An unchanged camera adds the new samples to each pixel's own history uncapped, so a
 * camera held still converges like the accumulator.  RSRT_ERR_NOT_READY: no accumulator or no AOV buffer; RSRT_ERR_INVALID_ARGUMENT:
 * a bad parameter, sample_total or aov_sample_total 0, an AOV buffer of another size than the accumulator, world_size > 1.
 * History is dropped (the next call acts as a first frame: out = (sum / S, S)) by rsrt_temporal_reset, by an accumulator resize or a
 * bind of another size, and by rsrt_upload_scene / rsrt_upload_environment.  The pass cannot see the render settings: a caller that
 * changes environment_index, max_bounces or the render flags calls rsrt_temporal_reset.  Each frame needs fresh sample indices
 * (a frame that reuses the previous frame's indices repeats its random numbers and adds nothing).  Asynchronous on hip_stream. */
typedef struct rsrt_temporal_params {
    uint32_t max_history;   /* cap of the reprojected history's sample weight, 1 .. 2^24 */
    float depth_tolerance;  /* plane-distance test |n . (Xq - X)| <= depth_tolerance * z, in [1e-6, 1e6] */
    float normal_tolerance; /* normal test n . nq >= normal_tolerance, in [-1, 1] */
} rsrt_temporal_params;
rsrt_status rsrt_temporal_accumulate(rsrt_context *ctx, const rsrt_camera *camera, uint32_t sample_total, uint32_t aov_sample_total,
                                     const rsrt_temporal_params *params, void *hip_stream);
rsrt_status rsrt_temporal_reset(rsrt_context *ctx);
/* the last frame's history to the host: W*H*4 floats (colour, weight); RSRT_ERR_NOT_READY when no frame ran since the last reset */
rsrt_status rsrt_temporal_download(rsrt_context *ctx, float *host_rgba, size_t n_floats);
/* rsrt_denoise_params.flags: filter the temporal pass's colour instead of sum / sample_total (sample_total is then ignored;
 * RSRT_ERR_NOT_READY when no temporal frame ran since the last reset) */
enum { RSRT_DENOISE_TEMPORAL = 2u };

/* -- variance guidance: temporal luminance moments, a variance-guided filter and a firefly clamp (no reference counterpart) ---------
 * rsrt_temporal_accumulate is rsrt_temporal_accumulate_ex with flags 0.  flags: RSRT_TEMPORAL_MOMENTS also keeps a float4 moment
 * record (mu1, mu2, frames, scale) per pixel of the luminance l of the frame's demodulated colour, reprojected and blended with the
 * colour's own taps and weights (include/rsrt_temporal.h, rsrt_tp_moments); scale (mu2 - mu1^2) estimates the variance of the output's
 * luminance.  The history and features such a frame writes are those of a plain frame, bit for bit.  Two more library-owned buffers
 * (32 B a pixel) are allocated on the first MOMENTS frame and freed with the history.  A frame whose MOMENTS flag differs from the
 * previous frame's drops the history (it acts as a first frame).  Unknown flags: RSRT_ERR_INVALID_ARGUMENT. */
enum { RSRT_TEMPORAL_MOMENTS = 1u };
rsrt_status rsrt_temporal_accumulate_ex(rsrt_context *ctx, const rsrt_camera *camera, uint32_t sample_total, uint32_t aov_sample_total,
                                        const rsrt_temporal_params *params, uint32_t flags, void *hip_stream);
/* the last frame's moment records to the host: W*H*4 floats (mu1, mu2, frames, scale); RSRT_ERR_NOT_READY when the last frame since
 * the last reset carried none */
rsrt_status rsrt_temporal_moments_download(rsrt_context *ctx, float *host_f32x4, size_t n_floats);
/* rsrt_denoise_params.flags (include/rsrt_variance.h; both act only when iterations >= 1, iterations 0 still returns the mean):
 *   RSRT_DENOISE_CLAMP     firefly clamp of the filter's input: a pixel whose luminance exceeds that of all 8 neighbours (and 0) is
 *                          scaled down to the brightest neighbour's.
 *   RSRT_DENOISE_VARIANCE  variance-guided levels (SVGF): the colour term compares luminance against sigma_color^2 times the 3x3 blur
 *                          of a per-pixel variance, which every level filters along with the colour.  sigma_color is then sigma_l,
 *                          of luminance in units of its standard deviation: default RSRT_SV_SIGMA_L 4.0 (no 2^i per level).  The
 *                          variance comes from the temporal moments under RSRT_DENOISE_TEMPORAL (the last temporal frame must have
 *                          carried them, otherwise RSRT_ERR_NOT_READY), or from the input's luminance itself; below 4 frames of
 *                          history it is estimated over a 7x7 window.  Requires RSRT_DENOISE_DEMODULATE (RSRT_ERR_INVALID_ARGUMENT). */
enum { RSRT_DENOISE_VARIANCE = 4u, RSRT_DENOISE_CLAMP = 8u };

/* -- guided upsampling: trace at a low size, rebuild the detail from first-hit records of the output size (no reference counterpart) --
 * A path sample costs several times what a first hit costs, and the demodulated colour (colour / first-hit albedo) is smooth: the
 * edges and the albedo's detail live in the first-hit records.  So an interactive caller renders the accumulator and its AOV buffer
 * at a LOW size w x h (of the output's aspect: ceil(W / 2) x ceil(H / 2) for half size), the first hits alone at the output size
 * W x H (the guide), and rsrt_upsample rebuilds the W x H picture: a joint-bilateral upsample of the low frame's demodulated colour,
 * nine taps weighted by a tent and by the denoiser's normal and relative-depth terms against the guide, multiplied by the guide's
 * albedo.  The arithmetic is published in include/rsrt_upsample.h.  Whole frame only, like the denoiser.
 *
 * The guide: width*height*8 f32 records exactly like the AOV buffer's, of a size of its own, W >= w, H >= h, both at most 16384.
 * Library-owned (allocated and zeroed by rsrt_guide_render on first use or when the size it is given changes; freed on destroy) or
 * caller-owned through rsrt_guide_bind (16-byte aligned; NULL goes back to the library's).  rsrt_guide_render adds the first hits of
 * samples [sample_begin, sample_begin + sample_count) as rsrt_aov_render does, for a frame of width x height; it needs no accumulator
 * and touches neither the accumulator nor the AOV buffer.  flags must be 0.  Give the guide as many samples as the low frame: its
 * edges then alias as the render's own pixel filter does (a 1-sample guide under a 4-sample frame measured worse than bilinear on
 * suzanne). */
rsrt_status rsrt_guide_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                              uint32_t sample_count, uint32_t flags, void *hip_stream);
rsrt_status rsrt_guide_bind(rsrt_context *ctx, void *device_f32x8, uint32_t width, uint32_t height);
rsrt_status rsrt_guide_clear(rsrt_context *ctx);
rsrt_status rsrt_guide_download(rsrt_context *ctx, float *host_f32x8, size_t n_floats);

/* rsrt_upsample_params.flags: DEMODULATE as the denoiser's; the low colour is the accumulator's sum / sample_total (default), the last
 * rsrt_denoise output (DENOISED) or the last temporal frame's colour (TEMPORAL); under either, sample_total is ignored.
 * Defaults: flags RSRT_UPSAMPLE_DEMODULATE, sigma_normal 0.5, sigma_depth 0.3 (each in [1e-6, 1e6]). */
enum { RSRT_UPSAMPLE_DEMODULATE = 1u, RSRT_UPSAMPLE_DENOISED = 2u, RSRT_UPSAMPLE_TEMPORAL = 4u };
typedef struct rsrt_upsample_params {
    uint32_t flags;
    float sigma_normal; /* of the mean normal, low tap against guide */
    float sigma_depth;  /* of the mean distance, relative to the guide pixel's */
} rsrt_upsample_params;
/* Writes W*H RGBA32F (alpha 1), W x H the guide's size, to device_out_rgba32f (16-byte aligned) or, when it is NULL, to a
 * library-owned buffer.  The AOV records hold aov_sample_total samples, the guide's guide_sample_total.  Writes nothing but its own
 * scratch (24 B a low pixel) and the output: the accumulator, the AOV buffer, the guide, the denoised image and the temporal history
 * keep their bits.  RSRT_ERR_NOT_READY: no accumulator, AOV buffer or guide, no denoised image under DENOISED, no temporal frame since
 * the last reset under TEMPORAL.  RSRT_ERR_INVALID_ARGUMENT: NULL params, unknown flags, DENOISED and TEMPORAL together, a sigma out
 * of range, a total of 0, an AOV buffer of another size than the accumulator, a guide smaller than the accumulator in either
 * dimension or above 16384, world_size > 1, a misaligned output pointer.  Nothing is launched on a refused call.  Asynchronous on
 * hip_stream (NULL = the context's stream). */
rsrt_status rsrt_upsample(rsrt_context *ctx, uint32_t sample_total, uint32_t aov_sample_total, uint32_t guide_sample_total,
                          const rsrt_upsample_params *params, void *device_out_rgba32f, void *hip_stream);
/* the last rsrt_upsample output (wherever it was written), to the host: W*H*4 floats */
rsrt_status rsrt_upsampled_download(rsrt_context *ctx, float *host_rgba, size_t n_floats);
/* ... through the display pass: rsrt_display_pixel(upsampled, 1.0f) per pixel (include/rsrt_tonemap.h), RGBA8, alpha 255 */
rsrt_status rsrt_upsampled_display_srgb8(rsrt_context *ctx, uint8_t *host_rgba8, size_t n_bytes);

/* -- noise estimate: how noisy is the picture in the accumulator still, and where (no reference counterpart) ------------------
 * The accumulator sums a pixel's samples in increasing order, so a copy of it taken at n1 samples and the accumulator at n2 > n1
 * hold two estimates of every pixel, the first n1 samples and all n2 (the half buffer of Dammertz et al., "A Hierarchical Automatic
 * Stopping Condition for Monte Carlo Global Illumination", 2010): one device copy, no extra ray.  Per pixel the estimate is the
 * summed absolute difference of the two means over the square root of the mean's rgb sum; per tile the mean over the tile's pixels
 * inside the frame; the arithmetic is published in include/rsrt_noise.h.  With n1 = n2 / 2 it estimates the error of the mean of all
 * n2 samples.  Whole frame only, like the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.  Nothing here
 * writes the accumulator, the AOV buffer, the guide or any history.
 *
 * The snapshot and the last estimate are dropped by rsrt_noise_reset, rsrt_accumulator_clear (a cleared accumulator makes the pair
 * meaningless), rsrt_accumulator_resize to another size and rsrt_accumulator_bind of another size; a bind of the same size keeps them.
 * rsrt_noise_params defaults: tile_w 16, tile_h 16, threshold 0, flags 0. */
typedef struct rsrt_noise_params {
    uint32_t tile_w, tile_h; /* tile_w * tile_h a multiple of 64, at most 4096 (the partition's rule); a tile may exceed the frame */
    float threshold;         /* what rsrt_noise_summary.tiles_above counts against: >= 0, +inf allowed */
    uint32_t flags;          /* 0 */
} rsrt_noise_params;
typedef struct rsrt_noise_summary {
    float max_error, mean_error; /* over the tile map in row-major order; the mean is a sequential f32 sum / tile count */
    uint32_t tiles_x, tiles_y;   /* ceil(width / tile_w), ceil(height / tile_h) */
    uint32_t tiles_above;        /* tiles with error > threshold; an infinite error (a pixel with inf or NaN radiance) always counts */
    uint32_t _pad;
} rsrt_noise_summary;
/* Copies the accumulator, the sum of sample_total >= 1 samples, into a library-owned buffer of its size (device to device, ordered
 * after everything enqueued so far; asynchronous on hip_stream, NULL = the context's stream).  RSRT_ERR_NOT_READY without an
 * accumulator; RSRT_ERR_INVALID_ARGUMENT for sample_total 0. */
rsrt_status rsrt_noise_snapshot(rsrt_context *ctx, uint32_t sample_total, void *hip_stream);
/* The tile map of the accumulator, now the sum of sample_total samples, against the snapshot: tiles_x * tiles_y floats in a
 * library-owned buffer.  Asynchronous.  RSRT_ERR_NOT_READY without an accumulator or a snapshot of it; RSRT_ERR_INVALID_ARGUMENT for
 * NULL params, non-zero flags, a bad tile, a negative or NaN threshold, sample_total not above the snapshot's.  Nothing is launched
 * on a refused call, and the last estimate stays what it was. */
rsrt_status rsrt_noise_estimate(rsrt_context *ctx, uint32_t sample_total, const rsrt_noise_params *params, void *hip_stream);
/* Waits, copies the last estimate's tiles_x * tiles_y floats (row-major) to host_tiles and fills *out.  host_tiles may be NULL for
 * the summary alone (n_floats is then ignored), out may be NULL for the tiles alone.  RSRT_ERR_NOT_READY without an estimate since
 * the last reset; RSRT_ERR_INVALID_ARGUMENT for another n_floats. */
rsrt_status rsrt_noise_download(rsrt_context *ctx, float *host_tiles, size_t n_floats, rsrt_noise_summary *out);
rsrt_status rsrt_noise_reset(rsrt_context *ctx);

/* -- auto-exposure: a luminance histogram meter and an exposed display (no reference counterpart) -----------------------------
 * Every other display call shows the picture at an exposure of 1, so whether it is usable depends on the scale of the environment
 * the caller uploaded.  rsrt_exposure_meter builds, on the device and in integers, a 256-bin histogram of the log-luminance of one
 * of the four images the library can hold (eight bins an octave, 2^-16 .. 2^16; word 256 counts the pixels with no positive
 * luminance); rsrt_exposure_download turns it into an exposure — the log-average ("key") meter of Reinhard et al. 2002 over the
 * ranks [low_permille, high_permille) of the metered pixels; rsrt_display_exposed_srgb8 is the display pass with the exposure
 * multiplied in after the binary16 rounding of the mean.  The arithmetic is published in include/rsrt_exposure.h; the histogram
 * is independent of the order pixels are counted in, so it and the exposure are bitwise reproducible.
 *
 * The library keeps NO exposure: adaptation over time goes through previous_exposure and blend (the State classes remember the
 * last value).  The histogram stays valid until the next rsrt_exposure_meter, rsrt_exposure_reset or rsrt_context_destroy.  Whole
 * frame only, like the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.  Nothing here writes the
 * accumulator, the AOV buffer, the guide, any history, the denoised image or the upsampled image.  A refused call launches nothing
 * and leaves the last histogram as it was.
 * rsrt_exposure_params defaults: low_permille 100, high_permille 950, key 0.18, min_exposure 2^-16, max_exposure 2^16, blend 1,
 * previous_exposure 0, flags 0. */
enum {
    RSRT_EXPOSURE_MEAN = 0,      /* the accumulator, sum / sample_total */
    RSRT_EXPOSURE_DENOISED = 1,  /* the last rsrt_denoise output */
    RSRT_EXPOSURE_TEMPORAL = 2,  /* the colour of the last temporal frame's history */
    RSRT_EXPOSURE_UPSAMPLED = 3  /* the last rsrt_upsample output, of the guide's size */
};
typedef struct rsrt_exposure_params {
    uint32_t low_permille, high_permille; /* the ranks metered, in thousandths of the metered pixels: low < high <= 1000 */
    float key;                            /* what the average luminance is exposed to: finite, > 0 */
    float min_exposure, max_exposure;     /* the clamp of the target: finite, > 0, min <= max */
    float blend;                          /* in [0, 1]: how far the exposure moves from previous_exposure towards the target */
    float previous_exposure;              /* 0: none, the exposure is the target; otherwise finite and > 0 */
    uint32_t flags;                       /* 0 */
} rsrt_exposure_params;
typedef struct rsrt_exposure_result {
    float exposure, target;    /* what to display with; the clamped key / average_luminance */
    float average_luminance;   /* the meter's reading (0: nothing metered) */
    uint32_t metered, skipped; /* pixels in the 256 bins; pixels with !(luminance > 0) */
    uint32_t _pad;
} rsrt_exposure_result;
/* Builds the histogram of `source` in a library-owned buffer (zeroed and filled by the enqueued work; asynchronous on hip_stream,
 * NULL = the context's stream, ordered after everything enqueued so far).  sample_total is ignored for all sources but
 * RSRT_EXPOSURE_MEAN.  RSRT_ERR_NOT_READY when the source image does not exist (no accumulator, no denoised or upsampled image, no
 * temporal frame since the last reset); RSRT_ERR_INVALID_ARGUMENT for an unknown source, sample_total 0 under RSRT_EXPOSURE_MEAN. */
rsrt_status rsrt_exposure_meter(rsrt_context *ctx, uint32_t source, uint32_t sample_total, void *hip_stream);
/* Waits, copies the last histogram's 257 words to host_hist and fills *out from it (rsrt_exposure_from_histogram, on the host).
 * host_hist may be NULL (n_words is then ignored), out may be NULL.  RSRT_ERR_NOT_READY without a histogram since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for NULL params, params rsrt_exposure_params_ok refuses, non-zero flags, n_words != 257 with a
 * non-NULL host_hist. */
rsrt_status rsrt_exposure_download(rsrt_context *ctx, const rsrt_exposure_params *params, uint32_t *host_hist, size_t n_words,
                                   rsrt_exposure_result *out);
rsrt_status rsrt_exposure_reset(rsrt_context *ctx); /* drops the histogram */
/* `source` through the exposed display pass: rsrt_display_pixel_exposed per pixel (include/rsrt_exposure.h), RGBA8, alpha 255; with
 * exposure 1 the bytes of rsrt_display_srgb8 / rsrt_denoised_display_srgb8 / rsrt_upsampled_display_srgb8.  Errors as for
 * rsrt_exposure_meter, and RSRT_ERR_INVALID_ARGUMENT for an exposure that is not finite and > 0 or another n_bytes than 4 a pixel. */
rsrt_status rsrt_display_exposed_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, uint8_t *host_rgba8,
                                       size_t n_bytes);

/* -- bloom: a bright-pass mip pyramid and a bloomed display (no reference counterpart) -----------------------------------------
 * The exposed display clips everything brighter than display white to the same white, so the sun and the glints on metal are dots.
 * rsrt_bloom builds, between the meter and the tone map, the thresholded mip-pyramid bloom of Jimenez 2014 (with the firefly
 * weighting of Karis 2013 on the first downsample) of one of the four images the library can hold: a prefilter (exposure, clamp,
 * threshold), `levels` 13-tap downsamples, a tent and a doubling on the way back up.  The bloom image B is half the source's size,
 * ceil(w / 2) x ceil(h / 2); rsrt_display_bloomed_srgb8 is the exposed display pass with intensity * up(B) added before the tone map.
 * The arithmetic is published in include/rsrt_bloom.h and is bitwise reproducible.
 *
 * The library keeps NO exposure: the caller passes the same exposure to rsrt_bloom and to rsrt_display_bloomed_srgb8 (the State
 * classes do).  B and the size of the source it was built for stay valid until the next rsrt_bloom, rsrt_bloom_reset, a change of the
 * accumulator's size (rsrt_accumulator_resize, a bind of another size or of NULL) or rsrt_context_destroy.  Whole frame only, like
 * the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.  Nothing here writes the accumulator, the AOV
 * buffer, the guide, any history, the denoised or upsampled image or the exposure histogram.  A refused call launches nothing and
 * leaves the last bloom image as it was.
 * rsrt_bloom_params defaults: levels 6, flags RSRT_BLOOM_KARIS, threshold 1.0 (in exposed units: what is brighter than display
 * white blooms); the default intensity is 0.1 (RSRT_BLOOM_* in include/rsrt_bloom.h). */
enum { RSRT_BLOOM_KARIS = 1u }; /* the first downsample weighs its five groups by 1 / (1 + luminance) */
typedef struct rsrt_bloom_params {
    uint32_t levels;  /* 1 .. 8 (RSRT_BLOOM_MAX_LEVELS); a level may be 1 x 1 */
    uint32_t flags;   /* RSRT_BLOOM_KARIS or 0 */
    float threshold;  /* finite, >= 0, in exposed units */
    float _pad;
} rsrt_bloom_params;
/* Builds B of `source` (RSRT_EXPOSURE_*) in a library-owned pyramid (about 11 bytes a source pixel); asynchronous on hip_stream,
 * NULL = the context's stream, ordered after everything enqueued so far.  sample_total is ignored for all sources but
 * RSRT_EXPOSURE_MEAN.  RSRT_ERR_NOT_READY when the source image does not exist; RSRT_ERR_INVALID_ARGUMENT for an unknown source,
 * sample_total 0 under RSRT_EXPOSURE_MEAN, an exposure that is not finite and > 0, NULL params or params rsrt_bloom_params_ok refuses
 * (levels, unknown flags, threshold).
 * Rust: pub fn rsrt_bloom(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32, params: *const RsrtBloomParams,
 *                         hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_bloom(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_bloom_params *params,
                       void *hip_stream);
/* Waits and copies B to host_rgba as RGBA32F, alpha 1; *width and *height (either may be NULL) receive its size, which is all a
 * call with host_rgba NULL and n_floats 0 asks for.  RSRT_ERR_NOT_READY without a bloom image since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for another n_floats than 4 a texel.
 * Rust: pub fn rsrt_bloom_download(ctx: *mut RsrtContext, host_rgba: *mut f32, n_floats: usize, width: *mut u32, height: *mut u32) -> i32; */
rsrt_status rsrt_bloom_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height);
/* Rust: pub fn rsrt_bloom_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_bloom_reset(rsrt_context *ctx); /* drops the bloom image */
/* `source` through the bloomed display pass: rsrt_display_pixel_bloomed per pixel (include/rsrt_bloom.h), RGBA8, alpha 255; with
 * intensity 0 the bytes of rsrt_display_exposed_srgb8.  Errors as for rsrt_exposure_meter, RSRT_ERR_NOT_READY without a bloom image
 * since the last reset, and RSRT_ERR_INVALID_ARGUMENT for an exposure that is not finite and > 0, an intensity that is not finite and
 * >= 0, a bloom image built for another size than `source` has, or another n_bytes than 4 a pixel.
 * Rust: pub fn rsrt_display_bloomed_srgb8(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32, intensity: f32,
 *                                         host_rgba8: *mut u8, n_bytes: usize) -> i32; */
rsrt_status rsrt_display_bloomed_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, float intensity,
                                       uint8_t *host_rgba8, size_t n_bytes);

/* -- local exposure: a bilateral-grid base layer and a graded display (no reference counterpart) ---------------------------------
 * The meter gives a frame ONE exposure: inside the house the walls are right and the sky through the openings clips, or the sky is
 * right and the room is black.  rsrt_local_exposure builds, between the meter and the tone map, the bilateral grid (Chen, Paris,
 * Durand 2007) of the log-luminance of one of the four images the library can hold: gx x gy x 32 cells of `cell` x `cell` pixels and
 * one octave, each a count and a sum, blurred with a 1-2-1 tent along every axis.  rsrt_display_local_srgb8 is the exposed (or
 * bloomed) display pass with a per-pixel gain before the tone map: the grid sliced at the pixel's position and log-luminance is the
 * base layer (Durand, Dorsey 2002), and the gain moves the base towards key / exposure by `shadows` (below it) or `highlights` (above
 * it) of the distance in octaves, at most max_stops.  The detail passes through.  The arithmetic is published in
 * include/rsrt_local.h and is bitwise reproducible.
 *
 * The grid is of the UNEXPOSED image: the library keeps NO exposure and no strengths, they enter at the display alone, and a change
 * of either needs no rebuild.  The grid and the size of the source it was built for stay valid until the next rsrt_local_exposure,
 * rsrt_local_exposure_reset, a change of the accumulator's size (rsrt_accumulator_resize, a bind of another size or of NULL) or
 * rsrt_context_destroy.  Whole frame only, like the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.
 * Nothing here writes the accumulator, the AOV buffer, the guide, any history, the denoised or upsampled image, the exposure
 * histogram or the bloom image.  A refused call launches nothing and leaves the last grid as it was.
 * rsrt_local_params defaults: shadows 0.5, highlights 0.5, key 0.18, max_stops 4; the default cell is 32 (RSRT_LOCAL_* in
 * include/rsrt_local.h). */
typedef struct rsrt_local_params {
    float shadows;    /* 0 .. 1: how far a base below key / exposure is lifted towards it */
    float highlights; /* 0 .. 1: how far a base above it is lowered */
    float key;        /* finite, > 0: the luminance the exposure is taken to put at mid-grey (the meter's key) */
    float max_stops;  /* 0 .. 16: the most octaves a gain moves a pixel, either way */
    uint32_t flags;   /* 0 */
    uint32_t _pad;
} rsrt_local_params;
/* Builds the blurred grid of `source` (RSRT_EXPOSURE_*) in library-owned memory (2 x 256 bytes a grid column: 0.5 MB at 1920 x 1080
 * and cell 32); asynchronous on hip_stream, NULL = the context's stream, ordered after everything enqueued so far.  sample_total is
 * ignored for all sources but RSRT_EXPOSURE_MEAN.  RSRT_ERR_NOT_READY when the source image does not exist;
 * RSRT_ERR_INVALID_ARGUMENT for an unknown source, sample_total 0 under RSRT_EXPOSURE_MEAN or a cell other than 8, 16, 32, 64.
 * Rust: pub fn rsrt_local_exposure(ctx: *mut RsrtContext, source: u32, sample_total: u32, cell: u32, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_local_exposure(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t cell, void *hip_stream);
/* Waits and copies the BLURRED grid to host_words: z-major, then y, then x, two words a cell (count, sum of q); dims_out (may be
 * NULL) receives gx, gy, gz, cell, which is all a call with host_words NULL and n_words 0 asks for.  RSRT_ERR_NOT_READY without a
 * grid since the last reset; RSRT_ERR_INVALID_ARGUMENT for another n_words than 2 * gx * gy * gz.
 * Rust: pub fn rsrt_local_exposure_download(ctx: *mut RsrtContext, host_words: *mut u32, n_words: usize, dims_out: *mut u32) -> i32; */
rsrt_status rsrt_local_exposure_download(rsrt_context *ctx, uint32_t *host_words, size_t n_words, uint32_t dims_out[4]);
/* Rust: pub fn rsrt_local_exposure_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_local_exposure_reset(rsrt_context *ctx); /* drops the grid */
/* The gain of every pixel of `source` at `exposure` under `params`, W x H f32 (1 for a skipped pixel): what
 * rsrt_display_local_srgb8 multiplies by, so that the slice can be held bit for bit.  Errors as for rsrt_display_local_srgb8, with
 * n_floats one a pixel.
 * Rust: pub fn rsrt_local_gain_download(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                       params: *const RsrtLocalParams, host_gain: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_local_gain_download(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params,
                                     float *host_gain, size_t n_floats);
/* `source` through the graded display pass: rsrt_display_pixel_local per pixel (include/rsrt_local.h), RGBA8, alpha 255.  With
 * bloom_intensity 0 no bloom image is needed; with bloom_intensity > 0 the rules are rsrt_display_bloomed_srgb8's.  With shadows and
 * highlights 0 the bytes are rsrt_display_exposed_srgb8's or rsrt_display_bloomed_srgb8's.  Errors as for rsrt_exposure_meter,
 * RSRT_ERR_NOT_READY without a grid (or, with bloom_intensity > 0, a bloom image) since the last reset, and
 * RSRT_ERR_INVALID_ARGUMENT for an exposure that is not finite and > 0, NULL params or params rsrt_local_params_ok refuses, a
 * bloom_intensity that is not finite and >= 0, a grid or a bloom image built for another size than `source` has, or another n_bytes
 * than 4 a pixel.
 * Rust: pub fn rsrt_display_local_srgb8(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                       params: *const RsrtLocalParams, bloom_intensity: f32, host_rgba8: *mut u8, n_bytes: usize) -> i32; */
rsrt_status rsrt_display_local_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *params,
                                     float bloom_intensity, uint8_t *host_rgba8, size_t n_bytes);

/* -- depth of field: a circle-of-confusion pass and a lens-blur image (no reference counterpart) ---------------------------------
 * The integrator traces the reference's pinhole camera, so everything is equally sharp at every distance.  rsrt_dof blurs one of the
 * four images the library can hold as a thin lens focused on a plane would: per pixel a signed blur radius (the circle of confusion)
 * from the first-hit distance in the pixel's AOV or guide record — negative in front of the focus plane, positive behind it, `aperture`
 * times the picture's height for a point at infinity, at most max_radius pixels — and a disc gather over (2 max_radius + 1)^2 taps
 * in which a tap behind the pixel spreads no wider than the pixel's own disc (the scatter-as-gather occlusion rule).  It is a blur
 * of LINEAR, UNEXPOSED radiance: it runs after rsrt_denoise / rsrt_temporal_accumulate / rsrt_upsample and before the meter, bloom
 * and local exposure, which take its output, the lens image, as their source RSRT_EXPOSURE_LENS.  The lens image has the size of the
 * source it was built from.  The arithmetic is published in include/rsrt_dof.h and is bitwise reproducible.  With aperture 0, or
 * everything on the focus plane, the lens image is the source's colour bit for bit.
 *
 * Sources RSRT_EXPOSURE_MEAN, _DENOISED and _TEMPORAL read the AOV buffer, which must have the accumulator's size;
 * RSRT_EXPOSURE_UPSAMPLED reads the guide, which must have the upsampled image's size.  The lens image and its size stay valid until
 * the next rsrt_dof, rsrt_dof_reset, a change of the accumulator's size (rsrt_accumulator_resize, a bind of another size or of NULL)
 * or rsrt_context_destroy.  Whole frame only, like the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.
 * Nothing here writes the accumulator, the AOV buffer, the guide, any history, the denoised or upsampled image, the exposure
 * histogram, the bloom image or the local-exposure grid.  A refused call launches nothing and leaves the last lens image as it was.
 * rsrt_dof_params defaults: focus_distance 1, aperture 0.01, max_radius 8, flags 0 (RSRT_DOF_* in include/rsrt_dof.h). */
enum { RSRT_EXPOSURE_LENS = 4 }; /* the last rsrt_dof output: a source of the meter, bloom, local exposure and their displays */
typedef struct rsrt_dof_params {
    float focus_distance; /* finite, > 0: the depth along the optical axis that is sharp, in scene units */
    float aperture;       /* finite, >= 0: the blur radius of a point at infinity as a fraction of the picture's height */
    uint32_t max_radius;  /* 1 .. 16 (RSRT_DOF_MAX_RADIUS): the largest blur radius, in pixels */
    uint32_t flags;       /* 0 */
} rsrt_dof_params;
/* Builds the lens image of `source` (RSRT_EXPOSURE_MEAN .. _UPSAMPLED, or RSRT_EXPOSURE_FOG, which is blurred with the records of the
 * image it was built from) seen through `camera` (the one the source and its records
 * were rendered with) into device_out_rgba32f (device memory, W x H x 4 f32, 16-byte aligned, alpha 1) or, when that is NULL, into
 * library-owned memory; 32 bytes of library-owned scratch a pixel either way.  Asynchronous on hip_stream, NULL = the context's
 * stream, ordered after everything enqueued so far.  sample_total is ignored for all sources but RSRT_EXPOSURE_MEAN.
 * RSRT_ERR_NOT_READY when the source image or its records do not exist; RSRT_ERR_INVALID_ARGUMENT for NULL camera or params, params
 * rsrt_dof_params_ok refuses (focus_distance not finite and > 0, aperture not finite and >= 0, max_radius outside 1 .. 16, flags not
 * 0), RSRT_EXPOSURE_LENS or an unknown source, sample_total 0 under RSRT_EXPOSURE_MEAN, records of another size than the source, a
 * misaligned output pointer.
 * Rust: pub fn rsrt_dof(ctx: *mut RsrtContext, source: u32, sample_total: u32, camera: *const RsrtCamera, params: *const RsrtDofParams,
 *                       device_out_rgba32f: *mut c_void, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_dof(rsrt_context *ctx, uint32_t source, uint32_t sample_total, const rsrt_camera *camera, const rsrt_dof_params *params,
                     void *device_out_rgba32f, void *hip_stream);
/* Waits and copies the lens image to host_rgba as RGBA32F, alpha 1; *width and *height (either may be NULL) receive its size, which
 * is all a call with host_rgba NULL and n_floats 0 asks for.  RSRT_ERR_NOT_READY without a lens image since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for another n_floats than 4 a pixel.
 * Rust: pub fn rsrt_dof_download(ctx: *mut RsrtContext, host_rgba: *mut f32, n_floats: usize, width: *mut u32, height: *mut u32) -> i32; */
rsrt_status rsrt_dof_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height);
/* Waits and copies the signed blur radii of the last rsrt_dof, one f32 a pixel, so that the circle-of-confusion step can be held bit
 * for bit.  Errors as for rsrt_dof_download, with n_floats one a pixel.
 * Rust: pub fn rsrt_dof_coc_download(ctx: *mut RsrtContext, host_r: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_dof_coc_download(rsrt_context *ctx, float *host_r, size_t n_floats);
/* Autofocus: the depth along the optical axis at pixel (x, y) of `source`'s records (rsrt_dof_depth, include/rsrt_dof.h), +inf on sky.
 * Waits and copies one record; needs no image and no lens image.  RSRT_ERR_NOT_READY without the records; RSRT_ERR_INVALID_ARGUMENT
 * for NULL camera or z_out, RSRT_EXPOSURE_LENS or an unknown source, records of another size than the accumulator (sources 0 .. 2),
 * x or y outside the records.
 * Rust: pub fn rsrt_dof_depth_at(ctx: *mut RsrtContext, source: u32, camera: *const RsrtCamera, x: u32, y: u32, z_out: *mut f32) -> i32; */
rsrt_status rsrt_dof_depth_at(rsrt_context *ctx, uint32_t source, const rsrt_camera *camera, uint32_t x, uint32_t y, float *z_out);
/* Rust: pub fn rsrt_dof_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_dof_reset(rsrt_context *ctx); /* drops the lens image */

/* -- camera motion blur: a velocity pass, tile maxima, a line gather (no reference counterpart) -----------------------------------
 * The integrator exposes every frame for an instant, so a camera that moves strobes from frame to frame.  The scene is static: the
 * camera's motion is all the motion there is, and rsrt_motion_blur blurs one of the five images the library can hold along it.  Per
 * pixel a velocity u from the first-hit distance in the pixel's AOV or guide record, the camera the source was rendered with and the
 * camera one frame earlier (while the shutter is open the pixel's image travels from p - u to p + u, |u| at most max_radius pixels);
 * per 16 x 16 tile the velocity of greatest length, and the greatest of those over the 3 x 3 tiles around each tile; then `taps` taps
 * along that neighbourhood velocity, each weighed by whether it or the pixel can reach the other and which of them is in front.  A
 * tile whose neighbourhood moves by less than half a pixel is copied.  It is a blur of LINEAR, UNEXPOSED radiance: it runs after
 * rsrt_dof and before the meter, bloom, local exposure, the white meter and their displays, which take its output, the motion image,
 * as their source RSRT_EXPOSURE_MOTION.  The motion image has the size of the source it was built from.  The arithmetic is published
 * in include/rsrt_motion.h and is bitwise reproducible.  With `previous` equal to `camera`, or shutter 0, the motion image is the
 * source's colour bit for bit.  The library keeps no camera and no shutter state.
 *
 * Sources RSRT_EXPOSURE_MEAN, _DENOISED and _TEMPORAL read the AOV buffer, which must have the accumulator's size;
 * RSRT_EXPOSURE_UPSAMPLED reads the guide, which must have the upsampled image's size; RSRT_EXPOSURE_LENS reads the records the lens
 * image was built from.  The motion image and its size stay valid until the next rsrt_motion_blur, rsrt_motion_reset, a change of the
 * accumulator's size or rsrt_context_destroy.  Whole frame only.  Nothing here writes any other image or buffer of the context.  A
 * refused call launches nothing and leaves the last motion image as it was.
 * rsrt_motion_params defaults: shutter 0.5, max_radius 16, taps 16, flags 0 (RSRT_MOTION_* in include/rsrt_motion.h). */
enum { RSRT_EXPOSURE_MOTION = 5 }; /* the last rsrt_motion_blur output: a source of the meters, bloom, local exposure and the displays */
typedef struct rsrt_motion_params {
    float shutter;       /* finite, in [0, 1]: the fraction of the frame interval the shutter is open (0.5: a 180 degree shutter) */
    uint32_t max_radius; /* 1 .. 16 (RSRT_MOTION_MAX_RADIUS): the largest blur half-length, in pixels */
    uint32_t taps;       /* even, 2 .. 32: taps along the line */
    uint32_t flags;      /* 0 */
} rsrt_motion_params;
/* Builds the motion image of `source` (RSRT_EXPOSURE_MEAN .. _LENS, or RSRT_EXPOSURE_FOG, which is blurred with the records of the
 * image it was built from) seen through `camera` (the one the source and its records were
 * rendered with) after `previous` (the camera one frame earlier) into device_out_rgba32f (device memory, W x H x 4 f32, 16-byte
 * aligned, alpha 1) or, when that is NULL, into library-owned memory; 44 bytes of library-owned scratch a pixel either way.
 * Asynchronous on hip_stream, NULL = the context's stream, ordered after everything enqueued so far.  sample_total is ignored for
 * all sources but RSRT_EXPOSURE_MEAN.  RSRT_ERR_NOT_READY when the source image or its records do not exist;
 * RSRT_ERR_INVALID_ARGUMENT for NULL camera, previous or params, params rsrt_motion_params_ok refuses, RSRT_EXPOSURE_MOTION or an
 * unknown source, sample_total 0 under RSRT_EXPOSURE_MEAN, records of another size than the source, a misaligned output pointer.
 * Rust: pub fn rsrt_motion_blur(ctx: *mut RsrtContext, source: u32, sample_total: u32, camera: *const RsrtCamera, previous: *const RsrtCamera,
 *                               params: *const RsrtMotionParams, device_out_rgba32f: *mut c_void, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_motion_blur(rsrt_context *ctx, uint32_t source, uint32_t sample_total, const rsrt_camera *camera, const rsrt_camera *previous,
                             const rsrt_motion_params *params, void *device_out_rgba32f, void *hip_stream);
/* Waits and copies the motion image to host_rgba as RGBA32F, alpha 1; *width and *height (either may be NULL) receive its size, which
 * is all a call with host_rgba NULL and n_floats 0 asks for.  RSRT_ERR_NOT_READY without a motion image since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for another n_floats than 4 a pixel.
 * Rust: pub fn rsrt_motion_download(ctx: *mut RsrtContext, host_rgba: *mut f32, n_floats: usize, width: *mut u32, height: *mut u32) -> i32; */
rsrt_status rsrt_motion_download(rsrt_context *ctx, float *host_rgba, size_t n_floats, uint32_t *width, uint32_t *height);
/* Waits and copies the velocities of the last rsrt_motion_blur, 3 f32 a pixel (ux, uy, l), so that the velocity step can be held bit
 * for bit.  Errors as for rsrt_motion_download, with n_floats three a pixel.
 * Rust: pub fn rsrt_motion_velocity_download(ctx: *mut RsrtContext, host_uvl: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_motion_velocity_download(rsrt_context *ctx, float *host_uvl, size_t n_floats);
/* Waits and copies every tile's own maximum of the last rsrt_motion_blur, 3 f32 a tile (ux, uy, l), rows of *tiles_x; *tiles_x and
 * *tiles_y (either may be NULL) receive the tile counts, which is all a call with host_uvl NULL and n_floats 0 asks for.
 * Rust: pub fn rsrt_motion_tiles_download(ctx: *mut RsrtContext, host_uvl: *mut f32, n_floats: usize, tiles_x: *mut u32, tiles_y: *mut u32) -> i32; */
rsrt_status rsrt_motion_tiles_download(rsrt_context *ctx, float *host_uvl, size_t n_floats, uint32_t *tiles_x, uint32_t *tiles_y);
/* Rust: pub fn rsrt_motion_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_motion_reset(rsrt_context *ctx); /* drops the motion image */

/* -- volumetric fog: a ray-marched sun-shaft pass and a fogged image (no reference counterpart) ----------------------------------
 * Every pass above rearranges radiance the integrator produced; none puts anything between the camera and the surfaces.
 * rsrt_fog_render marches a homogeneous participating medium along the camera rays rsrt_render casts: per pixel and sample, `steps`
 * points between the camera and the first hit (or max_distance), each asked by a shadow query against the scene whether it sees the
 * one directional light, each adding Henyey-Greenstein single scattering from the light where it does and a constant ambient term
 * everywhere, attenuated by the medium up to the point.  The pixel's record, 4 f32, gains (inscatter rgb, transmittance of the whole
 * segment) per sample; split calls give the bits of one call.  rsrt_fog_apply composes one of the four images with the records into
 * the fog image: colour * mean transmittance + mean inscatter.  It goes BEFORE the lens: rsrt_dof, rsrt_motion_blur, both meters,
 * bloom, local exposure and every display take the fog image as their source RSRT_EXPOSURE_FOG; for the lens and the shutter it
 * carries the first-hit records of the image it was built from.  The arithmetic is published in include/rsrt_fog.h (which also says
 * what the model leaves out: the light's own attenuation, multiple scattering, fog inside the integrator) and is bitwise
 * reproducible.  With density 0 the fog image is the source's colour bit for bit.
 *
 * The fog records have a size of their own, like the guide: library-owned (allocated zeroed on first use or when the given size
 * changes) or the caller's (rsrt_fog_bind).  rsrt_fog_render needs a scene and no accumulator.  The fog image has the size of the
 * source it was built from and stays valid until the next rsrt_fog_apply, rsrt_fog_reset, a change of the accumulator's size or
 * rsrt_context_destroy.  Whole frame only, like the denoiser: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.
 * Nothing here writes the accumulator, the AOV buffer, the guide or any other image of the context.  A refused call launches nothing
 * and leaves records and image as they were.
 * rsrt_fog_params (include/rsrt_types.h) defaults: density 0.05, albedo 1, anisotropy 0.6, ambient 0, max_distance 50, steps 16,
 * flags RSRT_FOG_JITTER (RSRT_FOG_* in include/rsrt_fog.h); the light has no default: rsrt_fog_light_from_sky there gives a sky's sun.
 * rsrt_fog_params_ok (there) accepts each field within the range rsrt_types.h gives it, and of those sets the ones for which one
 * sample stays finite ("Finiteness" in rsrt_fog.h): with S = (s * phase_hi) * max light_irradiance + s * max ambient, s = density *
 * max albedo, phase_hi the phase function at cos = +-1 with q's lower bound, and W_hi = min(max_distance, delta_hi + 1 / (density +
 * density^2 * delta_hi / 2)), delta_hi = max_distance / steps, it wants steps * S and S * W_hi at most 0.99 of the largest float.  The
 * largest irradiance beside density 1e6, or beside |anisotropy| 0.95 at density 1, is refused; either alone is not.  Every record of
 * an accepted set is finite sample by sample; summed over very many samples it may reach +inf, never NaN. */
enum { RSRT_EXPOSURE_FOG = 6 }; /* the last rsrt_fog_apply output: a source of the lens, the shutter, the meters, bloom, local exposure and the displays */
/* Adds the fog of samples [sample_begin, sample_begin + sample_count) of a width x height frame seen through `camera` to the fog
 * records.  Asynchronous on hip_stream, NULL = the context's stream, ordered after everything enqueued so far.
 * RSRT_ERR_NOT_READY without a scene; RSRT_ERR_INVALID_ARGUMENT for NULL camera or params, params rsrt_fog_params_ok refuses, a bad
 * resolution or sample range as in rsrt_aov_render, bound records of another size.
 * Rust: pub fn rsrt_fog_render(ctx: *mut RsrtContext, camera: *const RsrtCamera, width: u32, height: u32, sample_begin: u32,
 *                              sample_count: u32, params: *const RsrtFogParams, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_fog_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                            uint32_t sample_count, const rsrt_fog_params *params, void *hip_stream);
/* The caller's device memory (width x height x 4 f32, 16-byte aligned) as the fog records; NULL: back to the library's.
 * Rust: pub fn rsrt_fog_bind(ctx: *mut RsrtContext, device_f32x4: *mut c_void, width: u32, height: u32) -> i32; */
rsrt_status rsrt_fog_bind(rsrt_context *ctx, void *device_f32x4, uint32_t width, uint32_t height);
/* Rust: pub fn rsrt_fog_clear(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_fog_clear(rsrt_context *ctx); /* zeroes the records; RSRT_ERR_NOT_READY without any */
/* Waits and copies the records, 4 f32 a pixel (inscatter sum rgb, transmittance sum).  RSRT_ERR_NOT_READY without records;
 * RSRT_ERR_INVALID_ARGUMENT for another n_floats.
 * Rust: pub fn rsrt_fog_download(ctx: *mut RsrtContext, host_f32x4: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_fog_download(rsrt_context *ctx, float *host_f32x4, size_t n_floats);
/* Builds the fog image of `source` (RSRT_EXPOSURE_MEAN .. _UPSAMPLED) and the records of fog_sample_total samples into
 * device_out_rgba32f (device memory, W x H x 4 f32, 16-byte aligned, alpha 1) or, when that is NULL, into library-owned memory.
 * Asynchronous on hip_stream.  sample_total is ignored for all sources but RSRT_EXPOSURE_MEAN.  RSRT_ERR_NOT_READY when the source
 * image or the records do not exist; RSRT_ERR_INVALID_ARGUMENT for RSRT_EXPOSURE_LENS, _MOTION, _FOG or an unknown source,
 * fog_sample_total 0, sample_total 0 under RSRT_EXPOSURE_MEAN, records of another size than the source, a misaligned output pointer.
 * Rust: pub fn rsrt_fog_apply(ctx: *mut RsrtContext, source: u32, sample_total: u32, fog_sample_total: u32,
 *                             device_out_rgba32f: *mut c_void, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_fog_apply(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t fog_sample_total, void *device_out_rgba32f,
                           void *hip_stream);
/* rsrt_fog_apply for fog records SMALLER than the source (marched at half size, say: rsrt_fog_render with a width and height of its
 * own): the fog image of the source's size W x H is rebuilt from the w x h records (w <= W, h <= H) and the source's first-hit
 * records — the guide for RSRT_EXPOSURE_UPSAMPLED, the AOV buffer otherwise — of record_sample_total samples.  The inscatter is
 * divided by 1 - transmittance per low pixel, upsampled with a tent over 3 x 3 low pixels and multiplied by 1 - tau, where tau is the
 * output pixel's own transmittance, computed from its first-hit record and `params` (those the records were rendered with; density and
 * max_distance are read); out = colour * tau + inscatter.  The arithmetic is published in include/rsrt_fog_upsample.h and is bitwise
 * reproducible; with density 0 the fog image is the source's colour bit for bit.  Equal sizes are allowed and give the 3 x 3 tent, not
 * rsrt_fog_apply's result.  It leaves the fog image and its first-hit records exactly as rsrt_fog_apply does, so every later pass takes
 * the result as RSRT_EXPOSURE_FOG.  It refuses what rsrt_fog_apply refuses, records of another size excepted, and with
 * RSRT_ERR_INVALID_ARGUMENT NULL params, params rsrt_fog_params_ok refuses, record_sample_total 0, fog records wider or taller than the
 * source and first-hit records of another size than the source; RSRT_ERR_NOT_READY without first-hit records.  A refused call launches
 * nothing and leaves records and image as they were.
 * Rust: pub fn rsrt_fog_apply_upsampled(ctx: *mut RsrtContext, source: u32, sample_total: u32, fog_sample_total: u32,
 *                                       record_sample_total: u32, params: *const RsrtFogParams, device_out_rgba32f: *mut c_void,
 *                                       hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_fog_apply_upsampled(rsrt_context *ctx, uint32_t source, uint32_t sample_total, uint32_t fog_sample_total,
                                     uint32_t record_sample_total, const rsrt_fog_params *params, void *device_out_rgba32f, void *hip_stream);
/* Waits and copies the fog image to host_rgba as RGBA32F, alpha 1.  RSRT_ERR_NOT_READY without a fog image since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for another n_floats than 4 a pixel.
 * Rust: pub fn rsrt_fog_image_download(ctx: *mut RsrtContext, host_rgba: *mut f32, n_floats: usize) -> i32; */
rsrt_status rsrt_fog_image_download(rsrt_context *ctx, float *host_rgba, size_t n_floats);
/* Rust: pub fn rsrt_fog_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_fog_reset(rsrt_context *ctx); /* drops the records (a bound buffer is the caller's again) and the fog image */

/* -- white balance and colour grading: a chroma meter, a LUT display (no reference counterpart) ----------------------------------
 * The meter removes the picture's dependence on the environment's scale; nothing so far removes its dependence on the environment's
 * COLOUR: a low sun or a warm HDRI puts a cast over all of it, and the display ends in one hard-wired ACES -> sRGB step with nowhere to
 * put a look.  rsrt_white_meter builds, on the device and in integers, a 64 x 64 histogram of the log-chromaticity (log2 G/R, log2
 * G/B; 16 bins an octave, -2 .. +2 octaves; word 4096 counts the pixels without three positive channels) of one of the five images
 * the library can hold; rsrt_white_download turns it into a white point — per-channel gains that take the mode of the histogram,
 * found by a gated mean shift, to grey at constant luminance.  rsrt_colour_lut_build bakes an ASC CDL (slope, offset, power,
 * saturation) into an n^3 LUT on the device, rsrt_colour_lut_upload takes any LUT; the LUT's domain is the tone-mapped colour,
 * square-root encoded on both sides.  rsrt_display_colour_srgb8 is the graded display pass (local exposure and bloom optional) with
 * the white point multiplied in before the tone map and the LUT, read by tetrahedral interpolation, behind it.  The arithmetic is
 * published in include/rsrt_colour.h and is bitwise reproducible.  The gains are per channel in the working RGB: no chromatic
 * adaptation in a cone space is made, and the integrator knows nothing of the white point.
 *
 * The library keeps NO white point: adaptation over time goes through `previous` and `blend` (the State classes remember the last
 * value).  The histogram stays valid until the next rsrt_white_meter, rsrt_white_reset or rsrt_context_destroy; the LUT until the next
 * rsrt_colour_lut_build or _upload, rsrt_colour_lut_reset or rsrt_context_destroy; neither depends on the accumulator's size.  Whole
 * frame only: with world_size > 1 every call returns RSRT_ERR_INVALID_ARGUMENT.  Nothing here writes the accumulator, the AOV buffer,
 * the guide, any history, the denoised, upsampled or lens image, the exposure histogram, the bloom image or the local-exposure grid.
 * A refused call launches nothing and leaves the last histogram and LUT as they were.
 * rsrt_white_params defaults: gate 12, iterations 3, min_permille 50, strength 1, max_stops 2, blend 1, previous {0, 0, 0}, flags 0;
 * rsrt_cdl_params defaults: the identity; the default LUT size is 33 (RSRT_WHITE_*, RSRT_CDL_*, RSRT_COLOUR_* in
 * include/rsrt_colour.h). */
typedef struct rsrt_white_params {
    uint32_t gate;          /* 1 .. 31: half the width of the mean shift's window, in bins (1/16 octave) */
    uint32_t iterations;    /* 0 .. 8 mean-shift steps */
    uint32_t min_permille;  /* 0 .. 1000: no estimate when fewer than this share of all pixels lies in the final window */
    float strength;         /* 0 .. 1: how much of the cast the gains remove */
    float max_stops;        /* 0 .. 4: the most octaves a channel's gain moves, either way, before the luminance is put back */
    float blend;            /* 0 .. 1: how far the white point moves from `previous` towards the target */
    float previous[3];      /* all 0: none, the white point is the target; otherwise every channel finite and > 0 */
    uint32_t flags;         /* 0 */
} rsrt_white_params;
typedef struct rsrt_white_result {
    float white[3];         /* what to display with */
    float target[3];        /* the gains of this histogram alone */
    float illuminant[3];    /* the estimated cast, green 1 */
    float eu, ev;           /* log2 G/R and log2 G/B of the estimate, octaves */
    uint32_t gated;         /* pixels in the final window */
    uint32_t counted, skipped; /* pixels in the 4096 bins; pixels without three positive channels */
    uint32_t estimated;     /* 1: an estimate; 0: none (white = target = previous, or {1, 1, 1}) */
    uint32_t _pad;
} rsrt_white_result;
typedef struct rsrt_cdl_params {
    float slope[3];   /* 0 .. 16 */
    float offset[3];  /* -1 .. 1 */
    float power[3];   /* 0.25 .. 4 */
    float saturation; /* 0 .. 4 */
    uint32_t flags;   /* 0 */
    uint32_t _pad;
} rsrt_cdl_params;
typedef struct rsrt_colour_params {
    float white[3];     /* finite, > 0: multiplied in before the tone map */
    float lut_strength; /* 0 .. 1: 0 skips the LUT, which then need not exist */
    uint32_t flags;     /* 0 */
    uint32_t _pad[3];
} rsrt_colour_params;
/* Builds the chroma histogram of `source` (RSRT_EXPOSURE_MEAN .. RSRT_EXPOSURE_LENS) in a library-owned buffer (one launch;
 * asynchronous on hip_stream, NULL = the context's stream, ordered after everything enqueued so far).  Sources, sample_total and errors
 * as for rsrt_exposure_meter.
 * Rust: pub fn rsrt_white_meter(ctx: *mut RsrtContext, source: u32, sample_total: u32, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_white_meter(rsrt_context *ctx, uint32_t source, uint32_t sample_total, void *hip_stream);
/* Waits, copies the last histogram's 4097 words to host_hist and fills *out from it (rsrt_white_from_histogram, on the host).
 * host_hist may be NULL (n_words is then ignored), out may be NULL.  RSRT_ERR_NOT_READY without a histogram since the last reset;
 * RSRT_ERR_INVALID_ARGUMENT for NULL params, params rsrt_white_params_ok refuses, n_words != 4097 with a non-NULL host_hist.
 * Rust: pub fn rsrt_white_download(ctx: *mut RsrtContext, params: *const RsrtWhiteParams, host_hist: *mut u32, n_words: usize,
 *                                  out: *mut RsrtWhiteResult) -> i32; */
rsrt_status rsrt_white_download(rsrt_context *ctx, const rsrt_white_params *params, uint32_t *host_hist, size_t n_words, rsrt_white_result *out);
/* Rust: pub fn rsrt_white_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_white_reset(rsrt_context *ctx); /* drops the histogram */
/* Bakes the n^3 LUT of `cdl` on the device (rsrt_colour_lut_node per node; 16 bytes a node: 575 KB at n = 33); asynchronous on
 * hip_stream.  RSRT_ERR_INVALID_ARGUMENT for an n other than 2, 3, 17, 33, 65, NULL cdl or one rsrt_cdl_params_ok refuses.
 * Rust: pub fn rsrt_colour_lut_build(ctx: *mut RsrtContext, n: u32, cdl: *const RsrtCdlParams, hip_stream: *mut c_void) -> i32; */
rsrt_status rsrt_colour_lut_build(rsrt_context *ctx, uint32_t n, const rsrt_cdl_params *cdl, void *hip_stream);
/* Takes a LUT from the host: 3 * n^3 floats, rgb a node, red fastest, in the encoded domain.  RSRT_ERR_INVALID_ARGUMENT for an n
 * other than 2, 3, 17, 33, 65, NULL, another n_floats, or any value that is not finite and in [0, 1].
 * Rust: pub fn rsrt_colour_lut_upload(ctx: *mut RsrtContext, n: u32, host_rgb: *const f32, n_floats: usize) -> i32; */
rsrt_status rsrt_colour_lut_upload(rsrt_context *ctx, uint32_t n, const float *host_rgb, size_t n_floats);
/* Waits and copies the LUT's 3 * n^3 floats to host_rgb; *n_out (may be NULL) receives n, which is all a call with host_rgb NULL
 * and n_floats 0 asks for.  RSRT_ERR_NOT_READY without a LUT; RSRT_ERR_INVALID_ARGUMENT for another n_floats.
 * Rust: pub fn rsrt_colour_lut_download(ctx: *mut RsrtContext, host_rgb: *mut f32, n_floats: usize, n_out: *mut u32) -> i32; */
rsrt_status rsrt_colour_lut_download(rsrt_context *ctx, float *host_rgb, size_t n_floats, uint32_t *n_out);
/* Rust: pub fn rsrt_colour_lut_reset(ctx: *mut RsrtContext) -> i32; */
rsrt_status rsrt_colour_lut_reset(rsrt_context *ctx); /* drops the LUT */
/* `source` through the colour display pass: rsrt_display_pixel_colour per pixel (include/rsrt_colour.h), RGBA8, alpha 255.  `local`
 * may be NULL: the local gain is then 1 and no grid is needed.  With bloom_intensity 0 no bloom image is needed, with lut_strength 0
 * no LUT.  With white {1, 1, 1} and lut_strength 0 the bytes are rsrt_display_local_srgb8's or, with a NULL local, those of
 * rsrt_display_bloomed_srgb8 / rsrt_display_exposed_srgb8.  Errors as for rsrt_display_local_srgb8 (a NULL local is none), and
 * RSRT_ERR_INVALID_ARGUMENT for NULL colour or one rsrt_colour_params_ok refuses (white not finite and > 0, lut_strength outside
 * [0, 1], flags), RSRT_ERR_NOT_READY with lut_strength > 0 and no LUT.
 * Rust: pub fn rsrt_display_colour_srgb8(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                        local: *const RsrtLocalParams, bloom_intensity: f32, colour: *const RsrtColourParams,
 *                                        host_rgba8: *mut u8, n_bytes: usize) -> i32; */
rsrt_status rsrt_display_colour_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                                      float bloom_intensity, const rsrt_colour_params *colour, uint8_t *host_rgba8, size_t n_bytes);

/* -- finished display: sharpening, film grain and dither after the tone map (no reference counterpart) ---------------------------
 * Every pass so far works on linear radiance BEFORE the tone map; behind it stood one hard quantiser.  rsrt_display_finished_srgb8 is
 * rsrt_display_colour_srgb8 with three display-referred steps between the LUT and the byte, all in the square-root domain the LUT
 * uses: a contrast-adaptive sharpener over a pixel's cross (FSR 1's RCAS, optionally with its noise limiter), monochrome film grain
 * shaped so that it cannot leave [0, 1] (FSR 1's LFGA), and a triangular dither of one code's amplitude over the sRGB thresholds,
 * which breaks up the bands of skies, fog and bloom at 8 bits.  The noise is an integer hash of (x, y, seed, draw): the library keeps
 * NO seed, the same seed gives the same bytes, and a caller who wants grain that moves passes a frame index.  The arithmetic is
 * published in include/rsrt_finish.h and is bitwise reproducible; with sharpness, grain and dither all 0 the bytes are
 * rsrt_display_colour_srgb8's.  There is no sharpened IMAGE: the result exists only as bytes, and no other pass can take it as a source.
 * Whole frame only.  Nothing here writes any buffer the context holds.  A refused call launches nothing.
 * rsrt_finish_params defaults: sharpness 0.5, grain 0, dither 1, seed 0, flags 0 (RSRT_FINISH_* in include/rsrt_finish.h). */
#define RSRT_FINISH_NOISE_AWARE 1u /* rsrt_finish_params.flags: sharpen less where a pixel stands out of its cross (salt and pepper at 1 - 4 spp) */
typedef struct rsrt_finish_params {
    float sharpness; /* 0 .. 1: 0 skips the sharpener (and its kernel variant reads no neighbour) */
    float grain;     /* 0 .. 1: the grain's amplitude as a share of min(enc, 1 - enc) */
    float dither;    /* 0 .. 1: the dither's amplitude in codes; 0 is the hard quantiser */
    uint32_t seed;   /* of the noise */
    uint32_t flags;  /* RSRT_FINISH_NOISE_AWARE or 0 */
    uint32_t _pad[3];
} rsrt_finish_params;
/* `source` through the finished display pass: rsrt_finish_sdr per pixel, then rsrt_finish_pixel over its cross (include/rsrt_finish.h),
 * RGBA8, alpha 255.  Sources, `local`, bloom_intensity, `colour`, readiness and errors exactly as for rsrt_display_colour_srgb8, and
 * RSRT_ERR_INVALID_ARGUMENT for NULL finish or one rsrt_finish_params_ok refuses (sharpness, grain or dither not finite and in [0, 1],
 * an unknown flag).
 * Rust: pub fn rsrt_display_finished_srgb8(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                          local: *const RsrtLocalParams, bloom_intensity: f32, colour: *const RsrtColourParams,
 *                                          finish: *const RsrtFinishParams, host_rgba8: *mut u8, n_bytes: usize) -> i32; */
rsrt_status rsrt_display_finished_srgb8(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                                        float bloom_intensity, const rsrt_colour_params *colour, const rsrt_finish_params *finish, uint8_t *host_rgba8,
                                        size_t n_bytes);

/* -- HDR display: PQ 10-bit and scRGB output with content light levels (no reference counterpart) ----------------------------------
 * Every display above ends in rsrt_aces_tone_map and an sRGB byte.  rsrt_display_hdr is the colour display's chain up to the tone map —
 * the f16-rounded mean times exposure, plus the bloom, times the local gain, times the white point: linear Rec.709 in units of paper
 * white — and then, instead of the tone map, a hue-preserving shoulder between knee * peak and peak, the scale to nits and one of two
 * encodings for an HDR surface: RSRT_HDR_PQ10, Rec.2020 primaries (BT.2087's matrix) under the SMPTE ST 2084 curve, three 10-bit codes
 * packed R | G << 10 | B << 20 | 3 << 30 into one uint32 a pixel (HDR10 on wgpu Rgb10a2Unorm, DXGI R10G10B10A2, Vulkan
 * A2B10G10R10_PACK32), optionally with rsrt_display_finished_srgb8's triangular dither over the PQ thresholds; or RSRT_HDR_SCRGB16F,
 * linear Rec.709 with 1.0 = 80 cd/m^2 as four binary16 a pixel, alpha 1 (scRGB on Rgba16Float).  The same call can return the frame's
 * content light levels (CTA-861.3 MaxCLL and MaxFALL, HDR10's static metadata), reduced on the device in integers.  The arithmetic is
 * published in include/rsrt_hdr.h and is bitwise reproducible.  The colour LUT is display-referred SDR and does not apply: lut_strength
 * > 0 is refused.  There is no HDR IMAGE: the result exists only as output words, and no other pass can take it as a source.  Whole
 * frame only.  Nothing here writes any buffer the context holds.  A refused call launches nothing.
 * rsrt_hdr_params defaults: paper white 203 cd/m^2 (BT.2408), peak 1000, knee 0.5, dither 0, seed 0, RSRT_HDR_PQ10, flags 0
 * (RSRT_HDR_* in include/rsrt_hdr.h). */
#define RSRT_HDR_PQ10 0u     /* rsrt_hdr_params.encoding: 4 bytes a pixel */
#define RSRT_HDR_SCRGB16F 1u /* 8 bytes a pixel */
typedef struct rsrt_hdr_params {
    float paper_white_nits; /* 1 .. 10000: the luminance of a linear 1.0 (diffuse white) */
    float peak_nits;        /* paper_white_nits .. 10000: the display's peak; no channel leaves the call brighter */
    float knee;             /* 0 .. 0.95: the share of the peak below which a pixel passes unchanged */
    float dither;           /* 0 .. 1: the dither's amplitude in codes (RSRT_HDR_PQ10 only); 0 is the hard quantiser */
    uint32_t seed;          /* of the dither's noise */
    uint32_t encoding;      /* RSRT_HDR_PQ10 or RSRT_HDR_SCRGB16F */
    uint32_t flags;         /* 0 */
    uint32_t _pad;
} rsrt_hdr_params;
typedef struct rsrt_hdr_levels {
    uint64_t sum_q;  /* the sum over the frame's pixels of q = (uint32_t)(max(R, G, B) in nits * 64), in the encoding's primaries */
    uint32_t max_q;  /* the largest q */
    float max_cll;   /* max_q / 64: CTA-861.3 MaxCLL, cd/m^2 */
    float max_fall;  /* sum_q / (64 * pixels): MaxFALL of this one frame, cd/m^2 */
    uint32_t _pad;
} rsrt_hdr_levels;
/* `source` through the HDR display pass: rsrt_hdr_pixel_nits, then rsrt_hdr_pack_pq10 or rsrt_hdr_pack_scrgb per pixel
 * (include/rsrt_hdr.h).  n_bytes: pixels * 4 for RSRT_HDR_PQ10 (host_out holds uint32 words), pixels * 8 for RSRT_HDR_SCRGB16F (four
 * uint16 a pixel).  levels_out may be NULL: the reduction is then not run.  Sources, `local`, bloom_intensity, `colour`, readiness and
 * errors exactly as for rsrt_display_colour_srgb8, and RSRT_ERR_INVALID_ARGUMENT for NULL hdr, one rsrt_hdr_params_ok refuses (a value
 * outside the ranges above or not finite, peak below paper white, an unknown encoding or flag, dither > 0 with RSRT_HDR_SCRGB16F),
 * colour->lut_strength > 0, NULL host_out or another n_bytes.  A refused call writes neither host_out nor *levels_out.
 * Rust: pub fn rsrt_display_hdr(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                               local: *const RsrtLocalParams, bloom_intensity: f32, colour: *const RsrtColourParams,
 *                               hdr: *const RsrtHdrParams, host_out: *mut c_void, n_bytes: usize, levels_out: *mut RsrtHdrLevels) -> i32; */
rsrt_status rsrt_display_hdr(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                             float bloom_intensity, const rsrt_colour_params *colour, const rsrt_hdr_params *hdr, void *host_out, size_t n_bytes,
                             rsrt_hdr_levels *levels_out);

/* -- video output: Y'CbCr 4:2:0 frames at 8 and 10 bits (no reference counterpart) -------------------------------------------------
 * What an encoder, a stream or a player takes.  rsrt_display_video is the colour display's chain (RSRT_VIDEO_BT709: up to and with the
 * tone map and the LUT, the colour rsrt_display_colour_srgb8 quantises) or the HDR display's (RSRT_VIDEO_HDR10: rsrt_display_hdr's
 * Rec.2020 nits behind the shoulder), then per pixel a continuous transfer code over the sRGB or the PQ thresholds (no pow), the
 * BT.709 or the BT.2020 non-constant-luminance matrix, a 2 x 2 chroma reduction at one of three sitings, a quantiser at 8 or 10 bits
 * in limited or full range with an optional triangular dither, and a semi-planar (NV12, P010) or planar (I420, yuv420p10le) frame of a
 * third to three quarters of the RGB words' size.  The arithmetic is published in include/rsrt_video.h and is bitwise reproducible;
 * rsrt_video_planes there gives the frame's byte count and where its planes lie.  There is no video IMAGE: the frame exists only as
 * output bytes, and no pass takes it as a source.  Whole frame only.  Nothing here writes any buffer the context holds.  A refused
 * call launches nothing.  H.273 tags of the result: RSRT_VIDEO_BT709 colour primaries 1, transfer 13 (sRGB), matrix 1;
 * RSRT_VIDEO_HDR10 9, 16, 9; chroma sample location type = siting.
 * rsrt_video_params defaults: RSRT_VIDEO_BT709, 8 bits, RSRT_VIDEO_SEMIPLANAR, RSRT_VIDEO_LIMITED, RSRT_VIDEO_SITING_LEFT, dither 0,
 * seed 0, flags 0 (RSRT_VIDEO_DEFAULT_* in include/rsrt_video.h). */
#define RSRT_VIDEO_BT709 0u          /* rsrt_video_params.standard: SDR, sRGB transfer, BT.709 matrix */
#define RSRT_VIDEO_HDR10 1u          /* Rec.2020 primaries, PQ transfer, BT.2020 NCL matrix; 10 bits only */
#define RSRT_VIDEO_SEMIPLANAR 0u     /* .layout: a Y plane, then one plane of interleaved Cb, Cr: NV12 at 8 bits, P010 (code << 6) at 10 */
#define RSRT_VIDEO_PLANAR 1u         /* Y, Cb, Cr planes: I420 at 8 bits, yuv420p10le (code in the low bits) at 10 */
#define RSRT_VIDEO_LIMITED 0u        /* .range: luma 16 .. 235, chroma 16 .. 240 (times 4 at 10 bits) */
#define RSRT_VIDEO_FULL 1u           /* 0 .. 2^depth - 1 */
#define RSRT_VIDEO_SITING_LEFT 0u    /* .siting, H.273 chroma sample location type 0: MPEG-2, H.264, HEVC default */
#define RSRT_VIDEO_SITING_CENTRE 1u  /* type 1: JPEG, MPEG-1 */
#define RSRT_VIDEO_SITING_TOPLEFT 2u /* type 2: HDR10, UHD */
typedef struct rsrt_video_params {
    uint32_t standard; /* RSRT_VIDEO_BT709 or RSRT_VIDEO_HDR10 */
    uint32_t depth;    /* 8 or 10 bits a sample; RSRT_VIDEO_HDR10: 10 */
    uint32_t layout;   /* RSRT_VIDEO_SEMIPLANAR or RSRT_VIDEO_PLANAR */
    uint32_t range;    /* RSRT_VIDEO_LIMITED or RSRT_VIDEO_FULL */
    uint32_t siting;   /* RSRT_VIDEO_SITING_* */
    float dither;      /* 0 .. 1: the dither's amplitude in codes; 0 is the hard quantiser */
    uint32_t seed;     /* of the dither's noise */
    uint32_t flags;    /* 0 */
} rsrt_video_params;
/* `source` through the video pass (include/rsrt_video.h) into host_out, n_bytes = rsrt_video_planes(width, height, video, ..) of the
 * source's size.  hdr: NULL with RSRT_VIDEO_BT709; required with RSRT_VIDEO_HDR10, its encoding RSRT_HDR_PQ10, its dither and seed not
 * looked at.  levels_out: may be non-NULL only with RSRT_VIDEO_HDR10, and then holds the very integers rsrt_display_hdr gives for the
 * same parameters.  Sources, `local`, bloom_intensity, `colour`, readiness and errors exactly as for rsrt_display_colour_srgb8 and
 * rsrt_display_hdr (colour->lut_strength > 0 is refused with RSRT_VIDEO_HDR10), and RSRT_ERR_INVALID_ARGUMENT for NULL video, one
 * rsrt_video_params_ok refuses (an unknown enumerator, a depth other than 8 or 10, RSRT_VIDEO_HDR10 at 8 bits, a dither outside
 * [0, 1] or not finite, a flag), hdr or levels_out where they do not belong, NULL host_out or another n_bytes.  A refused call writes
 * neither host_out nor *levels_out.
 * Rust: pub fn rsrt_display_video(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                 local: *const RsrtLocalParams, bloom_intensity: f32, colour: *const RsrtColourParams,
 *                                 hdr: *const RsrtHdrParams, video: *const RsrtVideoParams, host_out: *mut c_void, n_bytes: usize,
 *                                 levels_out: *mut RsrtHdrLevels) -> i32; */
rsrt_status rsrt_display_video(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                               float bloom_intensity, const rsrt_colour_params *colour, const rsrt_hdr_params *hdr, const rsrt_video_params *video,
                               void *host_out, size_t n_bytes, rsrt_hdr_levels *levels_out);

/* -- JPEG output: a baseline JPEG / JFIF file built on the device (no reference counterpart) --------------------------------------------
 * What every viewer and browser opens.  rsrt_display_jpeg is the colour display's chain up to and with the tone map and the LUT (the
 * colour rsrt_display_colour_srgb8 quantises), then JFIF's BT.601 full-range Y'CbCr, 4:2:0 at the centre siting or 4:4:4, an 8 x 8 f32
 * DCT, the IJG-scaled Annex K quantisation tables and the Annex K Huffman tables: three launches (blocks, an exclusive scan of the
 * blocks' bit counts, the packer) and a copy of the scan alone: at 1920 x 1080 a quality-90 file of a noisy 8-spp render measured a
 * quarter of an NV12 frame's bytes, and the call 4.5 times the NV12 call (DESIGN.md 27 says where the time goes).  The arithmetic is
 * published in include/rsrt_jpeg.h and is bitwise reproducible; the host writes the headers, stuffs the scan and ends the file.  Whole
 * frame only.  Nothing here writes any buffer the context holds.  A refused call launches nothing and writes nothing.
 * rsrt_jpeg_params defaults: quality 90, RSRT_JPEG_420, flags 0, reserved 0 (RSRT_JPEG_DEFAULT_* in include/rsrt_jpeg.h). */
#define RSRT_JPEG_420 0u /* rsrt_jpeg_params.subsampling: MCU 16 x 16, four Y blocks, Cb, Cr */
#define RSRT_JPEG_444 1u /* MCU 8 x 8: Y, Cb, Cr */
typedef struct rsrt_jpeg_params {
    uint32_t quality;     /* 1 .. 100, the IJG scale */
    uint32_t subsampling; /* RSRT_JPEG_420 or RSRT_JPEG_444 */
    uint32_t flags;       /* 0 */
    uint32_t reserved;    /* 0 */
} rsrt_jpeg_params;
/* `source` as a complete JPEG file in host_out, *n_bytes_out its size.  capacity: host_out's room; rsrt_jpeg_max_bytes (rsrt_jpeg.h) of
 * the source's size always suffices.  Sources, local, bloom_intensity, colour, readiness, the partition refusal and the order of the
 * checks are rsrt_display_colour_srgb8's; RSRT_ERR_INVALID_ARGUMENT also for NULL jpeg, host_out or n_bytes_out, params
 * rsrt_jpeg_params_ok refuses (quality outside 1 .. 100, an unknown subsampling, a flag, reserved != 0), and a frame whose worst case
 * reaches 2^32 bits (rsrt_jpeg_size_ok in rsrt_jpeg.h).  A capacity smaller than the file: RSRT_ERR_INVALID_ARGUMENT with *n_bytes_out the size needed, host_out untouched
 * (the kernels have run by then: the size is the coded scan's).
 * Rust: pub fn rsrt_display_jpeg(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32, local: *const RsrtLocalParams,
 *                                bloom_intensity: f32, colour: *const RsrtColourParams, jpeg: *const RsrtJpegParams,
 *                                host_out: *mut c_void, capacity: usize, n_bytes_out: *mut usize) -> i32; */
rsrt_status rsrt_display_jpeg(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                              float bloom_intensity, const rsrt_colour_params *colour, const rsrt_jpeg_params *jpeg, void *host_out,
                              size_t capacity, size_t *n_bytes_out);
/* The first stage alone: the quantised coefficients, int16 in zigzag order, 64 a block, blocks in scan order (DC as it is, not its
 * difference).  n_values = 64 * rsrt_jpeg_blocks(width, height, subsampling).  Refusals as above.
 * Rust: pub fn rsrt_display_jpeg_coefficients(ctx: *mut RsrtContext, source: u32, sample_total: u32, exposure: f32,
 *                                             local: *const RsrtLocalParams, bloom_intensity: f32, colour: *const RsrtColourParams,
 *                                             jpeg: *const RsrtJpegParams, host_coefs: *mut i16, n_values: usize) -> i32; */
rsrt_status rsrt_display_jpeg_coefficients(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local,
                                           float bloom_intensity, const rsrt_colour_params *colour, const rsrt_jpeg_params *jpeg, int16_t *host_coefs,
                                           size_t n_values);
/* The second and third stage on the caller's coefficients (that layout) of a width x height picture: the file that quality's tables
 * and these coefficients make.  Needs no picture and no scene.  RSRT_ERR_INVALID_ARGUMENT also for a size of 0, another n_values and a
 * value outside [-1023, 1023] (a DC: [-1024, 1023]), found before anything is launched; the capacity protocol is rsrt_display_jpeg's.
 * Rust: pub fn rsrt_jpeg_encode_coefficients(ctx: *mut RsrtContext, width: u32, height: u32, jpeg: *const RsrtJpegParams,
 *                                            host_coefs: *const i16, n_values: usize, host_out: *mut c_void, capacity: usize,
 *                                            n_bytes_out: *mut usize) -> i32; */
rsrt_status rsrt_jpeg_encode_coefficients(rsrt_context *ctx, uint32_t width, uint32_t height, const rsrt_jpeg_params *jpeg, const int16_t *host_coefs,
                                          size_t n_values, void *host_out, size_t capacity, size_t *n_bytes_out);

/* -- ray-query probe: cast_ray / cast_ray_bvh for a batch of rays (shader.wgsl:469-601) -------
 * Exists for parity tests of traversal + intersection without the RNG: out records are
 * {did_hit u32, distance f32, hit_point 3xf32, normal 3xf32, material_id u32} = 36 bytes.
 * mode bit 0: 0 = cast_ray (BVH, then the brute-force fallback), 1 = cast_ray_bvh only;
 * mode bits 1-3, the traversal: 0 = threaded tree walk, 1 = the first kernel's stack walk, 2 = tree walk with typed leaf
 *   loops, 3 = flat loop over the leaf boxes (house, default, cube in production), 4 = fixed-order walk with ties
 *   decided by tabulated visiting ranks, 5 = wide walk (4-wide nodes, one ray a lane), 6 = cooperative wide walk (the same
 *   nodes; a wave's rays as (ray, node) / (ray, leaf) work items: suzanne and anything bigger in production) — the very device
 *   functions rt_render_pool_kernel's TRACE stage calls; a scene that does not qualify is RSRT_ERR_INVALID_ARGUMENT;
 * mode bit 4: read the scene from LDS exactly as the production kernel stages it for that traversal (whole image, or
 *   for mid-size scenes the nodes + escape links / the pre-order nodes) instead of from global memory.  Host pointers. */
typedef struct rsrt_hit {
    uint32_t did_hit;
    float distance;
    float hit_point[3];
    float normal[3];
    uint32_t material_id;
} rsrt_hit;
rsrt_status rsrt_cast_rays(rsrt_context *ctx, uint32_t n_rays, const float *origins_xyz, const float *directions_xyz,
                           uint32_t mode, uint32_t flags, rsrt_hit *out);

/* The scene's device image, built on the HOST exactly as rsrt_upload_scene builds it (csrc/hip/rt_scene_image.h, build_scene_image;
 * no context, no GPU: tests/test_scene_image.py reads it on the CPU).  The arrays are rsrt_upload_scene's and are checked the same way;
 * flat_oriented: whether the flat loop gets its per-octant leaf tables (what RSRT_FLAT_ORIENTED sets for a context, 1 by default).
 * image_out (may be NULL): 4 floats per float4; *n_float4: capacity in, count out; info_out (may be NULL): where each section lies
 * and every scalar the upload derives.  RSRT_ERR_INVALID_ARGUMENT: an array, an index or the tree's shape is refused (the reasons
 * rsrt_upload_scene gives; a tree deeper than the traversal stack is not among them here: stack_entries reports it), or image_out
 * is too small (*n_float4 then holds the count). */
typedef struct rsrt_scene_image_info {
    /* where each section begins, in float4s from the start of the image (rt_device.h DevScene names the sections); the LDS image is
     * nodes .. flat_leaves with its tables, flat_rank and what follows stay in global memory */
    uint64_t nodes, escape, prims, tri_normals, materials, fb_spheres, fb_planes, flat_leaves, flat_rank, pnodes, prim_rank, wnodes;
    uint64_t n_float4;          /* the whole image */
    uint64_t traversal_head_f4; /* nodes | escape links: what a mid-size scene's tree walks keep in LDS */
    uint32_t n_nodes, n_prims, n_tris, n_materials, n_spheres, n_planes, n_leaves, n_pnodes, n_wnodes;
    uint32_t tri_mask_lo, tri_mask_hi, plane_mask_lo, plane_mask_hi;
    uint32_t flat_ok, flat_ostride, typed_leaves, wide_ok, wide_deep, coop_ok;
    uint32_t stack_entries; /* tree depth + 1 */
    uint32_t lds_float4s;   /* float4s of the LDS image, 0: it does not fit small_image_bytes */
    float cull_min[8][3], cull_max[8][3];
    uint32_t cull_mask[8], cull_always, n_cull;
    uint32_t top_elems;  /* elements of the fixed-order walk's top block (the head of pnodes) */
    uint32_t wimg_nodes; /* wide nodes a mid-size scene may stage in LDS (all of them; 0 without a wide tree) */
    uint32_t small_image_bytes, hybrid_room_f4; /* the library's LDS room: a whole image's bytes, a walk's head in float4s */
    uint32_t _pad;
} rsrt_scene_image_info;
rsrt_status rsrt_scene_image_build(const rsrt_material *materials, uint32_t n_materials, const rsrt_sphere *spheres, uint32_t n_spheres,
                                   const rsrt_plane *planes, uint32_t n_planes, const rsrt_vec3 *vertices, uint32_t n_vertices,
                                   const rsrt_vec3 *normals, uint32_t n_normals, const rsrt_triangle *triangles, uint32_t n_triangles,
                                   const rsrt_primitive_info *primitives, uint32_t n_primitives, const rsrt_bvh_node *bvh_nodes,
                                   uint32_t n_bvh_nodes, uint32_t flat_oriented, float *image_out, size_t *n_float4,
                                   rsrt_scene_image_info *info_out);

/* The wide walk's tree (csrc/hip/rt_device.h, trace_wide) for a BVH, built on the HOST by the builder of the scene image
 * (csrc/hip/rt_scene_image.h, build_wide_tree; the image's wnodes section holds the same records; no GPU needed;
 * tests/test_wide_tree.py walks it on the CPU): the binary tree collapsed into 4-wide nodes, node 0
 * the root, a node's interior children consecutive, groups of siblings in the order their parents are expanded (largest box first).  wnodes_out (may be NULL): 32 floats per wide node, 8 x {x, y, z, word} — slot k's exact box is {[2k].xyz,
 * [2k + 1].xyz}; the words are the node's: [0] first interior child's node index (interior children come first and are consecutive)
 * | interior-slot mask << 26, [1] first record of the node's leaf children, [2] / [3] which of the 32 records from there are
 * triangles / planes, [4 + k] slot k's records as a mask from there (0: not a leaf); *n_wnodes: capacity in, count out; old_of_new (may be NULL):
 * for every record index the walk uses (whole leaves are reordered so that a wide node's leaf records are contiguous), the
 * index into `primitives` as given.  RSRT_ERR_INVALID_ARGUMENT: the tree's shape is one rsrt_upload_scene refuses, or the BVH does not qualify (boxes that do not nest, leaves of
 * more than 8 records or that share records, a wide tree of more than 25 levels: the walk's eight stack registers + sixteen overflow words) and keeps the fixed-order walk. */
rsrt_status rsrt_wide_tree_build(const rsrt_primitive_info *primitives, uint32_t n_primitives, const rsrt_bvh_node *bvh_nodes, uint32_t n_bvh_nodes,
                                 float *wnodes_out, uint32_t *n_wnodes, uint32_t *old_of_new);

/* Diagnostic words of an instrumented build (-DRT_INSTRUMENT: loop-trip counters behind
 * tools/simd_efficiency.py); all zero in the product build. Cumulative since context creation. */
rsrt_status rsrt_get_debug_counters(rsrt_context *ctx, uint64_t out[32]);
/* ... and the lanes that passed each region mark (rt_math.h RT_MARK; tools/ledger.py sets them against the regions' instruction counts).
 * Read and reset; all zero in the product build. */
rsrt_status rsrt_get_region_counters(rsrt_context *ctx, uint64_t out[32]);
/* What the cooperative wide walk (TRAV 6) did, cumulative since context creation, in the product build: out[0] node trips,
 * [1] leaf trips, [2] 64-item blocks of node items spilled to a wave's arena block, [3] blocks taken back, [4] node trips that
 * popped the newest items, [5] one-item node trips, [6] batches abandoned to the exact walk because the node ring could not take
 * a trip's items (the arena block was full), [7] the most node items one wave held outstanding (a maximum, not a sum).  The probe
 * (rsrt_cast_rays, traversal 6) counts all eight; a render counts only [6] (the counting would cost the render kernel registers it has
 * not got).  The first min(n, 8) words are written, any beyond are zeroed. */
rsrt_status rsrt_get_walk_counters(rsrt_context *ctx, uint64_t *out, uint32_t n);

/* Exhaustive device self-test of the numeric contract's one shortcut: the 3-instruction reciprocal used for
 * 1/x (rt_math.h, rt_rcp) against the compiler's correctly rounded division, over all 2^32 f32 bit patterns
 * (~0.1 s).  out[0] = inputs where the bits differ (must be 0), out[1] = inputs that took the short path,
 * out[2] = of those, how many the bare v_rcp_f32 gets wrong (shows the comparison is live), out[3] = smallest
 * failing bit pattern or UINT64_MAX. */
rsrt_status rsrt_selftest_numerics(rsrt_context *ctx, uint64_t out[4]);
/* Exhaustive device self-test of rsrt_sincosf (rsrt_detmath.h), the fused form the render kernels take the sine and cosine
 * of one angle with, against rsrt_sinf and rsrt_cosf, as bits, over all 2^32 f32 bit patterns (~0.2 s).  out[0] = inputs where
 * either result differs (must be 0), out[1] = inputs checked (2^32), out[2] = 0, out[3] = smallest failing bit pattern or
 * UINT64_MAX. */
rsrt_status rsrt_selftest_sincos(rsrt_context *ctx, uint64_t out[4]);

/* Library / device description, for logs: "librsrt <version>; <device name>; <CUs> CUs". */
const char *rsrt_describe(rsrt_context *ctx);
/* 16 hex digits: sha256 over the kernel sources this library was compiled from (plus any experiment knob).  The
 * rocprofv3 summaries under profiles/ carry the id of the library they were taken on; bench.py attaches a profile
 * to its roofline object only when the ids agree. */
const char *rsrt_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* RSRT_H */
