// rsrt_api.hip — kernels + C-ABI of librsrt.so (include/rsrt.h).  gfx950 only.
//
// Kernel design:
//  rt_render_pool_kernel persistent path-tracing kernel (rt_wavepool.h).  Every WAVE pulls chunks
//                     (one owned framebuffer tile x a block of sample indices) from one global
//                     atomic counter into its pool of path slots.  Each finished path stores its
//                     radiance to the sample buffer [sample][pixel slot]; nothing is accumulated in
//                     flight, so any lane may take any sample and the result cannot depend on
//                     scheduling.
//  rt_resolve_kernel  adds the buffered samples of every owned pixel into the RGBA32F
//                     accumulator in increasing sample order — the exact f32 sum that
//                     `sample_count` successive reference frames produce (shader.wgsl:1367-1371).
//  rt_cast_rays_kernel the ray-query probe.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/rsrt.h"
#include "../../../include/rsrt_tonemap.h"
#include "rt_device.h"

#define RT_BLOCK 256
#define RT_STATS_WORDS 48 // paths, ext, shadow, traversal steps + 32 diagnostic words (zero in the product build), 4 spare, the cooperative walk's 8 (rt_coop.h CoopCount)
#define RT_WAVE 64
#ifndef RT_WALK_POOL
#define RT_WALK_POOL 192u // path slots per wave of the 1024-thread walk kernels (hybrid scene view): measured 128 / 160 / 192 (profiles/r03_wide_walk.txt): the
                          // bigger pool wins even where it takes LDS from the top block (15 k-triangle scene: 161 instead of 352 wide nodes staged, same time)
#endif
#ifndef RT_BIG_POOL
#define RT_BIG_POOL 192u // the default form for a scene whose whole image fits LDS: 1024-thread workgroups, this many slots per wave
#endif

struct RenderParams {
    DevScene scene;
    DevEnv env;
    float cam_pos[3];
    float cam_rot[9]; // columns
    float fov_y;
    uint32_t width, height;
    uint32_t sample_begin, sample_count; // of this pass
    uint32_t max_bounces, flags;
    uint32_t tile_w, tile_h, tiles_x, n_tiles, rank, world, n_owned_tiles;
    uint32_t tiles_per_row, skew; // partition arithmetic, see owned_tile()
    uint32_t samples_per_chunk, n_sblocks, n_chunks;
    uint32_t chunk_px, n_subtiles; // a chunk covers chunk_px consecutive pixels of a tile (tile_px / n_subtiles)
    uint32_t n_slots; // n_owned_tiles * tile_w * tile_h
    uint32_t trace_budget, descend_quorum, flat_quorum, stop_quorum;
    uint32_t coop_lds_cap, coop_lifo_at, coop_narrow_at; // cooperative walk (rt_coop.h): node-queue entries kept in LDS, outstanding items at which a wave pops newest first / one item a trip
    uint32_t coop_gcap; // ... node items a wave may spill to its arena block (<= RT_COOP_GCAP)
    uint32_t *cold_state; // wave-pool kernel: global arena of the cold path-state columns
    float *sample_buf;
    unsigned int *work_counter;
    unsigned long long *stats; // paths, ext_rays, shadow_rays
};

// ------------------------------------------------------------------ framebuffer partition
// The frame is cut into tile_w x tile_h tiles; tile (tx, ty) belongs to rank (tx + ty * skew) % world: interleaved in x, and
// every row shifted by `skew` against the one above, so that a rank's tiles form a lattice whatever tiles_x is (plain
// t % world degenerates to fixed column stripes whenever tiles_x is a multiple of world: 1920 / 16 = 120 tiles, 8 GPUs).
// skew = the smallest odd number >= 3 that has no factor in common with world (3 for 2 / 4 / 8 GPUs).  Every rank owns
// tiles_per_row = ceil(tiles_x / world) tile slots of every tile row — the same number for all ranks, which is what lets the
// frame be GATHERED from equally sized compact buffers (rsrt_comm.h); a slot whose tx falls beyond the frame is padding.
__host__ __device__ inline uint32_t partition_skew(uint32_t world)
{
    for (uint32_t s = 3;; s += 2) {
        uint32_t a = s, b = world;
        while (b) { const uint32_t t = a % b; a = b; b = t; }
        if (a == 1u) return s;
    }
}
// rank's j-th tile slot -> tile coordinates; false: a padding slot (nothing to render)
__host__ __device__ inline bool owned_tile(uint32_t j, uint32_t rank, uint32_t world, uint32_t skew, uint32_t tiles_x, uint32_t tiles_per_row,
                                           uint32_t &tx, uint32_t &ty)
{
    ty = j / tiles_per_row;
    const uint32_t k = j - ty * tiles_per_row;
    tx = (rank + world - ((ty % world) * (skew % world)) % world) % world + k * world; // (32-bit: world <= 64)
    return tx < tiles_x;
}

template <bool LDS>
__device__ __forceinline__ SceneView<LDS> make_view(const DevScene &sc);

template <>
__device__ __forceinline__ SceneView<true> make_view<true>(const DevScene &sc)
{
    SceneView<true> v; // image order: nodes | escape links | primitive records | triangle normals | materials | fallback records | flat leaves | oriented leaves
    v.o_nodes = 0;
    v.o_esc = v.o_nodes + 2u * sc.n_nodes;
    v.o_prims = v.o_esc + (8u * sc.n_nodes + 3u) / 4u;
    v.o_trin = v.o_prims + 4u * sc.n_prims;
    v.o_mats = v.o_trin + 3u * sc.n_tris;
    v.o_fbs = v.o_mats + 4u * sc.n_materials;
    v.o_fbp = v.o_fbs + 4u * sc.n_spheres;
    v.o_flat = v.o_fbp + 4u * sc.n_planes;
    v.pnodes = sc.pnodes;
    v.wnodes = sc.wnodes;
    return v;
}
template <>
__device__ __forceinline__ SceneView<false> make_view<false>(const DevScene &sc)
{
    return SceneView<false>{sc.nodes, sc.prims, sc.tri_normals, sc.materials, sc.fb_spheres, sc.fb_planes, sc.escape, sc.flat_leaves, sc.pnodes, sc.wnodes};
}

__device__ __forceinline__ SceneViewHybrid make_view_hybrid(const DevScene &sc)
{
    const bool wide = sc.lds_hybrid == 3u; // the wide walk's image: a prefix of the wide nodes
    return SceneViewHybrid{0u, 2u * sc.n_nodes, sc.prims, sc.tri_normals, sc.materials, sc.fb_spheres, sc.fb_planes, sc.pnodes, sc.lds_float4s, sc.wnodes, sc.lds_hybrid,
                           wide ? sc.lds_wnodes : 0u};
}

// Copies the scene image into LDS (the arrays are contiguous in one device allocation, in the order
// make_view<true> assumes).
__device__ __forceinline__ void stage_scene_lds(const DevScene &sc)
{
    for (uint32_t i = threadIdx.x; i < sc.lds_float4s; i += blockDim.x) rt_smem[i] = sc.lds_src[i];
    __syncthreads();
}

struct PathState {
    V3 o, d, throughput, light;
    float last_pdf;
    uint32_t rng, bounce, slot; // slot = float index / 3 into the sample buffer
};

// shader.wgsl:1305-1364: seed, jitter, camera ray
__device__ __forceinline__ void start_path(const RenderParams &P, uint32_t px, uint32_t py, uint32_t sample, PathState &s)
{
    uint32_t pixel_index = py * P.width + px;
    uint32_t rng = 0;
    salt_rng(rng, pixel_index);
    salt_rng(rng, sample);
    float angle = random_uniform(rng) * 2.0f * 3.1415926f; // random_in_circle_uniform :627-631
    float cx, cy;
    rt_sincos(angle, cy, cx);
    float rad = rsrt_sqrtf(random_uniform(rng));
    float fx = (float)px + cx * rad, fy = (float)py + cy * rad;
    float sx = ((fx / (float)P.width) * 2.0f - 1.0f) * 1.0f;
    float sy = ((fy / (float)P.height) * 2.0f - 1.0f) * -1.0f;
    float m = rsrt_sinf(P.fov_y / 2.0f);
    float aspect = (float)P.width / (float)P.height;
    V3 rcs = v3(sx * m * aspect, sy * m, -1.0f);
    V3 c0 = v3(P.cam_rot[0], P.cam_rot[1], P.cam_rot[2]), c1 = v3(P.cam_rot[3], P.cam_rot[4], P.cam_rot[5]),
       c2 = v3(P.cam_rot[6], P.cam_rot[7], P.cam_rot[8]);
    s.o = v3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    s.d = normalize(mat3_mul(c0, c1, c2, rcs));
    s.throughput = v3(1, 1, 1);
    s.light = v3(0, 0, 0);
    s.last_pdf = 1.0f;
    s.rng = rng;
    s.bounce = 0;
}

#include "rt_wavepool.h"
// LDS of the 1024-thread walk kernels (hybrid scene view): sixteen waves' pools and beside them the traversal's part of the scene
static constexpr size_t kHybridPoolBytes = (size_t)(1024 / RT_WAVE) * 4u * ((size_t)H_COUNT * RT_WALK_POOL + pool_list_dwords(4));
static constexpr uint32_t kHybridRoomF4 = (uint32_t)((160 * 1024 - kHybridPoolBytes) / sizeof(float4));
// A small scene's whole image goes to LDS while it stays within this (the room beside the flat kernel's sixteen 192-slot pools)
static constexpr size_t kSmallImageBytes = 24 * 1024;
// ... and of the cooperative walk's kernel (TRAV 6): 128-slot pools with their two work stacks
#ifndef RT_COOP_POOL
#define RT_COOP_POOL 128u // (build-time A/B: -DRT_COOP_POOL=96u with RSRT_WPS=5 fits a fifth wave per SIMD beside 256-thread workgroups)
#endif
#ifndef RT_COOP_BLOCK
#define RT_COOP_BLOCK 1024 // threads of the one workgroup a CU holds beside the staged node prefix
#endif
static constexpr uint32_t kCoopRoomF4 = (uint32_t)((160 * 1024 - (size_t)(RT_COOP_BLOCK / RT_WAVE) * 4u * pool_wave_lds_dwords(6, RT_COOP_POOL)) / sizeof(float4));
#include "rt_alias_device.h"
#include "rt_bvh_device.h"
#include "rt_scene_image.h" // (host only: the scene's device image, from the constants of the headers above)

// total = textureLoad(cumulative) + sample, once per sample in order (shader.wgsl:1367-1371)
__global__ __launch_bounds__(RT_BLOCK) void rt_resolve_kernel(RenderParams P, float4 *accum)
{
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= P.n_slots) return;
    uint32_t tile_px = P.tile_w * P.tile_h;
    uint32_t j = slot / tile_px, p = slot % tile_px;
    uint32_t ttx, tty;
    if (!owned_tile(j, P.rank, P.world, P.skew, P.tiles_x, P.tiles_per_row, ttx, tty)) return;
    uint32_t px = ttx * P.tile_w + p % P.tile_w, py = tty * P.tile_h + p / P.tile_w;
    if (px >= P.width || py >= P.height) return;
    float4 a = accum[(size_t)py * P.width + px];
    const float *src = P.sample_buf + (size_t)slot * 3u;
    const size_t step = (size_t)P.n_slots * 3u;
    for (uint32_t k = 0; k < P.sample_count; k++, src += step) {
        const rt_f3v v = __builtin_nontemporal_load(reinterpret_cast<const rt_f3v_a4 *>(src)); // read once, never again
        a.x = a.x + v.x;
        a.y = a.y + v.y;
        a.z = a.z + v.z;
    }
    a.w = 1.0f;
    accum[(size_t)py * P.width + px] = a;
}

// The ray-query probe.  SV / TRAV as in rt_render_pool_kernel (where the scene is read from, which traversal
// runs); TRAV == 4 is the per-lane stack walk (trace_bvh).  mode bit 0: cast_ray_bvh only (no brute-force fallback).
template <int SV, int TRAV>
__global__ __launch_bounds__(RT_BLOCK) void rt_cast_rays_kernel(DevScene sc, uint32_t n, const float *origins, const float *dirs,
                                                                uint32_t mode, uint32_t flags, uint32_t repeat, rsrt_hit *out)
{
    if (SV != 0) stage_scene_lds(sc);
    const typename PoolView<SV>::type S = PoolView<SV>::make(sc);
    uint32_t *stack = reinterpret_cast<uint32_t *>(rt_smem + sc.lds_float4s) + threadIdx.x;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    V3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    const bool prune = (flags & RSRT_FLAG_PRUNE) != 0;
    Hit h;
    h.t = RT_INFINITY; h.ref = 0; h.src = SRC_BVH; h.u = h.v = 0.0f;
    if (TRAV == 4) { // the per-lane stack traversal
        trace_bvh<false>(S, o, d, prune, stack, RT_BLOCK, h);
    } else { // what the production kernel's TRACE stage runs, resumed until done as the scheduler would
#ifdef RT_INSTRUMENT
        DbgCounters dbg;
#endif
        uint32_t cur = 0, work = 0;
        unsigned long long flat_rem = 0ull;
        uint32_t wmem[RT_WSTATE_WORDS]; // (the wide walk parks its stack here between calls, as the pool kernel does in the slot's cold columns)
        constexpr int T = TRAV; // (probe numbering: 4 is the per-lane stack walk, handled above; 5 the wide walk — the form whose stack may overflow, which takes any tree)
        while (cur != RT_END) trace_dispatch<T>(DBG_ARG S, sc, o, d, prune, false, T >= 4 ? 2u : 12u, 50u, cur, h, nullptr, work, flat_rem, wmem, 1u, 60u);
        // RSRT_PROBE_REPEAT (tools/trace_rate.py): the same query again and again, so that a timing of this kernel is a timing
        // of the traversal and not of staging the scene for 256 rays; the result does not change
        for (uint32_t k = 1; k < repeat; k++) {
            asm volatile("" : "+v"(o.x), "+v"(d.x));
            Hit h2;
            h2.t = RT_INFINITY; h2.ref = 0; h2.src = SRC_BVH; h2.u = h2.v = 0.0f;
            cur = 0;
            while (cur != RT_END) trace_dispatch<T>(DBG_ARG S, sc, o, d, prune, false, T >= 4 ? 2u : 12u, 50u, cur, h2, nullptr, work, flat_rem, wmem, 1u, 60u);
            h.t = h2.t; h.ref = h2.ref; h.src = h2.src;
        }
        if (h.did_hit()) hit_barycentrics(S, h, o, d); // as SHADE does: the traversals do not carry u, v
    }
    if ((mode & 1u) == 0 && !h.did_hit()) { // cast_ray's brute-force fallback (the MISS stage)
        for (uint32_t k = 0; k < sc.n_spheres; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_SPHERE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_SPHERE; }
        }
        for (uint32_t k = 0; k < sc.n_planes; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_PLANE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_PLANE; }
        }
    }
    rsrt_hit r;
    memset(&r, 0, sizeof r);
    if (h.did_hit()) {
        Surface s = resolve_hit(S, h, o, d);
        r.did_hit = 1;
        r.distance = h.t;
        r.hit_point[0] = s.point.x; r.hit_point[1] = s.point.y; r.hit_point[2] = s.point.z;
        r.normal[0] = s.normal.x; r.normal[1] = s.normal.y; r.normal[2] = s.normal.z;
        r.material_id = s.material_id;
    } else if ((mode & 1u) == 0) {
        r.distance = RT_INFINITY; // cast_ray returns its `result` initialiser on a total miss (shader.wgsl:568-574, :600)
    }
    out[i] = r;
}

// The ray-query probe of the cooperative walk (TRAV 6, rt_coop.h): a wave takes 64 rays into a one-column "pool" of its own (slot = lane) and runs
// the very functions the production kernel's TRACE stage runs — coop_push_rays, coop_trace, coop_slow_rays.  gstack: RT_COOP_GCAP dwords a wave.
template <int SV>
__global__ __launch_bounds__(RT_BLOCK) void rt_cast_rays_coop_kernel(DevScene sc, uint32_t n, const float *origins, const float *dirs,
                                                                     uint32_t mode, uint32_t flags, uint32_t repeat, rsrt_hit *out, uint32_t *gstack,
                                                                     uint32_t lds_cap, uint32_t lifo_at, uint32_t narrow_at, uint32_t gcap,
                                                                     unsigned long long *stats)
{
    if (SV != 0) stage_scene_lds(sc);
    const typename PoolView<SV>::type S = PoolView<SV>::make(sc);
    constexpr uint32_t kPool = 64u;
    typedef CoopCols<kPool> C;
    const uint32_t lane = threadIdx.x & (RT_WAVE - 1u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / RT_WAVE));
    uint32_t *const W = reinterpret_cast<uint32_t *>(rt_smem + sc.lds_float4s) + wave * pool_wave_lds_dwords(6, kPool);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    const V3 o = valid ? v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]) : v3(0.0f, 0.0f, 0.0f);
    const V3 d = valid ? v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]) : v3(0.0f, 0.0f, 1.0f);
#ifdef RT_INSTRUMENT
    DbgCounters dbg;
#endif
    Hit h;
    h.t = RT_INFINITY; h.ref = 0; h.src = SRC_BVH; h.u = h.v = 0.0f;
    uint32_t work = 0;
    CoopCount cc;
    cc.zero();
    for (uint32_t k = 0; k < repeat; k++) { // (RSRT_PROBE_REPEAT: the same queries again; the result does not change)
        W[C::O + lane] = as_u(o.x); W[C::O + kPool + lane] = as_u(o.y); W[C::O + 2u * kPool + lane] = as_u(o.z);
        W[C::E + lane] = as_u(d.x); W[C::E + kPool + lane] = as_u(d.y); W[C::E + 2u * kPool + lane] = as_u(d.z);
        W[C::S + lane] = 0u; W[C::S + kPool + lane] = 0u; W[C::S + 2u * kPool + lane] = 0u;
        W[C::CT + lane] = (uint32_t)F_EXT | (uint32_t)TAG_TRACE;
        RT_WAVE_HANDOVER();
        CoopStacks cs;
        cs.ls = W + C::DWORDS; cs.ns = cs.ls + RT_COOP_LCAP; cs.map = reinterpret_cast<uint16_t *>(cs.ns + RT_COOP_NCAP);
        cs.gs = gstack + (size_t)(blockIdx.x * (RT_BLOCK / RT_WAVE) + wave) * RT_COOP_GCAP;
        cs.ns_h = cs.ns_n = cs.ls_n = cs.gs_n = 0u;
        cs.lds_cap = lds_cap; cs.lifo_at = lifo_at; cs.narrow_at = narrow_at; cs.gcap = gcap;
        coop_push_rays<kPool>(W, cs, cc, valid, lane, W[C::CT + lane], (uint32_t)F_EXT, (uint32_t)F_SHADOW);
        coop_trace<kPool>(DBG_ARG S, W, cs, cc, false, lane, work);
        RT_WAVE_HANDOVER();
        if (cs.overflowed() && valid) coop_abandon<kPool>(W, lane, (uint32_t)F_EXT, (uint32_t)F_SHADOW);
        const bool mine[1] = {valid};
        const uint32_t slots[1] = {lane};
        coop_slow_rays<kPool, 1u>(DBG_ARG S, sc, W, mine, slots, false, work);
        h.t = as_f(W[C::BEST + 2u * lane + 1u]);
        h.ref = W[C::BEST + 2u * lane];
        RT_WAVE_HANDOVER();
    }
    cc.flush(stats, lane);
    if (!valid) return; // (nothing wave-wide from here on)
    if (h.did_hit()) hit_barycentrics(S, h, o, d); // as SHADE does: the traversals do not carry u, v
    if ((mode & 1u) == 0 && !h.did_hit()) { // cast_ray's brute-force fallback (the MISS stage)
        for (uint32_t k = 0; k < sc.n_spheres; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_SPHERE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_SPHERE; }
        }
        for (uint32_t k = 0; k < sc.n_planes; k++) {
            float u, v;
            float t = test_record(S, k, SRC_FB_PLANE, o, d, u, v);
            if (t >= 0.0f && t < h.t) { h.t = t; h.ref = k; h.src = SRC_FB_PLANE; }
        }
    }
    rsrt_hit r;
    memset(&r, 0, sizeof r);
    if (h.did_hit()) {
        Surface s = resolve_hit(S, h, o, d);
        r.did_hit = 1;
        r.distance = h.t;
        r.hit_point[0] = s.point.x; r.hit_point[1] = s.point.y; r.hit_point[2] = s.point.z;
        r.normal[0] = s.normal.x; r.normal[1] = s.normal.y; r.normal[2] = s.normal.z;
        r.material_id = s.material_id;
    } else if ((mode & 1u) == 0) {
        r.distance = RT_INFINITY; // cast_ray returns its `result` initialiser on a total miss (shader.wgsl:568-574, :600)
    }
    out[i] = r;
}

__global__ void rt_mean_f16_kernel(const float4 *accum, size_t n, float inv_is_unused, uint32_t sample_total, ushort4 *out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 a = accum[i];
    float cnt = (float)sample_total; // total_light / f32(sample_count + 1), shader.wgsl:1369
    __half hx = __float2half_rn(a.x / cnt), hy = __float2half_rn(a.y / cnt), hz = __float2half_rn(a.z / cnt), hw = __float2half_rn(1.0f);
    out[i] = make_ushort4(__half_as_ushort(hx), __half_as_ushort(hy), __half_as_ushort(hz), __half_as_ushort(hw));
}

// The reference's developer views (shader.wgsl:1314-1338: what `main` writes to out_texture instead of a render when dev_index is 2 or 3).
// View 3 ("display HDRI", :1333-1338): out[x, y] = saturate(environment texel (x, y)), alpha 0; a pixel outside the map reads zeros.
__global__ void rt_dev_view_hdri_kernel(const float4 *env_rgba, uint32_t env_w, uint32_t env_h, uint32_t width, uint32_t height, ushort4 *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const uint32_t x = (uint32_t)(i % width), y = (uint32_t)(i / width);
    float3 c = make_float3(0.0f, 0.0f, 0.0f);
    if (x < env_w && y < env_h) { const float4 t = env_rgba[(size_t)y * env_w + x]; c = make_float3(t.x, t.y, t.z); } // (the texel's alpha is the device's own: not looked at)
    auto sat = [](float v) { return __builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f); };
    out[i] = make_ushort4(__half_as_ushort(__float2half_rn(sat(c.x))), __half_as_ushort(__float2half_rn(sat(c.y))), __half_as_ushort(__float2half_rn(sat(c.z))), __half_as_ushort(__float2half_rn(0.0f)));
}
// View 2 ("draw pixels based on distribution", :1314-1332): every pixel draws 20 indices from the environment's alias table, seeded as a
// render's pixel is (:1309-1312), and adds 0.1 / 20 to THAT texel's position of out_texture.  In the shader the invocations read-modify-write
// the binary16 texture unordered — which draws survive a frame depends on the GPU's scheduling; this is the frame in which every draw
// lands: first the draws are counted per texel (integer atomics), then each texel takes its count of `v <- f16(f32(v) + 0.1 / 20)` steps
// (equal addends: the order of the draws cannot matter), stopping early once a step no longer changes it.
__global__ void rt_dev_view_count_kernel(const uint4 *alias, uint32_t env_w, uint32_t env_h, uint32_t width, uint32_t height, uint32_t sample_count, uint32_t *counts)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)width * height) return;
    uint32_t rng = 0;
    salt_rng(rng, (uint32_t)i);      // pixel_index = y * resolution.x + x
    salt_rng(rng, sample_count);
    const uint32_t length = env_w * env_h;
    for (uint32_t k = 0; k < 20u; k++) { // random_index_in_environment, :689-706
        const uint32_t index = min(f2u(random_uniform(rng) * (float)length), length - 1u);
        const uint4 entry = alias[index];
        const uint32_t pick = random_uniform(rng) < as_f(entry.x) ? index : entry.y;
        const uint32_t x = pick % env_w, y = pick / env_w;
        if (x < width && y < height) atomicAdd(&counts[(size_t)y * width + x], 1u); // (a store outside the texture is dropped)
    }
}
__global__ void rt_dev_view_apply_kernel(const uint32_t *counts, size_t n, ushort4 *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = counts[i];
    if (c == 0u) return;
    const float step = 0.1f / 20.0f; // vec3(0.1, 0.1, 0.1) / f32(count)
    ushort4 v = out[i];
    unsigned short *ch[3] = {&v.x, &v.y, &v.z};
    for (int k = 0; k < 3; k++) {
        unsigned short h = *ch[k];
        for (uint32_t j = 0; j < c; j++) {
            const unsigned short nx = __half_as_ushort(__float2half_rn(__half2float(__ushort_as_half(h)) + step));
            if (nx == h) break; // (a fixed point: the remaining steps change nothing)
            h = nx;
        }
        *ch[k] = h;
    }
    v.w = __half_as_ushort(__float2half_rn(0.0f)); // textureStore(out_texture, .., vec4(color, 0.))
    out[i] = v;
}

// hdr.wgsl fs_main + the *Srgb surface write: mean (through binary16) -> ACES -> sRGB 8-bit
__global__ void rt_display_kernel(const float4 *accum, size_t n, uint32_t sample_total, uchar4 *out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    const float sum[3] = {a.x, a.y, a.z};
    unsigned char rgb[3];
    rsrt_display_pixel(sum, (float)sample_total, rgb);
    out[i] = make_uchar4(rgb[0], rgb[1], rgb[2], 255);
}

// =================================================================== host side
namespace {

thread_local std::string g_create_error;

struct Env {
    float4 *rgba = nullptr;
    uint4 *alias = nullptr;
    uint32_t width = 0, height = 0;
};

} // namespace

// Render kernel forms.  For a scene whose whole image fits LDS the default form is ONE 1024-thread workgroup per CU — one scene copy
// instead of four, which is what makes room for 192 slots per wave (-0.8 % on the BASELINE frame); the SMALL form, which pipelined
// small jobs run (and RSRT_KERNEL=2 forces), has 160 slots per wave in 256-thread workgroups, each with its own LDS copy of the
// scene (four workgroups per CU fit in LDS).  Other scene views have one form.
template <int SV, uint32_t BLOCK, uint32_t POOL>
static const void *pool_function(int trav)
{
    switch (trav) {
    case 0: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 0>);
    case 1: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 1>);
    case 3: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 3>);
    case 4: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 4>);
    case 5: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 5>);
    default: return reinterpret_cast<const void *>(&rt_render_pool_kernel<SV, BLOCK, POOL, 2>);
    }
}
// sv: 0 scene in global memory, 1 whole image in LDS, 2 hybrid (nodes + escape links in LDS, 1024-thread workgroups)
static const void *variant_function(bool small, int sv, int trav)
{
    if (trav == 6) // the cooperative walk: 128-slot pools; one 1024-thread workgroup per CU beside the staged node prefix, else 256-thread workgroups
        return sv == 2 ? reinterpret_cast<const void *>(&rt_render_pool_kernel<2, RT_COOP_BLOCK, RT_COOP_POOL, 6>)
                       : (sv == 1 ? reinterpret_cast<const void *>(&rt_render_pool_kernel<1, RT_BLOCK, RT_COOP_POOL, 6>) : reinterpret_cast<const void *>(&rt_render_pool_kernel<0, RT_BLOCK, RT_COOP_POOL, 6>));
    if (sv == 2) return pool_function<2, 1024, RT_WALK_POOL>(trav == 2 ? 1 : trav); // (the flat loop needs the whole image: never asked for here)
    if (sv == 1) return small ? pool_function<1, RT_BLOCK, 160>(trav) : pool_function<1, 1024, RT_BIG_POOL>(trav);
    return pool_function<0, RT_BLOCK, 160>(trav);
}

template <int SV>
static const void *probe_function_sv(int trav)
{
    switch (trav) {
    case 0: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, 0>);
    case 1: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, 1>);
    case 2: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, (SV == 2 ? 1 : 2)>); // (flat needs the whole image: never asked for with SV 2)
    case 3: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, 3>);
    case 5: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, 5>);
    case 6: return reinterpret_cast<const void *>(&rt_cast_rays_coop_kernel<SV>);
    default: return reinterpret_cast<const void *>(&rt_cast_rays_kernel<SV, 4>);
    }
}
static const void *probe_function(int sv, int trav)
{
    return sv == 0 ? probe_function_sv<0>(trav) : (sv == 1 ? probe_function_sv<1>(trav) : probe_function_sv<2>(trav));
}

// Scheduling of the render passes (see rsrt_context::Lane)
static constexpr uint32_t kLanes = 4;               // sets of work buffers, each with its own stream
static constexpr uint64_t kSmallPaths = 4ull << 20; // a call of at most this many paths is a small job
static constexpr int kPipeBlocks = 1;               // workgroups per CU of a pipelined small job (four such jobs fill a CU)
static constexpr uint32_t kChunksPerWave = 32;      // work chunks a resident wave should get at least: sets samples per chunk, and sub-tiles for small jobs
static constexpr uint32_t kDescendQuorum = 30;      // fixed-order / wide walk: a descending round ends once fewer than this percentage of its lanes are still descending
static constexpr uint32_t kStopQuorum = 40;         // wide walk: a TRACE call ends (the unfinished rays park their stacks) once fewer than this percentage of its lanes are still walking

// ------------------------------------------------------------------ image buffers (their helpers: "image buffers" below)
// A pixel buffer the caller may bind memory of its own to: `p` is the one in use, `owned` the library's (none while a caller's is bound).
struct PixelBuffer {
    const char *name, *pointer_name; // in error texts: "bound AOV buffer is ...", "AOV pointer must be ..."
    uint32_t f4;                     // float4 a pixel
    float4 *p = nullptr, *owned = nullptr;
    uint32_t w = 0, h = 0;
    bool is(uint32_t W, uint32_t H) const { return p && w == W && h == H; }
    size_t pixels() const { return (size_t)w * h; }
    size_t bytes() const { return pixels() * f4 * sizeof(float4); }
};
// A library-owned allocation that follows a size.
struct SizedAlloc {
    void *p = nullptr;
    uint32_t w = 0, h = 0;
    bool is(uint32_t W, uint32_t H) const { return p && w == W && h == H; }
    size_t pixels() const { return (size_t)w * h; }
};
// A histogram meter (rt_exposure.h): two histograms in one allocation (a call adds into the zero one and zeroes the other for the next),
// which of them holds the last call's, whether there was one since the last reset, and whether a failed launch left them unknown.
struct HistMeter {
    uint32_t *hist = nullptr;
    uint32_t cur = 0;
    bool have = false, dirty = false;
};
// An image one of the passes can read: sums of `total` samples a pixel (1: a colour).
struct ImageView {
    const float4 *img = nullptr;
    uint32_t w = 0, h = 0;
    float total = 1.0f;
    size_t pixels() const { return (size_t)w * h; }
};
enum ImageSource : uint32_t { IMAGE_MEAN = 0, IMAGE_DENOISED = 1, IMAGE_TEMPORAL = 2, IMAGE_UPSAMPLED = 3, IMAGE_LENS = 4, IMAGE_MOTION = 5, IMAGE_FOG = 6 }; // (= RSRT_EXPOSURE_*, include/rsrt.h)

struct rsrt_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::string error;
    std::string description;
    int cus = 0;
    // scene
    float4 *scene_blob = nullptr;
    DevScene scene{};
    bool scene_ready = false;
    uint32_t hybrid_head_f4 = 0, hybrid_pnode_f4 = 0; // mid-size scenes: float4s of nodes + escape links / of the pre-order nodes' top block (0 = none)
    // ... and the wide walks' LDS image: a prefix of the wimg_nodes wide nodes, as long as the launch has room for (0 = no image)
    uint32_t wimg_nodes = 0;
    // environments
    std::vector<Env> envs;
    // partition
    uint32_t rank = 0, world = 1, tile_w = 16, tile_h = 16;
    // accumulator (1 float4 a pixel).  A change of its size drops what was derived from it: accumulator_size_changed()
    PixelBuffer acc{"accumulator", "accumulator", 1u};
    // work buffers
    // kLanes sets of work buffers ("lanes"), used in turn by successive passes: a pass's path-tracing kernel runs on its lane's own
    // stream and touches nothing but its lane's buffers, so the kernel of call k + 1 fills the CUs that call k's tail is leaving
    // (a launch ends with ~0.5 ms of pipeline drain: at one sample per call — the reference's interactive mode, src/state.rs:
    // 760-833 — that was half the frame time).  Only the small resolve kernels, which add into the accumulator in sample
    // order, stay chained one behind the other (enqueue_pass).
    struct Lane {
        hipStream_t stream = nullptr;
        unsigned int *work_counter = nullptr;
        float *sample_buf = nullptr;
        size_t sample_buf_bytes = 0;
        uint32_t *cold_state = nullptr;
        size_t cold_bytes = 0;
        hipEvent_t resolved = nullptr; // recorded after the resolve that read this lane's sample buffer last
        bool resolved_valid = false;
        hipEvent_t traced = nullptr;   // recorded after this lane's last path-tracing kernel (asked, not waited for: is the GPU busy?)
        bool traced_valid = false;
        hipEvent_t caller_at = nullptr; // where the caller's stream stood when this lane's last pass was enqueued
    };
    // Ordinary jobs use lane 0.  SMALL jobs (at most kSmallPaths paths a call: the reference's one sample per
    // frame) that arrive while an earlier kernel is still running are PIPELINED: they take turns over all kLanes lanes and run the
    // small form of the kernel with kPipeBlocks workgroups per CU, so that up to four calls are resident side by side and one call's
    // ~0.5 ms of pipeline fill and drain is covered by its neighbours' steady state (a call alone on the GPU keeps the full grid:
    // its latency is what counts then).
    Lane lanes[kLanes];
    uint32_t next_small_lane = 1;
    unsigned long long *dev_stats = nullptr;
    // stats
    rsrt_stats stats{};
    struct PassEvents { hipEvent_t begin, traced, end; };
    std::vector<PassEvents> pending_events;
    double cum_trace_ms = 0, cum_resolve_ms = 0, base_trace_ms = 0, base_resolve_ms = 0;
    unsigned long long base_counts[4] = {0, 0, 0, 0};
    uint32_t cum_launches = 0, base_launches = 0;
    std::vector<hipEvent_t> event_pool;
    // Work buffers (work_counter, sample_buf, cold_state, scratch) and the accumulator are per-context
    // singletons, so everything the context enqueues is ONE chain whatever streams the caller passes:
    // `last_event` is recorded after every enqueue, and an enqueue on a different stream first waits for it.
    hipEvent_t last_event = nullptr;
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    // multi-GPU (rsrt_comm.h): this context's RCCL communicator (an ncclComm_t), NULL in a world of one
    void *comm = nullptr;
    bool comm_owned = false;
    bool comm_dense_mode = false; // RSRT_COMM_MODE=reduce / rsrt_comm_set_mode: the exchange is a dense ncclReduce instead of the gather of compact tile buffers
    uint32_t comm_rank = 0, comm_world = 1;
    struct ReduceEvents { hipEvent_t begin, end; };
    std::vector<ReduceEvents> pending_reduce;
    double cum_reduce_ms = 0, base_reduce_ms = 0;
    uint32_t cum_reduces = 0;
    void *comm_buf = nullptr; // compact tile buffers of the exchange step (rsrt_comm.h): one per rank on the root, one elsewhere
    size_t comm_buf_bytes = 0;
    // scratch for rsrt_resolve_mean_f16 / rsrt_display_srgb8 (grow-only; no per-frame hipMalloc)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    int blocks_per_cu[21] = {}; // [scene view * 7 + traversal], of the form small_form selects (a pipelined job has kPipeBlocks)
    bool small_form = false; // RSRT_KERNEL=2: every job runs the small form (tests reach it this way)
    int max_traversal = 6; // most specialised traversal to use where the scene allows it (rt_wavepool.h, TRAV)
    uint32_t coop_lds_cap = RT_COOP_NCAP, coop_lifo_at = RT_COOP_LIFO_AT, coop_narrow_at = RT_COOP_NARROW_AT; // RSRT_COOP_LDS_CAP / _LIFO_AT / _NARROW_AT (tests: force the node queue's spill / newest-first / one-item trips)
    uint32_t coop_gcap = RT_COOP_GCAP; // RSRT_COOP_GCAP (tests: a small arena block forces the overflow guard, rt_coop.h coop_overflow)
    bool allow_flat = true;
    bool flat_oriented = true; // RSRT_FLAT_ORIENTED=0: the flat loop orders each box's slab values itself instead of reading octant tables (A/B)
    bool allow_hybrid = true;
    uint32_t trace_budget = 0; // traversal steps per TRACE invocation before a ray is re-queued (0: 6 for the fixed-order walk, 12 for the tree walks)
    uint32_t flat_quorum = 20; // flat traversal: the triangle loop ends once fewer than this percentage of its lanes still hold triangles (0: never)
    // (every RSRT_* environment knob is read ONCE, in rsrt_context_create)
    size_t sample_buffer_budget = 16ull << 30; // RSRT_SAMPLE_BUFFER_MB: bytes of sample buffer per pass
    uint32_t probe_repeat = 1; // RSRT_PROBE_REPEAT: rsrt_cast_rays runs every query this many times (tools/trace_rate.py)
    // Pipelined small jobs want four kernels of one context resident at a time, each from a stream of its own; the HIP runtime maps a
    // process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams that share one run one after the other —
    // measured: 0.85 against 0.63 ms per single-sample call.  The HOST sets that variable, before its first HIP call; the
    // library only looks at it, and says so once when it pipelines over fewer queues than it has lanes.
    int hw_queues = 4;
    bool hw_queue_warned = false;
    unsigned long long debug_words[32] = {0};
    // The image-space passes' buffers (DESIGN.md §1 has the table: owner, size followed, what drops each).
    // denoiser (rt_denoise.h): the AOV records (2 float4 a pixel, of the accumulator's size), the filter's scratch and where the last
    // rsrt_denoise wrote
    PixelBuffer aov{"AOV buffer", "AOV", 2u};
    SizedAlloc dn_scratch;
    float4 *dn_last = nullptr;
    // temporal pass (rt_temporal.h): two history and two feature buffers (float4 each), which history holds the last frame, how many frames
    // ran since the last reset (0: the next one is a first frame) and the last camera
    SizedAlloc tp_hist;
    uint32_t tp_cur = 0, tp_frames = 0;
    float tp_cam[13] = {0}; // pos, rot (column-major 3x3), fov_y
    // the luminance moments (RSRT_TEMPORAL_MOMENTS): two float4 record buffers (allocated on the first MOMENTS frame) and whether the
    // last frame carried them
    SizedAlloc tp_mom;
    uint32_t tp_moments = 0;
    // guided upsampling (rt_upsample.h): the guide records of the output size (2 float4 a pixel; independent of the accumulator's size),
    // the low pass's scratch (float4 + ushort4 a low pixel), the library-owned output and where the last rsrt_upsample wrote
    PixelBuffer guide{"guide buffer", "guide", 2u};
    SizedAlloc up_scratch, up_out;
    ImageView up_last;
    // noise estimate (rt_noise.h): the snapshot of the accumulator, how many samples it holds (0: none), the tile map of the last
    // rsrt_noise_estimate (grow-only), its shape and threshold and whether there was one since the last reset
    SizedAlloc ns_snap;
    uint32_t ns_total = 0;
    float *ns_tiles = nullptr;
    size_t ns_tiles_cap = 0;
    uint32_t ns_tx = 0, ns_ty = 0;
    float ns_threshold = 0.0f;
    bool ns_have = false;
    // auto-exposure (rt_exposure.h): the luminance histograms of rsrt_exposure_meter.  The library keeps no exposure.
    HistMeter ex;
    // bloom (rt_bloom.h): the pyramid of the last rsrt_bloom — B, then D_1 .. D_8 — which follows the size of the source B was built
    // for, and whether there was one since the last reset
    SizedAlloc bl_pyr;
    bool bl_have = false;
    // local exposure (rt_local.h): the raw and the blurred bilateral grid of the last rsrt_local_exposure, one allocation that follows
    // the size of the source the grid was built for and has room for the smallest cell; the cell, and whether there was a grid since
    // the last reset.  The library keeps no exposure and no strengths.
    SizedAlloc lc_grid;
    uint32_t lc_cell = 0;
    bool lc_have = false;
    // depth of field (rt_dof.h): the prepared texels of the last rsrt_dof and, behind them, the library-owned lens image (a float4 a pixel
    // each), one allocation that follows the size of the source the lens image was built from; and where the last rsrt_dof wrote (img
    // NULL: no lens image since the last reset)
    SizedAlloc df_buf;
    ImageView df_last;
    const PixelBuffer *df_rec = nullptr; // the records the lens image was built from (the AOV buffer or the guide): rsrt_motion_blur of it reads them
    // camera motion blur (rt_motion.h): the prepared texels of the last rsrt_motion_blur (colour and l, z, u) and the library-owned motion
    // image, one allocation that follows the size of the source the motion image was built from; the tiles' maxima, which follow the tile
    // counts; and where the last rsrt_motion_blur wrote (img NULL: no motion image since the last reset).  The library keeps no camera.
    SizedAlloc mt_buf, mt_tiles;
    ImageView mt_last;
    // volumetric fog (rt_fog.h): the fog records (1 float4 a pixel: inscatter sum rgb, transmittance sum; a size of their own, like the
    // guide's), the library-owned fog image, which follows the size of the source it was built from, where the last rsrt_fog_apply wrote
    // (img NULL: no fog image since the last reset) and the first-hit records of that source: rsrt_dof and rsrt_motion_blur of it read them;
    // the rebuild's scratch (rsrt_fog_apply_upsampled: a float4 a LOW pixel, follows the records' size)
    PixelBuffer fog{"fog records", "fog", 1u};
    SizedAlloc fg_out, fg_src;
    ImageView fg_last;
    const PixelBuffer *fg_rec = nullptr;
    // white balance and colour grading (rt_colour.h): the chroma histograms of rsrt_white_meter and the colour LUT (cl_cap float4 nodes
    // of room; cl_n the LUT's size, 0: none).  Neither follows the accumulator's size: accumulator_size_changed() leaves them.  The
    // library keeps no white point.
    HistMeter wb;
    float4 *cl_lut = nullptr;
    size_t cl_cap = 0;
    uint32_t cl_n = 0;
};

namespace {

rsrt_status fail(rsrt_context *ctx, rsrt_status st, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->error = buf;
    else g_create_error = buf;
    return st;
}

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RSRT_ERR_OUT_OF_MEMORY : RSRT_ERR_HIP, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                              \
    } while (0)

struct DeviceGuard {
    explicit DeviceGuard(int dev) { (void)hipSetDevice(dev); }
};

// Orders `stream` after everything this context has enqueued so far (no-op on the same stream).
rsrt_status begin_work(rsrt_context *ctx, hipStream_t stream)
{
    if (ctx->last_valid && ctx->last_stream != stream) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->last_event, 0));
    return RSRT_OK;
}
// Marks the end of what was just enqueued on `stream`.
rsrt_status end_work(rsrt_context *ctx, hipStream_t stream)
{
    HIP_TRY(ctx, hipEventRecord(ctx->last_event, stream));
    ctx->last_stream = stream;
    ctx->last_valid = true;
    return RSRT_OK;
}
// Waits for everything the context has enqueued, on whatever stream.
rsrt_status sync_all(rsrt_context *ctx)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &L : ctx->lanes)
        if (L.stream) HIP_TRY(ctx, hipStreamSynchronize(L.stream));
    if (ctx->last_valid) HIP_TRY(ctx, hipEventSynchronize(ctx->last_event));
    return RSRT_OK;
}
rsrt_status ensure_scratch(rsrt_context *ctx, size_t bytes)
{
    if (bytes <= ctx->scratch_bytes) return RSRT_OK;
    rsrt_status st = sync_all(ctx);
    if (st) return st;
    if (ctx->scratch) { (void)hipFree(ctx->scratch); ctx->scratch = nullptr; ctx->scratch_bytes = 0; }
    HIP_TRY(ctx, hipMalloc(&ctx->scratch, bytes));
    ctx->scratch_bytes = bytes;
    return RSRT_OK;
}

// ------------------------------------------------------------------ image buffers
// What the image-space passes (rt_denoise.h, rt_temporal.h, rt_upsample.h, rt_noise.h, rt_exposure.h, rt_bloom.h, rt_local.h, rt_dof.h, rt_colour.h, rt_motion.h, rt_fog.h) share on the host: the buffers a
// caller may bind, the library's allocations that follow a size, which image a call means, and the way results reach the host.
// `what` is the calling entry point's name as its error texts spell it.

hipStream_t stream_of(rsrt_context *ctx, void *hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream; }

rsrt_status whole_frame(rsrt_context *ctx, const char *what)
{
    if (ctx->world != 1) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: whole frame only (partition of %u ranks)", what, ctx->world);
    return RSRT_OK;
}

void release(SizedAlloc &a)
{
    (void)hipFree(a.p);
    a = SizedAlloc{};
}
// a.p: bytes_per_pixel for each of w x h pixels, not initialised.  A new allocation waits for everything in flight first.
rsrt_status ensure_sized(rsrt_context *ctx, SizedAlloc &a, uint32_t w, uint32_t h, size_t bytes_per_pixel)
{
    if (a.is(w, h)) return RSRT_OK;
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    release(a);
    HIP_TRY(ctx, hipMalloc(&a.p, (size_t)w * h * bytes_per_pixel));
    a.w = w;
    a.h = h;
    return RSRT_OK;
}

// b is w x h: the bound buffer if it has that size, else the library's own, allocated zeroed
rsrt_status buffer_ensure(rsrt_context *ctx, PixelBuffer &b, uint32_t w, uint32_t h)
{
    if (b.is(w, h)) return RSRT_OK;
    if (b.p && b.p != b.owned) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bound %s is %ux%u but %ux%u was requested", b.name, b.w, b.h, w, h);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    (void)hipFree(b.owned);
    b.owned = b.p = nullptr;
    b.w = b.h = 0;
    const size_t bytes = (size_t)w * h * b.f4 * sizeof(float4);
    HIP_TRY(ctx, hipMalloc(&b.owned, bytes));
    // (on the context's stream, and finished before any pass can write the buffer: a plain hipMemset goes to the null stream, which the
    // context's non-blocking streams are not ordered against, and could land on top of the first pass)
    HIP_TRY(ctx, hipMemsetAsync(b.owned, 0, bytes, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    b.p = b.owned;
    b.w = w;
    b.h = h;
    return RSRT_OK;
}
// The caller's memory instead of the library's, which is given up; NULL: back to the library's (there is none after a bind)
rsrt_status buffer_bind(rsrt_context *ctx, PixelBuffer &b, void *device, uint32_t w, uint32_t h)
{
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (!device) {
        b.p = b.owned;
        if (!b.p) b.w = b.h = 0;
        return RSRT_OK;
    }
    if (w == 0 || h == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", w, h);
    if ((uintptr_t)device % 16) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s pointer must be 16-byte aligned", b.pointer_name);
    (void)hipFree(b.owned);
    b.owned = nullptr;
    b.p = static_cast<float4 *>(device);
    b.w = w;
    b.h = h;
    return RSRT_OK;
}
rsrt_status buffer_clear(rsrt_context *ctx, PixelBuffer &b)
{
    if (!b.p) return fail(ctx, RSRT_ERR_NOT_READY, "no %s", b.name);
    rsrt_status st = begin_work(ctx, ctx->stream);
    if (st) return st;
    HIP_TRY(ctx, hipMemsetAsync(b.p, 0, b.bytes(), ctx->stream));
    return end_work(ctx, ctx->stream);
}

// `want` floats at src -> host, after everything in flight
rsrt_status download_floats(rsrt_context *ctx, const char *what, const void *src, size_t want, float *host, size_t n_floats)
{
    if (!host || n_floats != want) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: expected %zu floats", what, want);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    HIP_TRY(ctx, hipMemcpy(host, src, want * sizeof(float), hipMemcpyDeviceToHost));
    return RSRT_OK;
}
rsrt_status buffer_download(rsrt_context *ctx, const char *what, const PixelBuffer &b, float *host, size_t n_floats)
{
    if (!b.p) return fail(ctx, RSRT_ERR_NOT_READY, "no %s", b.name);
    return download_floats(ctx, what, b.p, b.pixels() * b.f4 * 4u, host, n_floats);
}

// A result computed into ctx->scratch and copied to the host: enqueue(scratch) launches the kernels on ctx->stream (scratch has
// `bytes` + `extra` bytes; the first `bytes` of it are the result), and the call returns when `host` holds it.
template <class Enqueue>
rsrt_status read_back(rsrt_context *ctx, void *host, size_t bytes, size_t extra, Enqueue enqueue)
{
    rsrt_status st = ensure_scratch(ctx, bytes + extra);
    if (st || (st = begin_work(ctx, ctx->stream)) || (st = enqueue(ctx->scratch))) return st;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(host, ctx->scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = end_work(ctx, ctx->stream))) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RSRT_OK;
}

// The same for a result whose size the device decides.  scratch has `scratch_bytes` bytes; enqueue(scratch) launches as above; then the
// `count_bytes` bytes at scratch + count_at reach count_host, size_of() — which may read them — says how many bytes at scratch + data_at
// are the result, and the call returns when `host`, sized to that, holds them.  Two copies and two waits: the second's size is the first's news.
template <class Enqueue, class SizeOf>
rsrt_status read_back_counted(rsrt_context *ctx, size_t scratch_bytes, Enqueue enqueue, size_t count_at, void *count_host, size_t count_bytes, size_t data_at, SizeOf size_of,
                              std::vector<unsigned char> &host)
{
    rsrt_status st = ensure_scratch(ctx, scratch_bytes);
    if (st || (st = begin_work(ctx, ctx->stream)) || (st = enqueue(ctx->scratch))) return st;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(count_host, static_cast<const char *>(ctx->scratch) + count_at, count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = end_work(ctx, ctx->stream))) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = size_of();
    if (data_at + n > scratch_bytes) return fail(ctx, RSRT_ERR_HIP, "read_back_counted: the device counted %zu bytes, more than the scratch buffer's", n);
    host.resize(n);
    if (n) HIP_TRY(ctx, hipMemcpy(host.data(), static_cast<const char *>(ctx->scratch) + data_at, n, hipMemcpyDeviceToHost));
    return RSRT_OK;
}

// the snapshot and the last estimate mean nothing any more (a cleared accumulator, a reset); the buffers stay
void drop_noise(rsrt_context *ctx)
{
    ctx->ns_total = 0;
    ctx->ns_have = false;
}
// The accumulator's size is another one now, or there is no accumulator any more: what was computed from the old size goes.  This is
// the only place that knows the list, and every path that changes the size comes through here (after it has waited for the GPU).
void accumulator_size_changed(rsrt_context *ctx)
{
    release(ctx->dn_scratch);
    ctx->dn_last = nullptr;
    release(ctx->tp_hist);
    release(ctx->tp_mom);
    ctx->tp_cur = ctx->tp_frames = ctx->tp_moments = 0;
    release(ctx->ns_snap);
    drop_noise(ctx);
    release(ctx->bl_pyr);
    ctx->bl_have = false;
    release(ctx->lc_grid);
    ctx->lc_have = false;
    release(ctx->df_buf);
    ctx->df_last = ImageView{};
    release(ctx->mt_buf);
    release(ctx->mt_tiles);
    ctx->mt_last = ImageView{};
    release(ctx->fg_out);
    ctx->fg_last = ImageView{};
}
rsrt_status ensure_accumulator(rsrt_context *ctx, uint32_t w, uint32_t h)
{
    if (ctx->acc.is(w, h)) return RSRT_OK;
    if (ctx->acc.p == ctx->acc.owned) { // the library's own gives way to a new one (a bound one of another size is refused below)
        { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
        accumulator_size_changed(ctx);
    }
    return buffer_ensure(ctx, ctx->acc, w, h);
}
rsrt_status accumulator_and_aov(rsrt_context *ctx, const char *what, const PixelBuffer *also = nullptr)
{
    if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    if (!ctx->aov.p) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no AOV buffer (rsrt_aov_render or rsrt_aov_bind first)", what);
    if (also && !also->p) return fail(ctx, RSRT_ERR_NOT_READY, "%s: no %s (rsrt_guide_render or rsrt_guide_bind first)", what, also->name); // (rsrt_upsample's guide)
    if (ctx->aov.w != ctx->acc.w || ctx->aov.h != ctx->acc.h)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: AOV buffer is %ux%u, accumulator %ux%u", what, ctx->aov.w, ctx->aov.h, ctx->acc.w, ctx->acc.h);
    return RSRT_OK;
}

// the temporal history of the last frame (valid when tp_frames > 0)
float4 *temporal_history(rsrt_context *ctx) { return static_cast<float4 *>(ctx->tp_hist.p) + ctx->tp_cur * ctx->tp_hist.pixels(); }
// ... and its moment records (valid when tp_moments is set too)
float4 *temporal_moments(rsrt_context *ctx) { return static_cast<float4 *>(ctx->tp_mom.p) + ctx->tp_cur * ctx->tp_hist.pixels(); }

// Which image `source` means, or why there is none: the one place with each source's readiness rule.  prefix: "" or the caller's
// "name: " where its texts carry one.  acc_sized: the caller reads the image beside the accumulator, pixel for pixel.
rsrt_status resolve_image(rsrt_context *ctx, const char *what, const char *prefix, uint32_t source, uint32_t sample_total, bool acc_sized, ImageView *v)
{
    switch (source) {
    case IMAGE_MEAN:
        if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
        *v = ImageView{ctx->acc.p, ctx->acc.w, ctx->acc.h, (float)sample_total};
        return RSRT_OK;
    case IMAGE_DENOISED:
        if (!ctx->dn_last) return fail(ctx, RSRT_ERR_NOT_READY, "%sno denoised image (rsrt_denoise first)", prefix);
        *v = ImageView{ctx->dn_last, ctx->acc.w, ctx->acc.h, 1.0f};
        return RSRT_OK;
    case IMAGE_TEMPORAL:
        if (!ctx->tp_hist.p || !ctx->tp_frames || (acc_sized && !ctx->tp_hist.is(ctx->acc.w, ctx->acc.h)))
            return fail(ctx, RSRT_ERR_NOT_READY, "%sno temporal frame since the last reset (rsrt_temporal_accumulate first)", prefix);
        *v = ImageView{temporal_history(ctx), ctx->tp_hist.w, ctx->tp_hist.h, 1.0f};
        return RSRT_OK;
    case IMAGE_UPSAMPLED:
        if (!ctx->up_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "%sno upsampled image (rsrt_upsample first)", prefix);
        *v = ctx->up_last;
        return RSRT_OK;
    case IMAGE_LENS:
        if (!ctx->df_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "%sno lens image (rsrt_dof first)", prefix);
        *v = ctx->df_last;
        return RSRT_OK;
    case IMAGE_MOTION:
        if (!ctx->mt_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "%sno motion image (rsrt_motion_blur first)", prefix);
        *v = ctx->mt_last;
        return RSRT_OK;
    case IMAGE_FOG:
        if (!ctx->fg_last.img) return fail(ctx, RSRT_ERR_NOT_READY, "%sno fog image (rsrt_fog_apply first)", prefix);
        *v = ctx->fg_last;
        return RSRT_OK;
    default:
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: unknown source %u", what, source);
    }
}
rsrt_status image_download(rsrt_context *ctx, const char *what, uint32_t source, float *host, size_t n_floats)
{
    ImageView v;
    rsrt_status st = resolve_image(ctx, what, "", source, 1u, false, &v);
    return st ? st : download_floats(ctx, what, v.img, v.pixels() * 4u, host, n_floats);
}
// rsrt_display_srgb8 of any RGBA32F sum on ctx's device (sample_total is the kernel's integer, which v.total need not hold exactly)
rsrt_status display_view(rsrt_context *ctx, const ImageView &v, uint32_t sample_total, uint8_t *host_rgba8, size_t n_bytes)
{
    DeviceGuard g(ctx->device);
    const size_t n = v.pixels();
    if (!host_rgba8 || n_bytes != n * 4 || sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_srgb8: expected %zu bytes and sample_total > 0", n * 4);
    return read_back(ctx, host_rgba8, n * sizeof(uchar4), 0, [&](void *tmp) {
        hipLaunchKernelGGL(rt_display_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, v.img, n, sample_total, static_cast<uchar4 *>(tmp));
        return RSRT_OK;
    });
}
rsrt_status image_display(rsrt_context *ctx, const char *what, uint32_t source, uint32_t sample_total, uint8_t *host_rgba8, size_t n_bytes)
{
    ImageView v;
    rsrt_status st = resolve_image(ctx, what, "", source, sample_total, false, &v);
    return st ? st : display_view(ctx, v, sample_total, host_rgba8, n_bytes);
}

hipEvent_t get_event(rsrt_context *ctx)
{
    if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// Folds finished launches' HIP-event times into the cumulative totals (may run at any time, e.g. to
// bound the event pool) — it never touches the "since the previous rsrt_get_stats" window.
rsrt_status collect_events(rsrt_context *ctx)
{
    if (ctx->pending_events.empty() && ctx->pending_reduce.empty()) return RSRT_OK;
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    for (auto &re : ctx->pending_reduce) {
        float t = 0;
        HIP_TRY(ctx, hipEventSynchronize(re.end));
        HIP_TRY(ctx, hipEventElapsedTime(&t, re.begin, re.end));
        ctx->cum_reduce_ms += t;
        ctx->event_pool.push_back(re.begin);
        ctx->event_pool.push_back(re.end);
    }
    ctx->pending_reduce.clear();
    for (auto &pe : ctx->pending_events) {
        float t1 = 0, t2 = 0;
        HIP_TRY(ctx, hipEventSynchronize(pe.end));
        HIP_TRY(ctx, hipEventElapsedTime(&t1, pe.begin, pe.traced));
        HIP_TRY(ctx, hipEventElapsedTime(&t2, pe.traced, pe.end));
        ctx->cum_trace_ms += t1;
        ctx->cum_resolve_ms += t2;
        ctx->event_pool.push_back(pe.begin);
        ctx->event_pool.push_back(pe.traced);
        ctx->event_pool.push_back(pe.end);
    }
    ctx->pending_events.clear();
    return RSRT_OK;
}

// rsrt_get_stats: cumulative totals now, and the difference to the totals at the previous call.
rsrt_status collect_stats(rsrt_context *ctx)
{
    rsrt_status st = sync_all(ctx);
    if (st) return st;
    st = collect_events(ctx);
    if (st) return st;
    unsigned long long c[RT_STATS_WORDS] = {0}; // device counters are cumulative
    HIP_TRY(ctx, hipMemcpy(c, ctx->dev_stats, sizeof c, hipMemcpyDeviceToHost));
    rsrt_stats &s = ctx->stats;
    s.paths = c[0] - ctx->base_counts[0];
    s.ext_rays = c[1] - ctx->base_counts[1];
    s.shadow_rays = c[2] - ctx->base_counts[2];
    s.traversal_steps = c[3] - ctx->base_counts[3];
    s.trace_kernel_ms = ctx->cum_trace_ms - ctx->base_trace_ms;
    s.resolve_kernel_ms = ctx->cum_resolve_ms - ctx->base_resolve_ms;
    s.kernel_ms = s.trace_kernel_ms + s.resolve_kernel_ms;
    s.launches = ctx->cum_launches - ctx->base_launches;
    s.total_paths = c[0];
    s.total_ext_rays = c[1];
    s.total_shadow_rays = c[2];
    s.total_kernel_ms = ctx->cum_trace_ms + ctx->cum_resolve_ms;
    s.reduce_ms = ctx->cum_reduce_ms - ctx->base_reduce_ms;
    ctx->base_reduce_ms = ctx->cum_reduce_ms;
    for (int i = 0; i < 4; i++) ctx->base_counts[i] = c[i];
    ctx->base_trace_ms = ctx->cum_trace_ms;
    ctx->base_resolve_ms = ctx->cum_resolve_ms;
    ctx->base_launches = ctx->cum_launches;
    memcpy(ctx->debug_words, c + 4, sizeof ctx->debug_words);
    return RSRT_OK;
}
static_assert(RT_COOP_STATS + RT_COOP_NSTATS == RT_STATS_WORDS, "the cooperative walk's counters are the last stats words");


// Mid-size and big scenes (no whole image in LDS): what the chosen traversal keeps in LDS beside the pools (SceneViewHybrid) — the wide walk
// (trav 4) its image of nodes | records | shading arrays, the fixed-order walk (3) the top block of its elements (any prefix will do), the
// tree walks their nodes + escape links (all or nothing).  Sets the scene's lds_* fields; false: nothing is staged.
static bool hybrid_stage(const rsrt_context *ctx, DevScene &sc, int trav, uint32_t room_f4)
{
    sc.lds_wnodes = 0u;
    if (trav >= 4) {
        sc.lds_wnodes = std::min(ctx->wimg_nodes, room_f4 / 8u);
        if (sc.lds_wnodes == 0) return false;
        sc.lds_float4s = 8u * sc.lds_wnodes;
        sc.lds_hybrid = 3u;
        sc.lds_src = sc.wnodes; // a prefix of the array itself
        return true;
    }
    uint32_t head = trav == 3 ? ctx->hybrid_pnode_f4 : ctx->hybrid_head_f4;
    if (trav == 3) head = std::min(head, room_f4 / 2u * 2u);
    else if (head > room_f4) head = 0u;
    if (head == 0u) return false;
    sc.lds_float4s = head;
    sc.lds_hybrid = trav == 3 ? 2u : 1u;
    sc.lds_src = trav == 3 ? sc.pnodes : sc.nodes;
    return true;
}

// Which traversal TRACE runs (rt_wavepool.h, TRAV): the flat loop where the scene qualifies, else the fixed-order walk,
// else (leaves longer than 8 primitives) the generic tree walk; RSRT_TRAVERSAL / RSRT_FLAT cap the choice for A/B runs.
int select_traversal(const rsrt_context *ctx, const DevScene &sc, uint32_t max_bounces, uint32_t flags)
{
    if (ctx->max_traversal >= 2 && ctx->allow_flat && sc.flat_ok && max_bounces <= RT_FLAT_MAX_BOUNCES) return 2;
    // RSRT_FLAG_PRUNE wants the reference's near-child-first order: a close hit found early is what lets later boxes be
    // skipped (the fixed-order walk prunes 4 % of suzanne's steps, the near-first walk 8 %)
    if (ctx->max_traversal >= 6 && sc.wide_ok && sc.coop_ok && !(flags & RSRT_FLAG_PRUNE)) return 6; // the cooperative walk (rt_coop.h)
    if (ctx->max_traversal >= 4 && sc.wide_ok && !(flags & RSRT_FLAG_PRUNE)) return sc.wide_deep ? 5 : 4; // (5: the same walk with a stack that may overflow into memory)
    if (ctx->max_traversal >= 3 && sc.typed_leaves && !(flags & RSRT_FLAG_PRUNE)) return 3;
    if (ctx->max_traversal >= 1 && sc.typed_leaves) return 1;
    return 0;
}

// One pass of rsrt_render: the path-tracing kernel over P.sample_count samples, then the ordered resolve.
rsrt_status enqueue_pass(rsrt_context *ctx, RenderParams &P, const rsrt_context::PassEvents &pe, const void *kfn, uint32_t block, int bpc,
                         size_t smem, size_t per_sample, uint32_t max_bounces, hipStream_t caller_stream, rsrt_context::Lane &lane)
{
    const uint32_t tile_px = P.tile_w * P.tile_h;
    // the path-tracing kernel: on the lane's stream (behind the resolve that last read this lane's sample buffer: same stream)
    const hipStream_t stream = lane.stream;
    HIP_TRY(ctx, hipEventRecord(pe.begin, stream));
    if (max_bounces > 0) {
        // chunk = one tile x samples_per_chunk samples.  Up to 8 samples per chunk (2048 paths: the
        // counter is touched rarely), fewer when the job is small — e.g. one GPU's share of a
        // partitioned frame — so that every resident wave still gets >= ~32 chunks and the tail,
        // where waves run out of work at different times, stays a few percent.
        {
            const uint64_t waves = (uint64_t)ctx->cus * bpc * (block / RT_WAVE);
            const uint64_t want_chunks = (uint64_t)kChunksPerWave * waves;
            const uint64_t total_tile_samples = (uint64_t)P.n_owned_tiles * P.sample_count;
            uint64_t spc = total_tile_samples / std::max<uint64_t>(want_chunks, 1);
            spc = std::min<uint64_t>(std::max<uint64_t>(spc, 1), std::max<uint32_t>(1u, 2048u / tile_px));
            P.samples_per_chunk = (uint32_t)std::min<uint64_t>(spc, P.sample_count);
            // very small jobs (one sample per call, the reference's interactive mode): split tiles too,
            // down to one wave's worth of pixels per chunk
            P.n_subtiles = 1;
            while (P.samples_per_chunk == 1 && total_tile_samples * P.n_subtiles < want_chunks && tile_px / (P.n_subtiles * 2) >= RT_WAVE &&
                   tile_px % (P.n_subtiles * 2) == 0)
                P.n_subtiles *= 2;
            P.chunk_px = tile_px / P.n_subtiles;
        }
        P.n_sblocks = (P.sample_count + P.samples_per_chunk - 1) / P.samples_per_chunk;
        const uint64_t n_chunks = (uint64_t)P.n_owned_tiles * P.n_sblocks * P.n_subtiles;
        if (n_chunks > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "too many work chunks");
        P.n_chunks = (uint32_t)n_chunks;
        HIP_TRY(ctx, hipMemsetAsync(lane.work_counter, 0, sizeof(unsigned int), stream));
        const uint32_t waves_wanted = (uint32_t)std::min<uint64_t>(n_chunks, 0x7fffffffull);
        const uint32_t wpb = block / RT_WAVE;
        uint32_t grid = std::min<uint32_t>((waves_wanted + wpb - 1) / wpb, std::max<uint32_t>(1u, (uint32_t)(ctx->cus * bpc)));
        grid = std::max(grid, 1u);
        void *kargs[] = {&P};
        HIP_TRY(ctx, hipLaunchKernel(kfn, dim3(grid), dim3(block), kargs, smem, stream));
        ctx->cum_launches++;
    } else {
        HIP_TRY(ctx, hipMemsetAsync(lane.sample_buf, 0, per_sample * P.sample_count, stream));
    }
    HIP_TRY(ctx, hipEventRecord(pe.traced, stream));
    HIP_TRY(ctx, hipEventRecord(lane.traced, stream));
    lane.traced_valid = true;
    // The ordered resolve, behind the kernel on the lane's stream.  It adds into the accumulator, so it comes after (a) what the
    // caller's stream holds at this moment (a clear, a caller's own kernel on a bound accumulator) and (b) whatever the context
    // enqueued last on any stream — the previous pass's resolve above all: samples are added in increasing order.  Nothing is
    // put on the caller's stream that could wait there (several streams share a hardware queue: a wait parked in the caller's
    // queue holds up the lane that shares it — measured, 0.81 against 0.60 ms per single-sample call); the caller's stream is
    // ordered behind the resolve by rsrt_render once per call, if the caller named a stream of its own.
    HIP_TRY(ctx, hipEventRecord(lane.caller_at, caller_stream));
    HIP_TRY(ctx, hipStreamWaitEvent(stream, lane.caller_at, 0));
    if (ctx->last_valid && ctx->last_stream != stream) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->last_event, 0));
    hipLaunchKernelGGL(rt_resolve_kernel, dim3((P.n_slots + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, stream, P, ctx->acc.p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->cum_launches++;
    HIP_TRY(ctx, hipEventRecord(pe.end, stream));
    HIP_TRY(ctx, hipEventRecord(lane.resolved, stream));
    lane.resolved_valid = true;
    return end_work(ctx, stream); // the context's chain now ends on the lane's stream
}

// the device-only packing of an uploaded environment (rt_alias_device.h, rt_env_pack_*): pmf copies in the texels' alpha and
// in the alias entries' pad words
rsrt_status pack_environment(rsrt_context *ctx, Env &e)
{
    const size_t n = (size_t)e.width * e.height;
    rsrt_status st = begin_work(ctx, ctx->stream);
    if (st) return st;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(rt_env_pack_texels_kernel, dim3(nb), dim3(256), 0, ctx->stream, e.rgba, e.alias, n);
    hipLaunchKernelGGL(rt_env_pack_alias_kernel, dim3(nb), dim3(256), 0, ctx->stream, e.alias, n);
    HIP_TRY(ctx, hipGetLastError());
    if ((st = end_work(ctx, ctx->stream))) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RSRT_OK;
}

} // namespace

extern "C" {

rsrt_status rsrt_context_create(int device_index, rsrt_context **out)
{
    if (!out) return fail(nullptr, RSRT_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, RSRT_ERR_NO_DEVICE, "no HIP device available (%s); librsrt has no CPU path", hipGetErrorString(e));
    if (device_index < 0 || device_index >= n) return fail(nullptr, RSRT_ERR_INVALID_ARGUMENT, "device_index %d out of range [0,%d)", device_index, n);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_index)) != hipSuccess) return fail(nullptr, RSRT_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RSRT_ERR_NO_DEVICE, "device %d is %s; librsrt is built for gfx950 (MI355X) only", device_index, prop.gcnArchName);
    rsrt_context *ctx = new rsrt_context();
    ctx->device = device_index;
    ctx->cus = prop.multiProcessorCount;
    DeviceGuard g(device_index);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->last_event, hipEventDisableTiming)) != hipSuccess ||
        (e = [&] { hipError_t r = hipSuccess;
                   for (auto &L : ctx->lanes) {
                       if (r == hipSuccess) r = hipMalloc(&L.work_counter, sizeof(unsigned int));
                       if (r == hipSuccess) r = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
                       if (r == hipSuccess) r = hipEventCreateWithFlags(&L.resolved, hipEventDisableTiming);
                       if (r == hipSuccess) r = hipEventCreateWithFlags(&L.traced, hipEventDisableTiming);
                       if (r == hipSuccess) r = hipEventCreateWithFlags(&L.caller_at, hipEventDisableTiming);
                   }
                   return r; }()) != hipSuccess ||
        (e = hipMalloc(&ctx->dev_stats, RT_STATS_WORDS * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemsetAsync(ctx->dev_stats, 0, RT_STATS_WORDS * sizeof(unsigned long long), ctx->stream)) != hipSuccess || // (not the null stream:
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {                                                             // see buffer_ensure)
        fail(nullptr, RSRT_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
        delete ctx;
        return RSRT_ERR_HIP;
    }
    for (bool small : {false, true})
        for (int m = 0; m < 21; m++) (void)hipFuncSetAttribute(variant_function(small, m / 7, m % 7), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (const char *kv = getenv("RSRT_KERNEL")) ctx->small_form = atoi(kv) == 2; // 2: the small form for every job; 4 (the default) or anything else: the product's choice
    if (const char *hy = getenv("RSRT_HYBRID")) ctx->allow_hybrid = atoi(hy) != 0; // 0: mid-size scenes read everything from global memory (A/B)
    if (const char *ty = getenv("RSRT_TRAVERSAL")) ctx->max_traversal = atoi(ty); // cap: 0 generic tree walk, 1 typed leaf loops, 2 + flat small-scene loop, 3 + fixed-order walk (A/B)
    if (const char *fl = getenv("RSRT_FLAT")) ctx->allow_flat = atoi(fl) != 0; // 0: small scenes take the walk a big scene would (A/B)
    if (const char *fo = getenv("RSRT_FLAT_ORIENTED")) ctx->flat_oriented = atoi(fo) != 0; // 0: no per-octant leaf tables (A/B)
    if (const char *tb = getenv("RSRT_TRACE_BUDGET")) { int v = atoi(tb); if (v > 0) ctx->trace_budget = (uint32_t)v; }
    if (const char *fq = getenv("RSRT_FLAT_QUORUM")) { int v = atoi(fq); if (v >= 0 && v <= 100) ctx->flat_quorum = (uint32_t)v; }
    if (const char *e2 = getenv("RSRT_SAMPLE_BUFFER_MB")) { long v = atol(e2); if (v > 0) ctx->sample_buffer_budget = (size_t)v << 20; }
    if (const char *pr = getenv("RSRT_PROBE_REPEAT")) { int v = atoi(pr); if (v > 1 && v <= 4096) ctx->probe_repeat = (uint32_t)v; }
    if (const char *cl = getenv("RSRT_COOP_LDS_CAP")) { int v = atoi(cl); if (v >= (int)RT_COOP_MIN_LDS_CAP && v <= (int)RT_COOP_NCAP) ctx->coop_lds_cap = (uint32_t)v; }
    if (const char *cf = getenv("RSRT_COOP_LIFO_AT")) { int v = atoi(cf); if (v >= 0 && v <= (int)RT_COOP_NARROW_AT) ctx->coop_lifo_at = (uint32_t)v; }
    if (const char *cn = getenv("RSRT_COOP_NARROW_AT")) { int v = atoi(cn); if (v >= 0 && v <= (int)RT_COOP_NARROW_AT) ctx->coop_narrow_at = (uint32_t)v; }
    if (const char *cg = getenv("RSRT_COOP_GCAP")) { int v = atoi(cg); if (v >= 64 && v <= (int)RT_COOP_GCAP && v % 64 == 0) ctx->coop_gcap = (uint32_t)v; }
    if (const char *cm = getenv("RSRT_COMM_MODE")) ctx->comm_dense_mode = strcmp(cm, "reduce") == 0;
    if (const char *hq = getenv("GPU_MAX_HW_QUEUES")) { int v = atoi(hq); if (v > 0) ctx->hw_queues = v; }
    for (int m = 0; m < 21; m++) (void)hipFuncSetAttribute(probe_function(m / 7, m % 7), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    char buf[256];
    snprintf(buf, sizeof buf, "librsrt 0.1; %s (%s); %d CUs", prop.name, prop.gcnArchName, ctx->cus);
    ctx->description = buf;
    *out = ctx;
    return RSRT_OK;
}

void rsrt_context_destroy(rsrt_context *ctx)
{
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    (void)sync_all(ctx);
    (void)rsrt_comm_destroy(ctx);
    for (auto &re : ctx->pending_reduce) { (void)hipEventDestroy(re.begin); (void)hipEventDestroy(re.end); }
    if (ctx->last_event) (void)hipEventDestroy(ctx->last_event);
    (void)hipFree(ctx->scratch);
    (void)hipFree(ctx->comm_buf);
    for (auto &pe : ctx->pending_events) { (void)hipEventDestroy(pe.begin); (void)hipEventDestroy(pe.traced); (void)hipEventDestroy(pe.end); }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    (void)hipFree(ctx->scene_blob);
    for (auto &e : ctx->envs) { (void)hipFree(e.rgba); (void)hipFree(e.alias); }
    accumulator_size_changed(ctx);
    for (PixelBuffer *b : {&ctx->acc, &ctx->aov, &ctx->guide, &ctx->fog}) (void)hipFree(b->owned);
    release(ctx->up_scratch);
    release(ctx->up_out);
    release(ctx->fg_src);
    (void)hipFree(ctx->ns_tiles);
    (void)hipFree(ctx->ex.hist);
    (void)hipFree(ctx->wb.hist);
    (void)hipFree(ctx->cl_lut);
    for (auto &L : ctx->lanes) {
        (void)hipFree(L.sample_buf);
        (void)hipFree(L.cold_state);
        (void)hipFree(L.work_counter);
        if (L.resolved) (void)hipEventDestroy(L.resolved);
        if (L.traced) (void)hipEventDestroy(L.traced);
        if (L.caller_at) (void)hipEventDestroy(L.caller_at);
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    (void)hipFree(ctx->dev_stats);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *rsrt_last_error(const rsrt_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

#ifndef RSRT_BUILD_ID
#define RSRT_BUILD_ID "unknown"
#endif
const char *rsrt_build_id(void) { return RSRT_BUILD_ID; }

const char *rsrt_describe(rsrt_context *ctx) { return ctx ? ctx->description.c_str() : "librsrt 0.1"; }

// validate_scene, then build_scene_image (rt_scene_image.h) with the library's LDS room; a refusal's reason goes to ctx (NULL: to this thread's)
static rsrt_status checked_scene_image(rsrt_context *ctx, const SceneInputs &in, bool flat_oriented, SceneImage &out)
{
    uint32_t depth = 0;
    out.error = validate_scene(in, &depth);
    if (out.error.empty()) out = build_scene_image(in, depth, flat_oriented, kSmallImageBytes, kHybridRoomF4);
    return out.error.empty() ? RSRT_OK : fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s", out.error.c_str());
}

rsrt_status rsrt_upload_scene(rsrt_context *ctx, const rsrt_material *materials, uint32_t n_materials, const rsrt_sphere *spheres,
                              uint32_t n_spheres, const rsrt_plane *planes, uint32_t n_planes, const rsrt_vec3 *vertices,
                              uint32_t n_vertices, const rsrt_vec3 *normals, uint32_t n_normals, const rsrt_triangle *triangles,
                              uint32_t n_triangles, const rsrt_primitive_info *primitives, uint32_t n_primitives,
                              const rsrt_bvh_node *nodes, uint32_t n_nodes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ctx->tp_frames = 0; // the temporal history belongs to the old scene
    const SceneInputs in{materials, n_materials, spheres, n_spheres, planes, n_planes, vertices, n_vertices, normals, n_normals,
                         triangles, n_triangles, primitives, n_primitives, nodes, n_nodes};
    SceneImage built;
    if (rsrt_status st = checked_scene_image(ctx, in, ctx->flat_oriented, built)) return st; // (every refusal but one: the device is not touched yet)
    const rsrt_scene_image_info &im = built.info;

    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (ctx->scene_blob) { (void)hipFree(ctx->scene_blob); ctx->scene_blob = nullptr; }
    ctx->scene_ready = false;
    HIP_TRY(ctx, hipMalloc(&ctx->scene_blob, built.image.size() * sizeof(float4)));
    HIP_TRY(ctx, hipMemcpy(ctx->scene_blob, built.image.data(), built.image.size() * sizeof(float4), hipMemcpyHostToDevice));
    const float4 *blob = ctx->scene_blob;
    DevScene &sc = ctx->scene;
    sc.nodes = blob + im.nodes; sc.escape = blob + im.escape; sc.prims = blob + im.prims; sc.tri_normals = blob + im.tri_normals;
    sc.materials = blob + im.materials; sc.fb_spheres = blob + im.fb_spheres; sc.fb_planes = blob + im.fb_planes;
    sc.flat_leaves = blob + im.flat_leaves; sc.pnodes = blob + im.pnodes; sc.wnodes = blob + im.wnodes;
    sc.flat_rank = reinterpret_cast<const uint32_t *>(blob + im.flat_rank);
    sc.prim_rank = reinterpret_cast<const uint32_t *>(blob + im.prim_rank);
    sc.n_nodes = im.n_nodes; sc.n_prims = im.n_prims; sc.n_tris = im.n_tris; sc.n_materials = im.n_materials;
    sc.n_spheres = im.n_spheres; sc.n_planes = im.n_planes; sc.n_leaves = im.n_leaves; sc.n_pnodes = im.n_pnodes; sc.n_wnodes = im.n_wnodes;
    sc.tri_mask_lo = im.tri_mask_lo; sc.tri_mask_hi = im.tri_mask_hi; sc.plane_mask_lo = im.plane_mask_lo; sc.plane_mask_hi = im.plane_mask_hi;
    sc.flat_ok = im.flat_ok; sc.flat_ostride = im.flat_ostride; sc.typed_leaves = im.typed_leaves;
    sc.wide_ok = im.wide_ok; sc.wide_deep = im.wide_deep; sc.coop_ok = im.coop_ok;
    memcpy(sc.cull_min, im.cull_min, sizeof sc.cull_min);
    memcpy(sc.cull_max, im.cull_max, sizeof sc.cull_max);
    memcpy(sc.cull_mask, im.cull_mask, sizeof sc.cull_mask);
    sc.cull_always = im.cull_always; sc.n_cull = im.n_cull;
    sc.stack_entries = im.stack_entries;
    sc.lds_wnodes = 0u; // (set per launch, hybrid_stage)
    const size_t stack_bytes = (size_t)sc.stack_entries * RT_BLOCK * sizeof(uint32_t);
    if (stack_bytes > 128 * 1024) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bvh depth %u exceeds the supported traversal stack", sc.stack_entries - 1u); // (the one refusal that leaves the context without a scene)
    sc.lds_float4s = im.lds_float4s; // whole image in LDS only while it leaves room for the path pools
    sc.lds_hybrid = 0;
    sc.lds_src = sc.nodes; // the image starts with the nodes
    ctx->hybrid_head_f4 = ctx->hybrid_pnode_f4 = 0;
    ctx->wimg_nodes = 0;
    if (sc.lds_float4s == 0) { // mid-size: what every box step touches goes to LDS, one big workgroup per CU shares the copy
        if (im.traversal_head_f4 * sizeof(float4) <= 40 * 1024) ctx->hybrid_head_f4 = (uint32_t)im.traversal_head_f4; // nodes + escape links (tree walks; the render call checks the room beside its pools)
        ctx->hybrid_pnode_f4 = 2u * im.top_elems; // the top block of the fixed-order walk's nodes (all of them when the scene is mid-size)
        ctx->wimg_nodes = im.wimg_nodes; // the head of the wide-node array, as far as the room beside the launch's pools goes (hybrid_stage); a small scene runs from its whole image
    }
    memset(ctx->blocks_per_cu, 0, sizeof ctx->blocks_per_cu); // the kernels' dynamic LDS size depends on the scene: occupancy is asked for again
    ctx->scene_ready = true;
    return RSRT_OK;
}

// build_bvh (reference src/bvh.rs:13-337) on the device: csrc/hip/rt_bvh_device.h.  Same arguments and outputs as the host
// builder rsrt_build_bvh (include/rsrt_host.h) — host arrays in, host arrays out; the inputs are uploaded, the tree is built by
// kernels, the result is downloaded — plus the time the device spent building (events around the kernels, uploads excluded).
rsrt_status rsrt_build_bvh_device(rsrt_context *ctx, const rsrt_sphere *spheres, uint32_t n_spheres, const rsrt_plane_desc *planes, uint32_t n_planes,
                                  const rsrt_vec3 *vertices, uint32_t n_vertices, const rsrt_triangle *triangles, uint32_t n_triangles,
                                  rsrt_primitive_info *primitives_out, rsrt_bvh_node *nodes_out, uint32_t *n_nodes_out, uint32_t *depth_out, double *build_ms_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    const uint64_t n64 = (uint64_t)n_spheres + n_planes + n_triangles;
    if (n64 == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: empty scene"); // (the reference asserts, src/bvh.rs:222)
    if (n64 > 0x3fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: too many primitives");
    if (!primitives_out || !nodes_out || (n_spheres && !spheres) || (n_planes && !planes) || (n_triangles && (!triangles || !vertices)))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: NULL array");
    for (uint32_t i = 0; i < n_triangles; i++)
        if (triangles[i].vertex_0 >= n_vertices || triangles[i].vertex_1 >= n_vertices || triangles[i].vertex_2 >= n_vertices)
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: triangle %u: vertex index out of range", i);
    const uint32_t n = (uint32_t)n64;
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    // one allocation: inputs | items x 2 (3 float4 arrays each) | build nodes | tasks x 2 | pre, holes, backs | counters | outputs
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_sph = take((size_t)n_spheres * sizeof(rsrt_sphere)), o_pl = take((size_t)n_planes * sizeof(rsrt_plane_desc)),
                 o_v = take((size_t)n_vertices * sizeof(rsrt_vec3)), o_tri = take((size_t)n_triangles * sizeof(rsrt_triangle));
    size_t o_items[6];
    for (auto &o : o_items) o = take((size_t)n * sizeof(float4));
    const size_t o_nodes = take((size_t)2 * n * sizeof(BvhNodeB)), o_t0 = take((size_t)n * sizeof(BvhTask)), o_t1 = take((size_t)n * sizeof(BvhTask));
    const size_t o_pre = take((size_t)n * 4), o_holes = take((size_t)n * 4), o_backs = take((size_t)n * 4), o_cnt = take(16);
    const size_t o_outn = take((size_t)2 * n * sizeof(rsrt_bvh_node)), o_outp = take((size_t)n * sizeof(rsrt_primitive_info));
    char *blob = nullptr;
    HIP_TRY(ctx, hipMalloc(&blob, off));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } free_blob{blob};
    hipStream_t q = ctx->stream;
    if (n_spheres) HIP_TRY(ctx, hipMemcpyAsync(blob + o_sph, spheres, (size_t)n_spheres * sizeof(rsrt_sphere), hipMemcpyHostToDevice, q));
    if (n_planes) HIP_TRY(ctx, hipMemcpyAsync(blob + o_pl, planes, (size_t)n_planes * sizeof(rsrt_plane_desc), hipMemcpyHostToDevice, q));
    if (n_vertices) HIP_TRY(ctx, hipMemcpyAsync(blob + o_v, vertices, (size_t)n_vertices * sizeof(rsrt_vec3), hipMemcpyHostToDevice, q));
    if (n_triangles) HIP_TRY(ctx, hipMemcpyAsync(blob + o_tri, triangles, (size_t)n_triangles * sizeof(rsrt_triangle), hipMemcpyHostToDevice, q));
    BvhItems A{reinterpret_cast<float4 *>(blob + o_items[0]), reinterpret_cast<float4 *>(blob + o_items[1]), reinterpret_cast<float4 *>(blob + o_items[2])};
    BvhItems B{reinterpret_cast<float4 *>(blob + o_items[3]), reinterpret_cast<float4 *>(blob + o_items[4]), reinterpret_cast<float4 *>(blob + o_items[5])};
    BvhNodeB *bnodes = reinterpret_cast<BvhNodeB *>(blob + o_nodes);
    BvhTask *tasks[2] = {reinterpret_cast<BvhTask *>(blob + o_t0), reinterpret_cast<BvhTask *>(blob + o_t1)};
    uint32_t *counters = reinterpret_cast<uint32_t *>(blob + o_cnt);
    hipEvent_t e0 = get_event(ctx), e1 = get_event(ctx);
    struct Back { rsrt_context *c; hipEvent_t a, b; ~Back() { c->event_pool.push_back(a); c->event_pool.push_back(b); } } back{ctx, e0, e1};
    HIP_TRY(ctx, hipEventRecord(e0, q));
    hipLaunchKernelGGL(rt_bvh_items_kernel, dim3((n + 255) / 256), dim3(256), 0, q, reinterpret_cast<const rsrt_sphere *>(blob + o_sph), n_spheres,
                       reinterpret_cast<const rsrt_plane_desc *>(blob + o_pl), n_planes, reinterpret_cast<const rsrt_vec3 *>(blob + o_v),
                       reinterpret_cast<const rsrt_triangle *>(blob + o_tri), n_triangles, A);
    HIP_TRY(ctx, hipMemcpyAsync(B.bmin, A.bmin, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, q)); // (a root that is a leaf never writes the other copy)
    HIP_TRY(ctx, hipMemcpyAsync(B.bmax, A.bmax, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, q));
    HIP_TRY(ctx, hipMemcpyAsync(B.cen, A.cen, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, q));
    const BvhTask root{0u, n, 0u};
    uint32_t cnt[4] = {1u, 0u, 0u, 0u}; // build nodes allocated, tasks of the next level, error
    HIP_TRY(ctx, hipMemcpyAsync(tasks[0], &root, sizeof root, hipMemcpyHostToDevice, q));
    HIP_TRY(ctx, hipMemcpyAsync(counters, cnt, sizeof cnt, hipMemcpyHostToDevice, q));
    std::vector<std::pair<uint32_t, uint32_t>> levels; // first build node, count
    uint32_t n_tasks = 1, first = 0, n_build = 1;
    BvhItems *src = &A, *dst = &B;
    for (int lvl = 0; n_tasks > 0; lvl++) {
        if (lvl > 4096) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: tree deeper than 4096 levels");
        levels.push_back({first, n_tasks});
        hipLaunchKernelGGL(rt_bvh_level_kernel, dim3(n_tasks), dim3(RT_BVH_BLOCK), 0, q, tasks[lvl & 1], n_tasks, *src, *dst, bnodes, tasks[(lvl + 1) & 1], counters,
                           reinterpret_cast<uint32_t *>(blob + o_pre), reinterpret_cast<uint32_t *>(blob + o_holes), reinterpret_cast<uint32_t *>(blob + o_backs));
        hipLaunchKernelGGL(rt_bvh_copy_leaves_kernel, dim3(n_tasks), dim3(64), 0, q, tasks[lvl & 1], n_tasks, bnodes, *src, *dst);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(cnt, counters, sizeof cnt, hipMemcpyDeviceToHost, q));
        HIP_TRY(ctx, hipStreamSynchronize(q));
        if (cnt[2]) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_bvh: a split left one side empty (the reference's median fallback, src/bvh.rs:317-326, is not built on the device): use rsrt_build_bvh");
        first = n_build;
        n_tasks = cnt[1];
        n_build = cnt[0];
        cnt[1] = 0;
        HIP_TRY(ctx, hipMemcpyAsync(counters + 1, &cnt[1], 4, hipMemcpyHostToDevice, q));
        std::swap(src, dst);
    }
    // (after the swap `src` names the copy the last level wrote: every range is final in it)
    for (size_t d = levels.size(); d-- > 0;)
        hipLaunchKernelGGL(rt_bvh_sizes_kernel, dim3((levels[d].second + 255) / 256), dim3(256), 0, q, bnodes, levels[d].first, levels[d].second);
    for (size_t d = 0; d < levels.size(); d++)
        hipLaunchKernelGGL(rt_bvh_positions_kernel, dim3((levels[d].second + 255) / 256), dim3(256), 0, q, bnodes, levels[d].first, levels[d].second);
    hipLaunchKernelGGL(rt_bvh_emit_kernel, dim3((n_build + 255) / 256), dim3(256), 0, q, bnodes, n_build, reinterpret_cast<rsrt_bvh_node *>(blob + o_outn));
    hipLaunchKernelGGL(rt_bvh_prims_kernel, dim3((n + 255) / 256), dim3(256), 0, q, *src, n, reinterpret_cast<rsrt_primitive_info *>(blob + o_outp));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(e1, q));
    HIP_TRY(ctx, hipMemcpyAsync(nodes_out, blob + o_outn, (size_t)n_build * sizeof(rsrt_bvh_node), hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipMemcpyAsync(primitives_out, blob + o_outp, (size_t)n * sizeof(rsrt_primitive_info), hipMemcpyDeviceToHost, q));
    HIP_TRY(ctx, hipStreamSynchronize(q));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    if (n_nodes_out) *n_nodes_out = n_build;
    if (depth_out) *depth_out = (uint32_t)levels.size() - 1u;
    if (build_ms_out) *build_ms_out = ms;
    return RSRT_OK;
}

// The scene's device image on the host (no context, no GPU needed): what rsrt_upload_scene copies to the device and the layout it
// fills DevScene from (rt_scene_image.h), exposed so that a CPU test can read every table.  include/rsrt.h has the arguments.
rsrt_status rsrt_scene_image_build(const rsrt_material *materials, uint32_t n_materials, const rsrt_sphere *spheres, uint32_t n_spheres,
                                   const rsrt_plane *planes, uint32_t n_planes, const rsrt_vec3 *vertices, uint32_t n_vertices,
                                   const rsrt_vec3 *normals, uint32_t n_normals, const rsrt_triangle *triangles, uint32_t n_triangles,
                                   const rsrt_primitive_info *primitives, uint32_t n_primitives, const rsrt_bvh_node *nodes, uint32_t n_nodes,
                                   uint32_t flat_oriented, float *image_out, size_t *n_float4, rsrt_scene_image_info *info_out)
{
    if (!n_float4) return RSRT_ERR_INVALID_ARGUMENT;
    const SceneInputs in{materials, n_materials, spheres, n_spheres, planes, n_planes, vertices, n_vertices, normals, n_normals,
                         triangles, n_triangles, primitives, n_primitives, nodes, n_nodes};
    SceneImage built;
    if (rsrt_status st = checked_scene_image(nullptr, in, flat_oriented != 0, built)) return st; // (rsrt_last_error(NULL) has the reason)
    const size_t cap = *n_float4;
    *n_float4 = built.image.size();
    if (info_out) *info_out = built.info;
    if (image_out) {
        if (cap < built.image.size()) return fail(nullptr, RSRT_ERR_INVALID_ARGUMENT, "image_out holds %zu float4s, the image has %zu", cap, built.image.size());
        memcpy(image_out, built.image.data(), built.image.size() * sizeof(float4));
    }
    return RSRT_OK;
}

// The wide walk's tree for a BVH, on the host (no GPU needed): the wnodes section of the scene image on its own, with the permutation
// of the records, exposed so that a CPU test can walk it.  wnodes_out: 32 floats per wide node (DevScene::wnodes); *n_wnodes:
// capacity in, count out; old_of_new: for every record index the walk uses, the index into `primitives` as given.
// RSRT_ERR_INVALID_ARGUMENT: the scene does not qualify.
rsrt_status rsrt_wide_tree_build(const rsrt_primitive_info *primitives, uint32_t n_primitives, const rsrt_bvh_node *nodes, uint32_t n_nodes,
                                 float *wnodes_out, uint32_t *n_wnodes, uint32_t *old_of_new)
{
    if (!primitives || !nodes || !n_wnodes || n_nodes == 0) return RSRT_ERR_INVALID_ARGUMENT;
    uint32_t depth = 0;
    if (!validate_tree(nodes, n_nodes, n_primitives, &depth).empty()) return RSRT_ERR_INVALID_ARGUMENT;
    std::vector<WideNode> wide;
    std::vector<rsrt_primitive_info> pp;
    std::vector<rsrt_bvh_node> np;
    std::vector<uint32_t> oon;
    if (!build_wide_tree(nodes, n_nodes, primitives, n_primitives, wide, pp, np, &oon)) return RSRT_ERR_INVALID_ARGUMENT;
    const uint32_t cap = *n_wnodes;
    *n_wnodes = (uint32_t)wide.size();
    if (wnodes_out) {
        if (cap < wide.size()) return RSRT_ERR_INVALID_ARGUMENT;
        fill_wide_nodes(wide, np.data(), pp.data(), reinterpret_cast<float4 *>(wnodes_out));
    }
    if (old_of_new) memcpy(old_of_new, oon.data(), oon.size() * sizeof(uint32_t));
    return RSRT_OK;
}

rsrt_status rsrt_upload_environment(rsrt_context *ctx, uint32_t slot, uint32_t width, uint32_t height, const float *rgba,
                                    const rsrt_alias_entry *alias)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    ctx->tp_frames = 0; // the temporal history saw the old environment
    if (!rgba || width == 0 || height == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment: NULL data or zero size");
    if ((uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment too large");
    if (slot > 63) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "environment slot %u > 63", slot);
    const size_t n = (size_t)width * height;
    if (alias)
        for (size_t i = 0; i < n; i++)
            if (alias[i].alias_index >= n) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "alias entry %zu: alias_index %u out of range", i, alias[i].alias_index);
    if (ctx->envs.size() <= slot) ctx->envs.resize(slot + 1);
    Env &e = ctx->envs[slot];
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    if (e.rgba) { (void)hipFree(e.rgba); e.rgba = nullptr; }
    if (e.alias) { (void)hipFree(e.alias); e.alias = nullptr; }
    e.width = e.height = 0;
    HIP_TRY(ctx, hipMalloc(&e.rgba, n * sizeof(float4)));
    HIP_TRY(ctx, hipMalloc(&e.alias, n * sizeof(uint4)));
    HIP_TRY(ctx, hipMemcpy(e.rgba, rgba, n * sizeof(float4), hipMemcpyHostToDevice));
    if (alias) {
        HIP_TRY(ctx, hipMemcpy(e.alias, alias, n * sizeof(uint4), hipMemcpyHostToDevice));
        e.width = width;
        e.height = height;
        return pack_environment(ctx, e);
    }
    e.width = width;
    e.height = height;
    const rsrt_status st = rsrt_environment_build_alias(ctx, slot, nullptr, 0, nullptr); // AliasTable::build_by_luminance on the device
    if (st) { e.width = e.height = 0; }
    return st;
}

// AliasTable::build_by_luminance (environments.rs:96-187) for the texels ALREADY in `slot`, on the device
// (rt_alias_device.h): same bits as the host builder rsrt_alias_table_build.  Replaces the slot's alias table.
rsrt_status rsrt_environment_build_alias(rsrt_context *ctx, uint32_t slot, rsrt_alias_entry *host_out, size_t n_entries, uint32_t *leftover_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (slot >= ctx->envs.size() || !ctx->envs[slot].rgba || !ctx->envs[slot].alias || ctx->envs[slot].width == 0)
        return fail(ctx, RSRT_ERR_NOT_READY, "environment %u not uploaded", slot);
    Env &e = ctx->envs[slot];
    const size_t n = (size_t)e.width * e.height;
    if (host_out && n_entries != n) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "build_alias: expected %zu entries", n);
    const uint32_t nb = (uint32_t)((n + 255) / 256);
    // scratch: p[n] | small[n] | large[n] | block counts[nb] | {sum, n_small, leftover}
    const size_t bytes = n * 4 * 3 + (size_t)nb * 4 + 16;
    rsrt_status st = ensure_scratch(ctx, bytes);
    if (st || (st = begin_work(ctx, ctx->stream))) return st;
    float *p = static_cast<float *>(ctx->scratch);
    uint32_t *small = reinterpret_cast<uint32_t *>(p + n), *large = small + n, *blocks = large + n, *scalars = blocks + nb;
    hipStream_t q = ctx->stream;
    hipLaunchKernelGGL(rt_alias_weights_kernel, dim3(nb), dim3(256), 0, q, e.rgba, e.width, e.height, p);
    hipLaunchKernelGGL(rt_alias_sum_kernel, dim3(1), dim3(64), 0, q, p, n, reinterpret_cast<float *>(scalars));
    hipLaunchKernelGGL(rt_alias_normalise_kernel, dim3(nb), dim3(256), 0, q, p, n, reinterpret_cast<const float *>(scalars), e.alias, blocks);
    hipLaunchKernelGGL(rt_alias_scan_kernel, dim3(1), dim3(1024), 0, q, blocks, nb, scalars + 1);
    hipLaunchKernelGGL(rt_alias_scatter_kernel, dim3(nb), dim3(256), 0, q, p, n, blocks, small, large);
    hipLaunchKernelGGL(rt_alias_vose_kernel, dim3(1), dim3(64), 0, q, p, n, small, scalars + 1, large, e.alias, scalars + 2);
    hipLaunchKernelGGL(rt_alias_pmf_kernel, dim3(nb), dim3(256), 0, q, p, n, e.alias);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t left = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&left, scalars + 2, 4, hipMemcpyDeviceToHost, q));
    if (host_out) HIP_TRY(ctx, hipMemcpyAsync(host_out, e.alias, n * sizeof(uint4), hipMemcpyDeviceToHost, q)); // (before the pad words are packed)
    if ((st = end_work(ctx, q))) return st;
    HIP_TRY(ctx, hipStreamSynchronize(q));
    if (leftover_out) *leftover_out = left;
    return pack_environment(ctx, e);
}

rsrt_status rsrt_set_partition(rsrt_context *ctx, uint32_t rank, uint32_t world_size, uint32_t tile_w, uint32_t tile_h)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    if (world_size == 0 || world_size > 65535u || rank >= world_size) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "rank %u not in [0,%u) (or more than 65535 ranks)", rank, world_size);
    if (tile_w == 0 || tile_h == 0 || tile_w * tile_h > 4096 || (tile_w * tile_h) % RT_WAVE != 0)
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "tile %ux%u: pixel count must be a multiple of 64 and at most 4096", tile_w, tile_h);
    ctx->rank = rank; ctx->world = world_size; ctx->tile_w = tile_w; ctx->tile_h = tile_h;
    return RSRT_OK;
}

rsrt_status rsrt_accumulator_resize(rsrt_context *ctx, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", width, height);
    if (ctx->acc.p != ctx->acc.owned) { rsrt_status st0 = rsrt_accumulator_bind(ctx, nullptr, 0, 0); if (st0) return st0; } // a caller's is let go first
    return ensure_accumulator(ctx, width, height);
}

rsrt_status rsrt_accumulator_bind(rsrt_context *ctx, void *device_rgba32f, uint32_t width, uint32_t height)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    const uint32_t w0 = ctx->acc.w, h0 = ctx->acc.h;
    const rsrt_status st = buffer_bind(ctx, ctx->acc, device_rgba32f, width, height);
    if (ctx->acc.w != w0 || ctx->acc.h != h0) accumulator_size_changed(ctx); // (to "none" too: NULL with no buffer of the library's to go back to)
    return st;
}

rsrt_status rsrt_accumulator_clear(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    const rsrt_status st = buffer_clear(ctx, ctx->acc);
    if (!st) drop_noise(ctx); // (a snapshot of what was cleared pairs with nothing)
    return st;
}

rsrt_status rsrt_accumulator_download(rsrt_context *ctx, float *host_rgba, size_t n_floats)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return buffer_download(ctx, "download", ctx->acc, host_rgba, n_floats);
}

rsrt_status rsrt_resolve_mean_f16(rsrt_context *ctx, uint32_t sample_total, uint16_t *host, size_t n_halfs)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    const size_t n = ctx->acc.pixels();
    if (!host || n_halfs != n * 4 || sample_total == 0) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "resolve_mean_f16: expected %zu halfs and sample_total > 0", n * 4);
    return read_back(ctx, host, n * sizeof(ushort4), 0, [&](void *tmp) {
        hipLaunchKernelGGL(rt_mean_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->acc.p, n, 0.0f, sample_total, static_cast<ushort4 *>(tmp));
        return RSRT_OK;
    });
}

rsrt_status rsrt_debug_view_f16(rsrt_context *ctx, uint32_t dev_index, uint32_t environment_index, uint32_t sample_count, uint16_t *host_inout, size_t n_halfs)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->acc.p) return fail(ctx, RSRT_ERR_NOT_READY, "no accumulator");
    if (dev_index != 2u && dev_index != 3u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "debug_view: dev_index %u (2: draws of the alias table, 3: the HDRI)", dev_index);
    if (environment_index >= ctx->envs.size() || !ctx->envs[environment_index].rgba) return fail(ctx, RSRT_ERR_NOT_READY, "debug_view: environment slot %u is empty", environment_index);
    const Env &e = ctx->envs[environment_index];
    const size_t n = ctx->acc.pixels();
    if (!host_inout || n_halfs != n * 4) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "debug_view: expected %zu halfs", n * 4);
    return read_back(ctx, host_inout, n * sizeof(ushort4), n * sizeof(uint32_t), [&](void *scratch) {
        ushort4 *tex = static_cast<ushort4 *>(scratch);
        uint32_t *counts = reinterpret_cast<uint32_t *>(tex + n);
        const unsigned nb = (unsigned)((n + 255) / 256);
        if (dev_index == 3u) {
            hipLaunchKernelGGL(rt_dev_view_hdri_kernel, dim3(nb), dim3(256), 0, ctx->stream, e.rgba, e.width, e.height, ctx->acc.w, ctx->acc.h, tex);
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(tex, host_inout, n * sizeof(ushort4), hipMemcpyHostToDevice, ctx->stream)); // out_texture as the last frame left it
            HIP_TRY(ctx, hipMemsetAsync(counts, 0, n * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(rt_dev_view_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, e.alias, e.width, e.height, ctx->acc.w, ctx->acc.h, sample_count, counts);
            hipLaunchKernelGGL(rt_dev_view_apply_kernel, dim3(nb), dim3(256), 0, ctx->stream, counts, n, tex);
        }
        return RSRT_OK;
    });
}

rsrt_status rsrt_display_srgb8(rsrt_context *ctx, uint32_t sample_total, uint8_t *host_rgba8, size_t n_bytes)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    return image_display(ctx, "display_srgb8", IMAGE_MEAN, sample_total, host_rgba8, n_bytes);
}

rsrt_status rsrt_render(rsrt_context *ctx, const rsrt_camera *camera, uint32_t width, uint32_t height, uint32_t sample_begin,
                        uint32_t sample_count, uint32_t max_bounces, uint32_t environment_index, uint32_t flags, void *hip_stream)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!camera) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if (environment_index >= ctx->envs.size() || !ctx->envs[environment_index].rgba) return fail(ctx, RSRT_ERR_NOT_READY, "environment %u not uploaded", environment_index);
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "bad resolution %ux%u", width, height);
    if ((uint64_t)sample_begin + sample_count > 0xffffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "sample range overflows u32");
    if (flags & ~(uint32_t)(RSRT_FLAG_REFERENCE_TRAVERSAL | RSRT_FLAG_PRUNE)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
    rsrt_status st = ensure_accumulator(ctx, width, height);
    if (st) return st;
    if (ctx->pending_events.size() + ctx->pending_reduce.size() >= 32) { st = collect_events(ctx); if (st) return st; } // bounds the event pool
    if (sample_count == 0) return RSRT_OK;

    RenderParams P;
    memset(&P, 0, sizeof P);
    P.scene = ctx->scene;
    const Env &env = ctx->envs[environment_index];
    P.env.rgba = env.rgba; P.env.alias = env.alias; P.env.width = env.width; P.env.height = env.height;
    P.env.wf = (float)env.width;
    P.env.hf = (float)env.height;
    P.env.dphi_dtheta = (RT_TWO_PI / (float)env.width) * (RT_PI / (float)env.height);
    P.env.width_shift = (env.width & (env.width - 1)) == 0 ? (uint32_t)__builtin_ctz(env.width) : 0xffffffffu;
    memcpy(P.cam_pos, camera->pos, 12);
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) P.cam_rot[3 * j + k] = camera->rot_transform[j][k];
    P.fov_y = camera->fov_y;
    P.width = width; P.height = height;
    P.max_bounces = max_bounces; P.flags = flags;
    P.tile_w = ctx->tile_w; P.tile_h = ctx->tile_h;
    P.tiles_x = (width + P.tile_w - 1) / P.tile_w;
    const uint32_t tiles_y = (height + P.tile_h - 1) / P.tile_h;
    P.n_tiles = P.tiles_x * tiles_y;
    P.rank = ctx->rank; P.world = ctx->world;
    P.skew = partition_skew(P.world);
    P.tiles_per_row = (P.tiles_x + P.world - 1) / P.world;
    P.n_owned_tiles = tiles_y * P.tiles_per_row; // tile slots, the same for every rank (some may be padding, see owned_tile)
    const uint32_t tile_px = P.tile_w * P.tile_h;
    if ((uint64_t)P.n_owned_tiles * tile_px > 0x7fffffffull) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "frame too large");
    P.n_slots = P.n_owned_tiles * tile_px;
    P.descend_quorum = kDescendQuorum;
    P.flat_quorum = ctx->flat_quorum;
    P.stop_quorum = kStopQuorum;
    P.stats = ctx->dev_stats;
    if (P.n_slots == 0) return RSRT_OK;

    // sample buffer: [samples of this pass][slot][3]; passes bound its size
    const size_t budget = ctx->sample_buffer_budget;
    const size_t per_sample = (size_t)P.n_slots * 3 * sizeof(float);
    uint32_t pass_samples = (uint32_t)std::max<size_t>(1, std::min<size_t>(sample_count, budget / per_sample));
    pass_samples = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(pass_samples, 0xffffffffull / P.n_slots)); // slot ids are 32-bit
    const size_t need = per_sample * pass_samples;

    const int trav = select_traversal(ctx, P.scene, max_bounces, flags);
    int sv = P.scene.lds_float4s != 0 ? 1 : 0;
    if (sv == 0 && ctx->allow_hybrid) { // mid-size scene: what the chosen traversal's box steps touch, in LDS
        if (hybrid_stage(ctx, P.scene, trav, trav == 6 ? kCoopRoomF4 : kHybridRoomF4)) sv = 2;
    }
    // measured on suzanne and the 15 k-triangle grid (profiles/r02_bvh_knobs.txt): with the quorum vote a round is short, and
    // handing the slot back to the scheduler after about one round beats running several rounds with thinning lanes
    P.trace_budget = ctx->trace_budget ? ctx->trace_budget : (trav >= 4 ? 4u : (trav == 3 ? 6u : 12u)); // (wide walk: rounds, not steps)
    P.coop_lds_cap = ctx->coop_lds_cap;
    P.coop_lifo_at = ctx->coop_lifo_at;
    P.coop_narrow_at = ctx->coop_narrow_at;
    P.coop_gcap = ctx->coop_gcap;
    // a small job behind a kernel that is still running: the small form, kPipeBlocks workgroups per CU, on one of the lanes (see Lane)
    bool pipelined = false;
    if (!ctx->small_form && sv == 1 && trav != 6 && (uint64_t)P.n_slots * sample_count <= kSmallPaths && sample_count <= pass_samples)
        for (auto &L : ctx->lanes) pipelined = pipelined || (L.traced_valid && hipEventQuery(L.traced) == hipErrorNotReady);
    const bool small = ctx->small_form || pipelined;
    const bool big = !small && sv == 1 && trav != 6; // one workgroup per CU shares the scene copy
    const uint32_t pool = trav == 6 ? RT_COOP_POOL : (sv == 2 ? RT_WALK_POOL : (big ? RT_BIG_POOL : 160u));
    const uint32_t block = (sv == 2 && trav == 6) ? (uint32_t)RT_COOP_BLOCK : ((sv == 2 || big) ? 1024u : (uint32_t)RT_BLOCK);
    const size_t smem = (size_t)P.scene.lds_float4s * sizeof(float4) + (size_t)(block / RT_WAVE) * 4u * pool_wave_lds_dwords(trav, pool);
    if (smem > 160 * 1024) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "kernel needs %zu bytes of LDS (> 160 KiB): bvh too deep for this pool size", smem);
    const void *kfn = variant_function(small, sv, trav);
    if (pipelined && !ctx->hw_queue_warned && ctx->hw_queues < (int)kLanes + 1) { // (the lanes' streams and the caller's)
        ctx->hw_queue_warned = true;
        fprintf(stderr, "librsrt: pipelining single-sample calls over %u streams on %d hardware queues: set GPU_MAX_HW_QUEUES=8 before the first HIP call (INTEGRATION.md)\n",
                kLanes, ctx->hw_queues);
    }
    int pipe_blocks = kPipeBlocks;
    int &bpc = pipelined ? pipe_blocks : ctx->blocks_per_cu[sv * 7 + trav];
    if (bpc == 0) {
        int nb = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kfn, (int)block, smem);
        if (e != hipSuccess || nb <= 0) nb = 1;
        bpc = std::min(nb, 8);
    }

    const size_t need_cold = (size_t)ctx->cus * bpc * (block / RT_WAVE) * pool_wave_cold_dwords(trav, pool) * sizeof(uint32_t); // cold path-state arena: one block (rt_cold_layout.h: the walks' columns, the flat kernel's 64-byte records) per wave that can be resident
    // the context's buffers are shared by every call: enqueue_pass orders each resolve after whatever ran last (another stream's
    // render, rsrt_accumulator_clear on the context's own stream, ...)
    rsrt_context::Lane *last_lane = nullptr;
    for (uint32_t done = 0; done < sample_count; done += pass_samples) {
        P.sample_begin = sample_begin + done;
        P.sample_count = std::min(pass_samples, sample_count - done);
        uint32_t li = 0; // ordinary jobs: lane 0, one after the other (a frame's kernel time is then its own, not its neighbour's too)
        if (pipelined) { li = ctx->next_small_lane; ctx->next_small_lane = (li + 1u) % kLanes; }
        else ctx->next_small_lane = 1u;
        rsrt_context::Lane &lane = ctx->lanes[li];
        if (need > lane.sample_buf_bytes || need_cold > lane.cold_bytes) { // (grow-only; a reallocation waits for everything in flight)
            if ((st = sync_all(ctx))) return st;
            if (need > lane.sample_buf_bytes) {
                if (lane.sample_buf) { (void)hipFree(lane.sample_buf); lane.sample_buf = nullptr; lane.sample_buf_bytes = 0; }
                HIP_TRY(ctx, hipMalloc(&lane.sample_buf, need));
                lane.sample_buf_bytes = need;
            }
            if (need_cold > lane.cold_bytes) {
                if (lane.cold_state) { (void)hipFree(lane.cold_state); lane.cold_state = nullptr; lane.cold_bytes = 0; }
                HIP_TRY(ctx, hipMalloc(&lane.cold_state, need_cold));
                lane.cold_bytes = need_cold;
            }
        }
        P.sample_buf = lane.sample_buf;
        P.cold_state = lane.cold_state;
        P.work_counter = lane.work_counter;
        rsrt_context::PassEvents pe = {get_event(ctx), get_event(ctx), get_event(ctx)};
        const rsrt_status pst = enqueue_pass(ctx, P, pe, kfn, block, bpc, smem, per_sample, max_bounces, stream, lane);
        if (pst != RSRT_OK) { // nothing of this pass is pending: the three events go back to the pool
            ctx->event_pool.push_back(pe.begin); ctx->event_pool.push_back(pe.traced); ctx->event_pool.push_back(pe.end);
            // earlier passes may be in flight: the chain's end stays where the last successful pass recorded it (its lane's
            // resolve); recording it on the caller's stream here would drop the dependency on those resolves
            return pst;
        }
        ctx->pending_events.push_back(pe);
        last_lane = &lane;
    }
    // a caller that named a stream of its own gets that stream's semantics: what it enqueues there next comes after this render
    if (hip_stream && last_lane) HIP_TRY(ctx, hipStreamWaitEvent(stream, last_lane->resolved, 0));
    return RSRT_OK;
}

rsrt_status rsrt_synchronize(rsrt_context *ctx)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    return sync_all(ctx);
}

rsrt_status rsrt_get_stats(rsrt_context *ctx, rsrt_stats *out)
{
    if (!ctx || !out) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = collect_stats(ctx);
    if (st) return st;
    *out = ctx->stats;
    return RSRT_OK;
}

// Exhaustive check of rt_rcp against the compiler's correctly rounded division, all 2^32 bit patterns.
__global__ void rt_selftest_rcp_kernel(unsigned long long *out)
{
    unsigned long long bad = 0, raw_differs = 0, fast_path = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = as_f((uint32_t)i);
        const float ref = 1.0f / x;
        if (as_u(rt_rcp(x)) != as_u(ref)) {
            bad++;
            atomicMin(&out[3], (unsigned long long)i);
        }
        const uint32_t ex = ((uint32_t)i >> 23) & 0xffu;
        if (ex - 2u < 251u) {
            fast_path++;
            if (as_u(__builtin_amdgcn_rcpf(x)) != as_u(ref)) raw_differs++; // sanity: the Newton step is doing something
        }
    }
    atomicAdd(&out[0], bad);
    atomicAdd(&out[1], fast_path);
    atomicAdd(&out[2], raw_differs);
}

// Exhaustive check of rsrt_sincosf against rsrt_sinf and rsrt_cosf, as bits, all 2^32 bit patterns.
__global__ void rt_selftest_sincos_kernel(unsigned long long *out)
{
    unsigned long long bad = 0, checked = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = as_f((uint32_t)i);
        float s, c;
        rsrt_sincosf(x, &s, &c);
        checked++;
        if (as_u(s) != as_u(rsrt_sinf(x)) || as_u(c) != as_u(rsrt_cosf(x))) {
            bad++;
            atomicMin(&out[3], (unsigned long long)i);
        }
    }
    atomicAdd(&out[0], bad);
    atomicAdd(&out[1], checked);
}

static rsrt_status run_selftest(rsrt_context *ctx, void (*kernel)(unsigned long long *), uint64_t out[4])
{
    if (!ctx || !out) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    unsigned long long *d = nullptr, h[4] = {0, 0, 0, ~0ull};
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    HIP_TRY(ctx, hipMalloc(&d, sizeof h));
    hipError_t e = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3(ctx->cus * 8), dim3(256), 0, ctx->stream, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(ctx, RSRT_ERR_HIP, "selftest: %s", hipGetErrorString(e));
    for (int i = 0; i < 4; i++) out[i] = h[i];
    return RSRT_OK;
}

rsrt_status rsrt_selftest_numerics(rsrt_context *ctx, uint64_t out[4]) { return run_selftest(ctx, rt_selftest_rcp_kernel, out); }
rsrt_status rsrt_selftest_sincos(rsrt_context *ctx, uint64_t out[4]) { return run_selftest(ctx, rt_selftest_sincos_kernel, out); }

rsrt_status rsrt_get_debug_counters(rsrt_context *ctx, uint64_t out[32])
{
    if (!ctx || !out) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    rsrt_status st = collect_stats(ctx);
    if (st) return st;
    for (int i = 0; i < 32; i++) out[i] = ctx->debug_words[i];
    return RSRT_OK;
}

// The cooperative walk's counters (rt_coop.h CoopCount), cumulative since the context was created; read on their own, so that the
// rsrt_get_stats window is not touched.
rsrt_status rsrt_get_walk_counters(rsrt_context *ctx, uint64_t *out, uint32_t n)
{
    if (!ctx || (!out && n != 0)) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    unsigned long long c[RT_COOP_NSTATS];
    HIP_TRY(ctx, hipMemcpy(c, ctx->dev_stats + RT_COOP_STATS, sizeof c, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n && i < RT_COOP_NSTATS; i++) out[i] = c[i];
    for (uint32_t i = RT_COOP_NSTATS; i < n; i++) out[i] = 0;
    return RSRT_OK;
}

rsrt_status rsrt_get_region_counters(rsrt_context *ctx, uint64_t out[32])
{
    if (!ctx || !out) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    for (int i = 0; i < 32; i++) out[i] = 0;
#ifdef RT_INSTRUMENT
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    unsigned long long h[32], z[32] = {0};
    HIP_TRY(ctx, hipMemcpyFromSymbol(h, HIP_SYMBOL(rt_region_lanes), sizeof h));
    HIP_TRY(ctx, hipMemcpyToSymbol(HIP_SYMBOL(rt_region_lanes), z, sizeof z));
    for (int i = 0; i < 32; i++) out[i] = h[i];
#endif
    return RSRT_OK;
}

rsrt_status rsrt_cast_rays(rsrt_context *ctx, uint32_t n, const float *origins, const float *dirs, uint32_t mode, uint32_t flags,
                           rsrt_hit *out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!ctx->scene_ready) return fail(ctx, RSRT_ERR_NOT_READY, "no scene uploaded");
    if (n == 0) return RSRT_OK;
    if (!origins || !dirs || !out || mode > 31 || ((mode >> 1) & 7u) > 6u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: bad arguments");
    // mode: bit 0 = cast_ray_bvh only; bits 1-3 = traversal (0 threaded, 1 stack, 2 typed leaf loops, 3 flat, 4 fixed-order, 5 wide, 6 cooperative wide);
    // bit 4 = scene read from LDS exactly as the production kernel stages it for that traversal (whole image, or for a
    // mid-size scene the nodes + escape links / the pre-order nodes)
    DevScene sc = ctx->scene;
    const uint32_t sel = (mode >> 1) & 7u;
    const int trav = sel == 0 ? 0 : (sel == 1 ? 4 : (sel == 2 ? 1 : (sel == 3 ? 2 : (sel == 4 ? 3 : (sel == 5 ? 5 : 6))))); // (probe numbering: 4 = stack walk, 5 = wide walk, 6 = cooperative wide walk)
    const size_t coop_lds = trav == 6 ? (size_t)(RT_BLOCK / RT_WAVE) * 4u * pool_wave_lds_dwords(6, 64u) : 0u; // the probe's four one-column pools with their stacks
    int sv = 0;
    if (mode & 16u) {
        if (sc.lds_float4s != 0) {
            sv = 1;
        } else {
            // (what the production kernel stages for that traversal — the probe has no pools beside it; only the stack walk needs a stack)
            const uint32_t all_f4 = 160u * 1024u / (uint32_t)sizeof(float4);
            const uint32_t stack_f4 = trav == 4 ? (uint32_t)(((size_t)sc.stack_entries * RT_BLOCK * sizeof(uint32_t) + 15u) / 16u) : 0u;
            const uint32_t coop_f4 = (uint32_t)((coop_lds + 15u) / 16u);
            if (!hybrid_stage(ctx, sc, trav == 5 ? 4 : (trav == 4 ? 0 : trav), all_f4 > stack_f4 + coop_f4 ? all_f4 - stack_f4 - coop_f4 : 0u))
                return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: this scene is not staged in LDS by the production kernel");
            sv = 2;
        }
    } else {
        sc.lds_float4s = 0;
    }
    if (trav == 6 && !(sc.wide_ok && sc.coop_ok)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: the cooperative walk needs what the wide walk needs, fewer than 2^21 records and 2^24 wide nodes");
    if (trav == 5 && !sc.wide_ok) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: the wide walk needs nested boxes, leaves of at most 8 primitives that share no record, and a wide tree of at most 25 levels");
    if ((trav == 1 || trav == 3) && !sc.typed_leaves) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: typed leaf loops need leaves of at most 8 primitives");
    if (trav == 2 && (!sc.flat_ok || sv == 2)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: the flat traversal needs a scene of at most 64 records with nested boxes");
    { rsrt_status st0 = sync_all(ctx); if (st0) return st0; }
    float *d_o = nullptr, *d_d = nullptr;
    rsrt_hit *d_h = nullptr;
    uint32_t *d_g = nullptr; // (cooperative walk: the waves' overflow blocks)
    const uint32_t n_blocks = (n + RT_BLOCK - 1) / RT_BLOCK;
    hipError_t e = hipMalloc(&d_o, (size_t)n * 12);
    if (e == hipSuccess && trav == 6) e = hipMalloc(&d_g, (size_t)n_blocks * (RT_BLOCK / RT_WAVE) * RT_COOP_GCAP * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_d, (size_t)n * 12);
    if (e == hipSuccess) e = hipMalloc(&d_h, (size_t)n * sizeof(rsrt_hit));
    if (e == hipSuccess) e = hipMemcpy(d_o, origins, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_d, dirs, (size_t)n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const size_t smem = (size_t)sc.lds_float4s * sizeof(float4) + (trav == 4 ? (size_t)sc.stack_entries * RT_BLOCK * sizeof(uint32_t) : 0u) + coop_lds; // (only the stack walk has a stack)
        if (smem > 160 * 1024) { (void)hipFree(d_o); (void)hipFree(d_d); (void)hipFree(d_h); (void)hipFree(d_g); return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "cast_rays: needs %zu bytes of LDS", smem); }
        uint32_t repeat = ctx->probe_repeat;
        void *kargs[] = {&sc, &n, &d_o, &d_d, &mode, &flags, &repeat, &d_h, &d_g, &ctx->coop_lds_cap, &ctx->coop_lifo_at, &ctx->coop_narrow_at, &ctx->coop_gcap,
                         &ctx->dev_stats}; // (from d_g on: the cooperative walk's probe only)
        e = hipLaunchKernel(probe_function(sv, trav), dim3(n_blocks), dim3(RT_BLOCK), kargs, smem, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_h, (size_t)n * sizeof(rsrt_hit), hipMemcpyDeviceToHost);
    (void)hipFree(d_o); (void)hipFree(d_d); (void)hipFree(d_h); (void)hipFree(d_g);
    if (e != hipSuccess) return fail(ctx, RSRT_ERR_HIP, "cast_rays: %s", hipGetErrorString(e));
    return RSRT_OK;
}

} // extern "C"

#include "rsrt_comm.h"
#include "rt_denoise.h"
#include "rt_temporal.h"
#include "rt_variance.h"
#include "rt_upsample.h"
#include "rt_noise.h"
#include "rt_exposure.h"
#include "rt_bloom.h"
#include "rt_local.h"
#include "rt_dof.h"
#include "rt_sky.h"
#include "rt_colour.h"
#include "rt_motion.h"
#include "rt_fog.h"
#include "rt_finish.h"
#include "rt_hdr.h"
#include "rt_video.h"
#include "rt_jpeg.h"
