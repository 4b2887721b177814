"""A context that lives: cases and helpers of tests/test_lifecycle.py (no GPU: the cases reach what they aim at) and
tests/test_lifecycle_gpu.py (one rsrt_context across scene, size, tile, accumulator and environment changes), in the manner of
tests/edge_scenes.py.  Nearly every other GPU test builds a State, uploads one scene, sets one size, renders and closes; the integration
keeps ONE context for the whole program, resizes it on every window event and uploads again on every scene change.  What that
leaves behind in the context — device pointers and counts of the old scene, the occupancy cache, grow-only work buffers sized by
whichever scene asked first, scratch shared by kernels with different layouts — is what the chains here walk through.

Every image is the checker's, computed once per (scene, environment, size, sample range, bounce limit) and shared read-only.

Part A, the chain of scenes (CHAIN): every kernel class boundary in both directions —
  default       flat loop, whole image in LDS
  suzanne       cooperative walk, a prefix of the wide nodes staged in LDS
  long_leaf     util.long_leaf_scene(): leaves of more than 8 records, so no wide tree and no typed leaf loops.  Its 22 records in two
                leaves still qualify for the FLAT loop, which takes any leaf length; the step renders with max_bounces 0x10000, one
                more than the flat loop's 16-bit bounce field holds (rt_wavepool.h RT_FLAT_MAX_BOUNCES), and so gets the generic tree
                walk (paths of this open scene end by escape long before: the image is that of any large limit)
  deck          util.deck_scene(DECK_LEVELS): 42 levels, not the builder's default 14 — 14 levels are 28 records, which the flat loop
                takes, under a wide tree of 5 levels; 42 are 84 records (no flat loop) under 15 wide levels, more than the wide walk's
                eight stack registers serve (wide_deep); its whole image fits LDS: the walk's 256-thread form
  big           util.big_scene(dir, 4): 15,488 triangles, 2,064 wide nodes of which the launch stages the first 160
  cube, spheres_only, default   flat again, the smallest blob behind the largest."""
import collections
import functools
import os
import re

import numpy as np

import denoise_ref as D
import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import partition, types as T

INVALID, NOT_READY = 1, 4  # rsrt_status
MB = 4                     # max_bounces wherever a step does not say otherwise
DECK_LEVELS = 42
TOO_DEEP_LEVELS = 140      # deck_scene of this many levels: a valid tree, 141 stack entries x 256 lanes x 4 bytes > the 128 KiB rsrt_upload_scene allows
COOP_REFUSED = "the cooperative walk needs what the wide walk needs"

# ---------------------------------------------------------------------------------------------------- scenes, environments, images
_scenes = {}


def scene(name, out_dir=None):
    """The scene called `name`, built once.  "big" is written as files first: the first caller passes a directory of its own."""
    if name not in _scenes:
        if name == "long_leaf":
            _scenes[name] = util.long_leaf_scene()
        elif name == "deck":
            _scenes[name] = util.deck_scene(DECK_LEVELS)
        elif name == "big":
            assert out_dir is not None, "the big scene is built by whoever holds a temporary directory"
            _scenes[name] = R.Scene.load_toml(util.big_scene(out_dir, 4))
        else:
            _scenes[name] = R.Scene.load_toml(util.scene_path(name))
    return _scenes[name]


ENVS = {"small": (64, 32), "odd": (100, 37), "tiny": (8, 4)}  # util.small_env sizes; "odd" is edge_scenes.odd_env()


def env(name):
    return util.small_env(*ENVS[name])


def camera(sc):
    return np.array(sc.camera_uniform()).view(T.CAMERA).reshape(1).copy()


@functools.lru_cache(maxsize=None)
def reference(scene_name, env_name, w, h, begin, count, mb=MB, fast=False):
    """The checker's image sums and counters (callers must not write into them)."""
    sc = scene(scene_name)
    img, st = oracle.render(util.oracle_scene(sc), util.oracle_env(env(env_name)), camera(sc).view(oracle.CAMERA), w, h, begin, count, mb, fast=fast)
    img.setflags(write=False)
    return img, st


def counters(st):
    return st["paths"], st["ext_rays"], st["shadow_rays"]


# ---------------------------------------------------------------------------------------------------- A: the chain of scenes
Step = collections.namedtuple("Step", "scene klass max_bounces env_index sels lds_sels")
ALL, WALKS = (0, 1, 2, 3, 4, 5, 6), (0, 1, 2, 4, 5, 6)  # rsrt_cast_rays traversal selectors (util.probe_modes): 3 is the flat loop
CHAIN_ENVS = ("small", "odd")  # slots 0 and 1 of the chain's context; the steps alternate
W, H, SPP = 48, 32, 2
CHAIN = [Step("default", "flat", MB, 0, ALL, ALL),
         Step("suzanne", "coop", MB, 1, WALKS, WALKS),
         Step("long_leaf", "generic", 0x10000, 0, (0, 1, 3), (0, 1, 3)),  # (typed leaf loops and wide walks refuse leaves of more than 8 records)
         Step("deck", "coop", MB, 1, WALKS, WALKS),
         # (of this scene the production kernels stage a prefix of the wide nodes — selectors 5 and 6 — or of the fixed-order walk's
         # elements — 4; nodes + escape links of 8,731 nodes are 0.5 MiB, above the 40 KiB the tree walks 0, 1, 2 would have staged:
         # their LDS form is refused, BIG_LDS_REFUSED)
         Step("big", "coop", MB, 0, WALKS, (4, 5, 6)),
         Step("cube", "flat", MB, 1, ALL, ALL),
         Step("spheres_only", "flat", MB, 0, ALL, ALL),
         Step("default", "flat", MB, 1, ALL, ALL)]
REFUSED_AFTER = 1  # the refused uploads come behind this step (suzanne)
BIG_LDS_REFUSED = [(sel << 1) | 16 | bvh_only for sel in (0, 1, 2) for bvh_only in (0, 1)]
NOT_STAGED = "this scene is not staged in LDS by the production kernel"


def step_reference(step):
    return reference(step.scene, CHAIN_ENVS[step.env_index], W, H, 0, SPP, step.max_bounces)


def probe_modes(step):
    """Every way rsrt_cast_rays runs a query on the step's scene: selector x scene from global memory / as staged in LDS x cast_ray / cast_ray_bvh."""
    return [(sel << 1) | lds | bvh_only for sel in step.sels for lds in (0, 16) if not lds or sel in step.lds_sels for bvh_only in (0, 1)]


_Rays = collections.namedtuple("_Rays", "camera sample_begin")


@functools.lru_cache(maxsize=None)
def probe(scene_name):
    """(origins, directions, {bvh_only: the checker's hit records as [n, 9] words}): 6 rows of camera rays and the centre ray, 55 in all."""
    sc = scene(scene_name)
    o, d = E.probe_rays(_Rays(camera(sc), 0), n=6)
    osc = util.oracle_scene(sc)
    return o, d, {b: oracle.cast_rays(osc, o, d, b, 0).view(np.uint32).reshape(-1, 9) for b in (0, 1)}


def out_of_range_copy(sc):
    """sc with the first triangle's first vertex index one past the vertex array."""
    bad = R.Scene(sc.materials, sc.spheres, sc.plane_descs, sc.vertices, sc.normals, sc.triangles.copy(), sc.camera_desc,
                  planes=sc.planes, primitives=sc.primitives, bvh_nodes=sc.bvh_nodes, bvh_depth=sc.bvh_depth)
    bad.triangles["vertex_0"][0] = len(sc.vertices)
    return bad


# ---------------------------------------------------------------------------------------------------- B: the chain of sizes
SIZES = [(64, 40), (16, 16), (1, 1), (200, 120), (64, 40), (7, 300)]  # (w, h): shrink, the smallest, grow past everything before, a size again, tall and thin
SIZE_ENVS = ("small", "odd")


@functools.lru_cache(maxsize=None)
def dev_view(env_name, index, w, h, sample_count):
    out = oracle.debug_view(index, util.oracle_env(env(env_name)), w, h, sample_count)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def aov_reference(scene_name, w, h, begin, count):
    sc = scene(scene_name)
    out = D.aov_records(sc, util.oracle_scene(sc), camera(sc)[0], w, h, begin, count)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- C: tile shapes
TILES = [(64, 1), (1, 64), (8, 8), (4, 16), (32, 2), (64, 64), (128, 32)]  # (w, h)
WORLDS = {1: 3, 2: 3, 3: 5, 5: 3}  # world size -> skew
FRAMES = [(100, 37), (65, 129), (40, 40)]  # the last: smaller than one 64 x 64 tile, rendered with that tile only
RANGES = [(0, 1), (3, 6)]  # (begin, count): one sample, which enqueue_pass cuts into sub-tiles where the tile allows; [3, 9), six sample blocks.
# (At these frame sizes a job is far below 32 chunks a resident wave, so enqueue_pass keeps ONE sample a chunk: six blocks of one, and
# the remainder branch of its block count — a sample count that is no multiple of the samples per chunk — is out of reach of part C.)
REJECTED_TILES = [(10, 10), (0, 16), (128, 64)]  # 100 pixels are no whole waves; empty; 8192 pixels
TILE_SCENES = ("default", "suzanne")


def tiles_of(frame):
    return [(64, 64)] if frame == (40, 40) else TILES


def tile_cases(frame):
    return [(tw, th, world, rank) for tw, th in tiles_of(frame) for world in WORLDS for rank in range(world)]


# ---------------------------------------------------------------------------------------------------- header constants
def header_define(name, header):
    """#define `name` of csrc/hip/`header`, as an integer (a `u` suffix dropped)."""
    text = open(os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip", header)).read()
    m = re.search(r"^\s*#\s*define\s+%s\s+\(?(0x[0-9a-fA-F]+|\d+)u?\b" % name, text, re.M)
    assert m, (name, header)
    return int(m.group(1), 0)


def coop_room_float4s():
    """kCoopRoomF4 of rsrt_api.hip: the LDS (160 KiB a workgroup) left beside the cooperative walk's pools, in 16-byte units —
    (160 KiB - RT_COOP_BLOCK / 64 waves x 4 bytes x pool_wave_lds_dwords(6, RT_COOP_POOL)) / 16, where rt_wavepool.h has
    pool_wave_lds_dwords(6, pool) = 12 hot columns x pool + RT_COOP_LCAP + RT_COOP_NCAP + RT_COOP_MAP.  A wide node is 8 float4."""
    pool, block = header_define("RT_COOP_POOL", "rsrt_api.hip"), header_define("RT_COOP_BLOCK", "rsrt_api.hip")
    wave_dwords = 12 * pool + sum(header_define(n, "rt_coop.h") for n in ("RT_COOP_LCAP", "RT_COOP_NCAP", "RT_COOP_MAP"))
    return (160 * 1024 - (block // 64) * 4 * wave_dwords) // 16
