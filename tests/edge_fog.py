"""Edge inputs of the fog march (rsrt_fog_render, csrc/hip/rt_fog.h): named cases of (scene, camera record, w, h, sample_begin,
sample_count, fog parameters), in the manner of tests/edge_images.py and tests/edge_scenes.py.  The march makes rays of its own — its
points are the origins of shadow rays along light_dir — so it meets the scene walkers' edges from another side than rsrt_render's ray
generator does.  Three families:
  scene   every case of tests/edge_scenes.py under one slanted light: scaled geometry (with the medium scaled along where the checker
          still records hits), cameras inside and on surfaces and along the poles, one-pixel-wide frames;
  tree    trees the walk must take as they are: the builders' degenerate ones (tests/edge_trees.py TRAVERSED), leaves of eleven records,
          the chain trees, and the hand-edited BVHs of tests/foreign_trees.py — boxes that do not nest, a shared record, a twin in
          another leaf, 60 spheres no leaf holds (the closest hit's fallback finds them, the shadow query does not);
  param   the ends of what rsrt_fog_params_ok accepts, on default and house: axis-parallel lights (1 / light_dir = +-inf, the slab
          test's 0 * inf), a light at either end of the accepted length, g = 0 and +-0.95, albedo 0, density 0, 1e6 and one whose
          transmittance reaches rsrt_sky_exp2's clamp part-way along a march, max_distance 1e-30, 1e-44 and the largest float (march
          points up to 3e38 units away), steps 1, 63 and 64; each with the jitter off and on.
test_fog_edges.py shows from the restatement (tests/fog_ref.py) that the cases reach their edges and stay finite; test_fog_edges_gpu.py
holds the kernel to the restatement bit for bit."""
import collections
import functools

import numpy as np

import edge_scenes as ES
import edge_trees as ET
import fog_ref
import foreign_trees
import util
from rsoderh_raytracing_amd import types as T

F = np.float32
BEGIN, COUNT = 3, 2  # every case's sample range
STEPS = 4            # unless the case is about steps
SLANT = fog_ref.unit((0.4, 0.6, -0.7))
LARGEST = float(fog_ref.LARGEST)
# the medium of the scene and tree families, and what the parameter family varies: three different channels, some ambient light
MEDIUM = dict(light_dir=SLANT, light_irradiance=(4.0, 3.0, 2.0), ambient=(0.02, 0.03, 0.05), albedo=(0.9, 0.8, 0.7), max_distance=20.0, steps=STEPS)
# rsrt_sky_exp2 returns exactly 0 below -EXP2_CLAMP (tests/sky_ref.py exp2; test_fog_edges.py checks this value against it).  With
# sigma' * 10 = EXP2_CLAMP a march of length 20 has its points beyond t = 10 at transmittance exactly 0 and the nearer ones above it.
EXP2_CLAMP = 126.0
CLAMP_DENSITY = float(F(EXP2_CLAMP / (10.0 * float(fog_ref.LOG2E))))

Case = collections.namedtuple("Case", "name family scene camera w h sample_begin sample_count params")

PARAM_SCENES = {"default": (24, 16), "house": (32, 18)}
LIGHTS = {"light_+y": (0.0, 1.0, 0.0), "light_-0+y-0": (-0.0, 1.0, -0.0), "light_+x": (1.0, 0.0, 0.0), "light_-y": (0.0, -1.0, 0.0), "light_-z": (0.0, 0.0, -1.0),
          "light_long_+x": (1.0004, 0.0, 0.0), "light_short_-y": (0.0, -0.9996, 0.0)}
AXIS_PARALLEL = ("light_+y", "light_-0+y-0", "light_+x", "light_-y", "light_-z", "light_long_+x", "light_short_-y")
PARAM_EDGES = dict({k: {"light_dir": v} for k, v in LIGHTS.items()}, **{
    "g_0": {"anisotropy": 0.0}, "g_+0.95": {"anisotropy": 0.95}, "g_-0.95": {"anisotropy": -0.95},
    "albedo_0": {"albedo": 0.0}, "albedo_0_0.5_1": {"albedo": (0.0, 0.5, 1.0)},
    "density_0": {"density": 0.0}, "density_1e6": {"density": 1.0e6}, "density_clamp_midway": {"density": CLAMP_DENSITY},
    "distance_1e-30": {"max_distance": 1.0e-30}, "distance_1e-44": {"max_distance": 1.0e-44},
    "distance_largest_clear_3_steps": {"max_distance": LARGEST, "density": 0.0, "steps": 3},
    "distance_largest_1e-38_7_steps": {"max_distance": LARGEST, "density": 1.0e-38, "steps": 7},
    "steps_1": {"steps": 1}, "steps_63": {"steps": 63}, "steps_64": {"steps": 64}})
FAR = ("distance_largest_clear_3_steps", "distance_largest_1e-38_7_steps")  # march points up to 3e38 units away
CLEAR = ("density_0", "distance_largest_clear_3_steps")                      # density 0: the records are (0, 0, 0, n)


def camera_of(scene):
    return np.array(scene.camera_uniform()).view(T.CAMERA).reshape(1).copy()


def scaled_medium(k):
    """MEDIUM for a scene scaled by 2^k: max_distance times 2^k, density times 2^-k, both exact."""
    s = F(2.0) ** F(k)
    return dict(MEDIUM, max_distance=float(F(20.0) * s), density=float(F(0.05) / s))


# the edge_scenes cases in which the checker still records hits on scaled geometry -> k: the medium is scaled along (ES.SCALE_HIT)
SCALED = {"scale_%s_2^%d" % (n, k): k for n, k in ES.SCALE_HIT}
# ... of which every march point sees the light, under SLANT (test_fog_edges.py asserts exactly these): kept for their march length
SCALED_ALL_LIT = set()

TREES = [(name, lambda name=name: ET.scene(name)) for name in ET.TRAVERSED] + [
    ("long_leaf", util.long_leaf_scene), ("deck_42", lambda: util.deck_scene(42)), ("deck_60", lambda: util.deck_scene(60)),
    ("foreign_shrunken_box", foreign_trees.shrunken_box_scene), ("foreign_shared_record", foreign_trees.shared_record_scene),
    ("foreign_twin_sphere", foreign_trees.twin_sphere_scene), ("foreign_hidden_spheres", foreign_trees.hidden_spheres_scene)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, family, scene, cam, w, h, **over):
        p = fog_ref.params(**dict(MEDIUM, **over))
        out.append(Case(name, family, scene, np.array(cam).view(T.CAMERA).reshape(1).copy(), w, h, BEGIN, COUNT, p))

    for c in ES.cases():
        w, h = (c.w, c.h) if c.family == "shapes" else (min(c.w, 24), min(c.h, 16))
        over = scaled_medium(SCALED[c.name]) if c.name in SCALED else {}
        add("scene_" + c.name + ("_all_lit" if c.name in SCALED_ALL_LIT else ""), "scene", c.scene, c.camera, w, h, **over)
    for name, make in TREES:
        sc = make()
        add("tree_" + name, "tree", sc, camera_of(sc), 24, 16)
    for scene_name, (w, h) in PARAM_SCENES.items():
        sc = ES.plain(scene_name)
        for edge, over in PARAM_EDGES.items():
            for jitter in (0, 1):
                add("param_%s_%s_jitter_%d" % (scene_name, edge, jitter), "param", sc, camera_of(sc), w, h, flags=jitter, **over)
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def family(name):
    return [c for c in cases() if c.family == name]


def names(fam):
    return [c.name for c in family(fam)]


def param_case(scene_name, edge, jitter):
    return case("param_%s_%s_jitter_%d" % (scene_name, edge, jitter))


# ---------------------------------------------------------------------------------------------------- the restatement's view of a case
@functools.lru_cache(maxsize=None)
def reference(name):
    """(records [H, W, 4], lit [sample_count, H, W, steps]) of case `name` from tests/fog_ref.py, computed once; read-only."""
    c = case(name)
    rec, lit = fog_ref.records(util.oracle_scene(c.scene), c.camera[0], c.w, c.h, c.sample_begin, c.sample_count, c.params)
    rec.setflags(write=False)
    lit.setflags(write=False)
    return rec, lit


def shares(lit):
    """(lit, mixed) of reference()'s lit [sample_count, H, W, steps]: the share of march points that see the light, and the share of
    pixels whose march points (of all samples) are neither all lit nor all dark."""
    lit = np.asarray(lit)
    return float(lit.mean()), float((lit.any(axis=(0, 3)) & ~lit.all(axis=(0, 3))).mean())


def march(name):
    """The camera rays, closest hits and march points of case `name`, sample by sample, as fog_ref.records makes them:
    [(o [N, 3], d [N, 3], hits [N] (oracle.HIT), t [N, steps], points [N, steps, 3])], pixels row-major."""
    import denoise_ref
    import oracle
    c = case(name)
    k = fog_ref.prepare(c.params)
    py, px = np.mgrid[0:c.h, 0:c.w]
    px, py = px.reshape(-1), py.reshape(-1)
    out = []
    for s in range(c.sample_begin, c.sample_begin + c.sample_count):
        o, d = denoise_ref.camera_rays(c.camera[0], c.w, c.h, px, py, s)
        xi = fog_ref.jitter(c.w, px, py, s) if k["flags"] & fog_ref.JITTER else np.full(px.size, F(0.5))
        hits = oracle.cast_rays(util.oracle_scene(c.scene), o, d, mode=0)
        dl = fog_ref.delta(k, fog_ref.segment(k, hits["did_hit"] != 0, hits["distance"].astype(F)))
        t = np.stack([fog_ref.t_of(i, xi, dl) for i in range(k["steps"])], axis=1)
        out.append((o, d, hits, t, np.stack([fog_ref.point(o, d, t[:, i]) for i in range(k["steps"])], axis=1)))
    return out


@functools.lru_cache(maxsize=None)
def kernel_form(name):
    """Which form of rt_fog_kernel the case runs: "lds" (the scene's whole image staged in LDS) or "global" — the lds_float4s of
    rsrt_scene_image_build's info, which is what rsrt_upload_scene keeps and the launch reads."""
    from test_scene_image import arrays, build
    built = build(arrays(case(name).scene))
    assert not isinstance(built, str), (name, built)
    return "lds" if built[1].lds_float4s else "global"
