"""Edge inputs of the environment path (sky_light, environment_direction_pdf, sample_environment, the alias tables, the packed pmf
copies of the device layout, the developer views): named cases of (environment map, alias table), in the manner of tests/edge_scenes.py.
Every other rendered test uses the smooth synthetic sky under the table build_by_luminance makes for it; here the maps are tiny, one
texel wide or high, not a power of two, black, spiked, partly negative or very bright, and some tables are the CALLER's: entries that
build_by_luminance would never make, which include/rsrt.h accepts all the same (any in-range alias_index).

  library-built (Environment(rgba): the host builder's table)
    one 1x1, row2 2x1, col2 1x2, quad 2x2   every escaping ray and every pick goes through the clamp-to-edge taps and the u == 1 clamp
    odd6 3x2                                the smallest width that is no power of two (pick / width instead of the shift)
    strip 64x1, pillar 1x37                 one row (both bilinear rows clamp), one column
    spike 5x3                               black but for texel (1, 1): one large entry takes every small one
    black 8x4                               sum 0: every entry stays the default {1, self, 1/N}
    wild 7x5                                one texel in ten negative (weights below zero, probabilities above one)
    bright 6x4                              10^3 .. 10^4.5
    odd_noise 100x37                        an ordinary odd size
  caller-made, on one 5x3 noise map (N = 15)
    uniform      {1, i, 1/N}
    chain        {0.5, (i + 1) % N, (i + 1) / (1 + .. + N)}: a pmf that differs from entry to entry and is NOT what the entries'
                 probabilities imply, so a kernel has to read the pmf of the right entry and cannot derive it
    never_self   {0, (i + 7) % N, the same pmfs}: every pick is the alias target

"noise" is 10 ** uniform(-2, 2) per channel.  Everything is finite, and every case renders finite in the checker (default and suzanne,
48x32, 4 spp, 6 bounces: no NaN, no inf; `wild` has a few negative pixels): reference() asserts it, so a comparison against a
reference that stopped being finite fails instead of passing on NaN == NaN.  Plain data and helpers; no pytest settings."""
import collections
import functools

import numpy as np

import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import types as T

Case = collections.namedtuple("Case", "name env library")  # library: the library's builders made the table

W, H, SPP, BOUNCES = 48, 32, 4, 6  # the rendered frames
SCENES = ("default", "suzanne")    # default: the flat kernel (both packed reads); suzanne: the cooperative walk (the texels' copy only)


def noise(rng, w, h, lo=-2.0, hi=2.0):
    return 10.0 ** rng.uniform(lo, hi, (h, w, 3))


def rgba_of(rgb):
    """[H, W, 3] -> [H, W, 4] float32, alpha 0 (as src/texture.rs writes it)."""
    rgb = np.asarray(rgb, np.float64)
    return np.ascontiguousarray(np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,))], axis=2).astype(np.float32))


def table(probability, alias_index, pmf):
    t = np.zeros(len(alias_index), T.ALIAS_ENTRY)
    t["probability"], t["alias_index"], t["pmf"] = probability, alias_index, pmf
    return t


NOISE_SHAPES = [("one", 1, 1), ("row2", 2, 1), ("col2", 1, 2), ("quad", 2, 2), ("odd6", 3, 2), ("strip", 64, 1), ("pillar", 1, 37)]
CALLER_W, CALLER_H = 5, 3


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for seed, (name, w, h) in enumerate(NOISE_SHAPES):
        out.append(Case(name, R.Environment(rgba_of(noise(np.random.default_rng(100 + seed), w, h))), True))
    spike = np.zeros((3, 5, 3))
    spike[1, 1] = 7.0
    out.append(Case("spike", R.Environment(rgba_of(spike)), True))
    out.append(Case("black", R.Environment(rgba_of(np.zeros((4, 8, 3)))), True))
    rng = np.random.default_rng(110)
    wild = noise(rng, 7, 5)
    negative = rng.uniform(size=(5, 7, 1)) < 0.1
    assert 1 <= int(negative.sum()) <= 7
    out.append(Case("wild", R.Environment(rgba_of(np.where(negative, -wild, wild))), True))
    out.append(Case("bright", R.Environment(rgba_of(noise(np.random.default_rng(111), 6, 4, 3.0, 4.5))), True))
    out.append(Case("odd_noise", R.Environment(rgba_of(noise(np.random.default_rng(112), 100, 37))), True))
    texels = rgba_of(noise(np.random.default_rng(113), CALLER_W, CALLER_H))
    n = CALLER_W * CALLER_H
    i = np.arange(n)
    pmf = ((i + 1) / float(n * (n + 1) // 2)).astype(np.float32)
    out.append(Case("uniform", R.Environment(texels, table(1.0, i, np.float32(1.0) / np.float32(n))), False))
    out.append(Case("chain", R.Environment(texels, table(0.5, (i + 1) % n, pmf)), False))
    out.append(Case("never_self", R.Environment(texels, table(0.0, (i + 7) % n, pmf)), False))
    for c in out:
        assert np.isfinite(c.env.rgba).all() and (c.env.rgba[..., 3] == 0).all() and len(c.env.alias) == c.env.width * c.env.height
        assert (c.env.alias["alias_index"] < len(c.env.alias)).all()
    assert len({c.name for c in out}) == len(out)
    return out


NAMES = ["one", "row2", "col2", "quad", "odd6", "strip", "pillar", "spike", "black", "wild", "bright", "odd_noise", "uniform", "chain", "never_self"]
LIBRARY_NAMES = NAMES[:12]


def case(name):
    return next(c for c in cases() if c.name == name)


def rebuilt(name):
    """Case `name`'s texels under the table build_by_luminance makes for them."""
    return R.Environment(case(name).env.rgba)


# ---------------------------------------------------------------------------------------------------- cameras onto the open sky
def seam_camera(pos, fov_y):
    """A camera whose centre ray (rot * (0, 0, -1)) is EXACTLY (-1, 0, 0), the direction of the u = 0 / u = 1 seam of the map: written
    down like edge_scenes.pole_camera (right (0, 0, -1), up (0, 1, 0), back (1, 0, 0))."""
    cam = np.zeros(1, T.CAMERA)
    cam["pos"][0] = pos
    cam["rot_transform"][0][:, :3] = [(0, 0, -1), (0, 1, 0), (1, 0, 0)]  # columns
    cam["fov_y"] = fov_y
    return cam


# scene `cube` is the cube [-1, 1]^3 alone.  up: nothing but sky around the +y pole; down: from above the cube, its top face in the middle
# (first bounces leave it around +y) and the -y pole around it; seam: along -x just over the cube, the seam in the middle of the image
SKY_CAMERAS = {"pole_up": E.pole_camera((0.0, 1.0, 3.0), True, 1.2), "pole_down": E.pole_camera((0.0, 3.0, 0.0), False, 1.2),
               "seam": seam_camera((4.0, 1.5, 0.0), 1.2)}


# ---------------------------------------------------------------------------------------------------- the checker's view
@functools.lru_cache(maxsize=None)
def reference(env_key, scene_name, camera_name=None):
    """The checker's sums and counters of scene `scene_name` (through SKY_CAMERAS[camera_name], or its own camera) under an
    environment: a case's name, or "rebuilt:<name>".  Computed once; not to be written to.  Finite, or an AssertionError."""
    env = rebuilt(env_key[len("rebuilt:"):]) if env_key.startswith("rebuilt:") else case(env_key).env
    sc = E.plain(scene_name)
    cam = SKY_CAMERAS[camera_name] if camera_name else sc.camera_uniform()
    img, st = oracle.render(util.oracle_scene(sc), util.oracle_env(env), np.asarray(cam).view(oracle.CAMERA), W, H, 0, SPP, BOUNCES)
    assert np.isfinite(img).all(), (env_key, scene_name, camera_name, int((~np.isfinite(img)).sum()))
    img.setflags(write=False)
    return img, st


def counters(st):
    return st["paths"], st["ext_rays"], st["shadow_rays"]
