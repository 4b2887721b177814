"""Edge inputs of the path tracer (rsrt_render, rsrt_cast_rays, rsrt_aov_render, the BVH builders): named cases of (scene, camera,
environment, max_bounces, sample range, image size), in the manner of tests/edge_images.py.  Each case aims at one place where the
shader's arithmetic runs out of range or switches branch: geometry scaled until squared lengths underflow or overflow, materials at and
beyond the upload's clamps, vertex normals that are no unit vectors, cameras inside and on surfaces and along the poles of the
environment map, bounce limits around the flat kernel's 16-bit field, the last sample indices of the u32 range, one-pixel-wide images.
test_scene_edges.py shows from the checker's output that every case reaches its edge; test_scene_edges_gpu.py holds the kernels to it.

Cases whose checker output holds NaN or inf (NaN policy: the same elements must be NaN on the device; the bits equal elsewhere):
  materials_r0 .. r6: inf, no NaN.  Emission 3e38 summed over two samples, or met with a throughput above 1 (colour 1.5), is inf.
  normals_wall: NaN, no inf.  A zero-length vertex normal normalises to NaN (0 * inf), and so does the interpolated normal where two
      opposed vertex normals cancel; every path through such a hit is NaN (42 of 1536 pixels).
The scale family stays finite although its arithmetic does not.  At 2^61 and 2^64 the plane's forward x right overflows, its normal
and base-change matrix are NaN, the triangles' determinants are inf, and at 2^64 the sphere's dot(l, l) is inf as well: the checker then
records no hit (a NaN distance loses every `<`) and the image is the sky; only default's spheres are still hit at 2^61, with squared
distances in the format's last octaves.  At 2^-63 and 2^-70 the same cross product underflows to 0 (normal 0 * inf = NaN), and from
2^-13 or so downwards the shader's own epsilons (t < 1e-4, 1e-5, 1e-3) reject every hit, so the scaled-down scenes are sky too, reached
through subnormal products.
Every other case is finite everywhere (NAN_OR_INF_CASES names the ones that are not)."""
import collections
import functools

import numpy as np

import denoise_ref as D
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host, types as T

F = np.float32
SQRT_001 = F(np.sqrt(np.float64(0.001)))  # roughness whose f32 square is the clamp's neighbourhood (see ROUGHNESS)

NAN_OR_INF_CASES = {"materials_r%d" % i for i in range(7)} | {"normals_wall"}  # the cases listed in the docstring above

Case = collections.namedtuple("Case", "name family scene camera env max_bounces sample_begin sample_count w h")


def odd_env():
    """A non-power-of-two environment for the walk kernels (test_alias_device renders odd ones through the flat kernel only)."""
    return util.small_env(100, 37)


# ---------------------------------------------------------------------------------------------------- scenes
def rebuilt(sc, **over):
    """sc with some arrays replaced; plane uniforms and the BVH made again by the host library."""
    a = dict(materials=sc.materials, spheres=sc.spheres, plane_descs=sc.plane_descs, vertices=sc.vertices, normals=sc.normals,
             triangles=sc.triangles, camera_desc=sc.camera_desc)
    a.update(over)
    return R.Scene(a["materials"], a["spheres"], a["plane_descs"], a["vertices"], a["normals"], a["triangles"], a["camera_desc"])


@functools.lru_cache(maxsize=None)
def scaled_scene(name, k):
    """tests/golden/assets scene `name` with every position, radius, plane vector, vertex and the camera position times 2^k (exact in
    f32 for the k used here: nothing in the inputs leaves the normal range)."""
    sc = R.Scene.load_toml(util.scene_path(name))
    s = F(2.0) ** F(k)
    sph, pls, ver, cam = sc.spheres.copy(), sc.plane_descs.copy(), sc.vertices.copy(), sc.camera_desc.copy()
    sph["pos"] *= s
    sph["radius"] *= s
    for key in ("pos", "forward", "right"):
        pls[key] *= s
    ver["v"] *= s
    cam["pos"] *= s
    for a in (sph["pos"], sph["radius"], pls["pos"], pls["forward"], pls["right"], ver["v"], cam["pos"]):
        assert np.isfinite(a).all() and (np.abs(a[a != 0]) >= F(2.0) ** -126).all()
    return rebuilt(sc, spheres=sph, plane_descs=pls, vertices=ver, camera_desc=cam)


WALL_W, WALL_H = 8.0, 5.0  # the wall of triangles: x in [-4, 4], y in [0, 5], at z = 0, facing +z
WALL_CAMERA = dict(pos=(0.0, 2.5, 7.5), yaw=0.0, pitch=0.0, fov_y=0.765)


def wall_scene(materials, cols, rows, tri_material, tri_normals, skip=0):
    """cols x rows cells; cell c >= skip holds one triangle (material tri_material[c - skip], vertex normals tri_normals[c - skip]:
    [3, 3]); with skip == 2 cell 0 holds a sphere (material 0) and a floor plane in front of the wall has material 1."""
    cw, ch = WALL_W / cols, WALL_H / rows
    n = cols * rows - skip
    assert len(tri_material) == n and len(tri_normals) == n
    ver, nor, tri = np.zeros(3 * n, T.VEC3), np.zeros(3 * n, T.VEC3), np.zeros(n, T.TRIANGLE)
    for t in range(n):
        c = t + skip
        x0, y0 = -WALL_W / 2 + (c % cols) * cw, (c // cols) * ch
        ver["v"][3 * t:3 * t + 3] = [(x0 + 0.05 * cw, y0 + 0.08 * ch, 0), (x0 + 0.95 * cw, y0 + 0.08 * ch, 0), (x0 + 0.5 * cw, y0 + 0.96 * ch, 0)]
        nor["v"][3 * t:3 * t + 3] = tri_normals[t]
        tri[t] = (3 * t, 3 * t + 1, 3 * t + 2, 3 * t, 3 * t + 1, 3 * t + 2, tri_material[t])
    sph, pls = np.zeros(1 if skip else 0, T.SPHERE), np.zeros(1 if skip else 0, T.PLANE_DESC)
    if skip:
        sph["pos"], sph["radius"], sph["material_id"] = (-WALL_W / 2 + 0.5 * cw, 0.5 * ch, 0.0), 0.45 * ch, 0
        pls["pos"], pls["forward"], pls["right"], pls["material_id"] = (-WALL_W / 2, 0.0, 0.0), (0, 0, 6.0), (WALL_W, 0, 0), 1
    return R.Scene(materials, sph, pls, ver, nor, tri, host.make_camera_desc(**WALL_CAMERA))


# the material grid: roughness x metallic x colour x emission.  alpha = max(0.001, roughness^2): SQRT_001 and its f32 neighbours
# square to values just below, at or just above f32(0.001) — which of them does what is asserted in test_scene_edges.py
ROUGHNESS = [F(0.0), np.nextafter(SQRT_001, F(0)), SQRT_001, np.nextafter(SQRT_001, F(1)), F(1.0), F(1.5), F(-0.5)]
METALLIC = [F(0.0), F(1.0), F(-0.25), F(1.75)]
COLOUR = [F(0.0), F(1.0), F(1.5), F(1e-5)]
EMISSION = [F(0.0), F(1e-42), F(3e38), F(-1.0)]


def grid_materials(roughness):
    """The 64 materials metallic x colour x emission of one roughness value.  Colour and emission are tinted (x 1, 0.75, 0.5) so that the
    three channels differ, except where the value itself is the point (0 stays 0; 1e-42 is a subnormal in every channel)."""
    m = np.zeros(64, T.MATERIAL)
    tint = F([1.0, 0.75, 0.5])
    i = 0
    for me in METALLIC:
        for co in COLOUR:
            for em in EMISSION:
                m[i]["color"], m[i]["roughness"], m[i]["metallic"], m[i]["emission"] = co * tint, roughness, me, em * tint
                i += 1
    return m


@functools.lru_cache(maxsize=None)
def material_scene(r_index):
    """A sphere (material 0), a floor plane (1) and 62 triangles (2 .. 63) under one page of the grid: 64 records, so the flat kernel
    takes it by default."""
    z = np.tile(F([0, 0, 1]), (62, 3, 1))
    return wall_scene(grid_materials(ROUGHNESS[r_index]), 8, 8, list(range(2, 64)), z, skip=2)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


NZ_EDGE = [F(0.9985), np.nextafter(F(0.999), F(0)), F(0.999), np.nextafter(F(0.999), F(1)), F(0.9995)]  # around make_frame's switch
NORMAL_SPECS = [("plus_z", [(0, 0, 1)] * 3), ("minus_z_opposed", [(0, 0, -1)] * 3), ("zero", [(0, 0, 0)] * 3),
                ("short_z", [(0, 0, 1e-3)] * 3), ("long_z", [(0, 0, 1e3)] * 3),
                ("short_tilted", [tuple(F(1e-3) * _unit((0.3, 0.2, 0.9)))] * 3), ("long_tilted", [tuple(F(1e3) * _unit((0.3, 0.2, 0.9)))] * 3),
                ("opposed_tilted", [tuple(_unit((0.2, 0.1, -0.97)))] * 3), ("cancelling", [(0, 0, 1), (0, 0, -1), (0, 0, 1)]),
                ("mixed_lengths", [(0, 0, 1e3), (1e-3, 0, 0), (0, 1, 0)])] + \
               [("nz_%d" % i, [(float(np.sqrt(F(1) - nz * nz)), 0.0, float(nz))] * 3) for i, nz in enumerate(NZ_EDGE)] + \
               [("minus_nz_2", [(0.0, float(np.sqrt(F(1) - NZ_EDGE[2] * NZ_EDGE[2])), -float(NZ_EDGE[2]))] * 3)]


@functools.lru_cache(maxsize=None)
def normals_scene():
    """16 triangles in a 4 x 4 wall, one NORMAL_SPECS entry each, over four ordinary materials."""
    m = np.zeros(4, T.MATERIAL)
    m["color"] = [[0.8, 0.7, 0.6], [0.9, 0.9, 0.9], [0.6, 0.8, 0.9], [0.7, 0.9, 0.6]]
    m["roughness"], m["metallic"] = [0.5, 0.0, 1.0, 0.3], [0.5, 1.0, 0.0, 0.0]
    m["emission"][3] = (0.2, 0.1, 0.3)
    assert len(NORMAL_SPECS) == 16
    return wall_scene(m, 4, 4, [i % 4 for i in range(16)], np.array([s[1] for s in NORMAL_SPECS], np.float32))


HUGE_EDGE = F(2.0 ** 63.5)  # edge length L of the huge triangle: L^2 = 2^127


@functools.lru_cache(maxsize=None)
def huge_triangle_scene():
    """A floor that is ONE triangle with edges of 2^63.5 along x and -z, a corner next to the camera, and a few small spheres on it.  The
    triangle test's determinant is L^2 * d.y = 2^127 * d.y: for the steeply downward camera rays (|d.y| >= 0.5) it is 2^126 or more, so
    its reciprocal — subnormal — comes from rt_rcp's full-division branch (exponent field 253 and up), and the hit distance
    t = (L^2 * 1.5) * (1 / det) of every floor pixel, and all the shading behind it, depends on that value."""
    m = np.zeros(2, T.MATERIAL)
    m["color"], m["roughness"], m["metallic"] = [[0.8, 0.7, 0.6], [0.6, 0.8, 0.9]], [0.6, 0.2], [0.0, 1.0]
    ver, nor, tri = np.zeros(3, T.VEC3), np.zeros(1, T.VEC3), np.zeros(1, T.TRIANGLE)
    ver["v"] = [(-2, -1, 2), (HUGE_EDGE, -1, 2), (-2, -1, -HUGE_EDGE)]
    nor["v"][0] = (0, 1, 0)
    tri[0] = (0, 1, 2, 0, 0, 0, 0)
    sph = np.zeros(5, T.SPHERE)  # (five of them, so that the builder makes a tree: the wide walks want three nodes or more)
    sph["pos"] = [(0.3, -0.6, -0.8), (-0.9, -0.8, -0.3), (1.2, -0.75, -0.2), (-0.5, -0.85, -1.6), (0.9, -0.9, -1.7)]
    sph["radius"], sph["material_id"] = [0.4, 0.2, 0.25, 0.15, 0.1], 1
    return R.Scene(m, sph, np.zeros(0, T.PLANE_DESC), ver, nor, tri, host.make_camera_desc((0, 0.5, 0), 0.0, -1.1, 0.8))


@functools.lru_cache(maxsize=None)
def plain(name):
    return R.Scene.load_toml(util.scene_path(name))


# ---------------------------------------------------------------------------------------------------- cameras
def camera(pos, yaw=0.0, pitch=0.0, fov_y=1.2):
    return host.camera_uniform(host.make_camera_desc(pos, yaw, pitch, fov_y))


def pole_camera(pos, up, fov_y):
    """A camera whose centre ray (rot * (0, 0, -1)) is EXACTLY (0, +1, 0) (up) or (0, -1, 0): the rotation is written down, not made from
    sin / cos of a rounded pi / 2 (whose cosine is -4.4e-8, not 0)."""
    cam = np.zeros(1, T.CAMERA)
    cam["pos"][0] = pos
    cam["rot_transform"][0][:, :3] = [(1, 0, 0), (0, 0, 1), (0, -1, 0)] if up else [(1, 0, 0), (0, 0, -1), (0, 1, 0)]  # columns
    cam["fov_y"] = fov_y
    return cam


HALF_PI = F(np.pi / 2)
# camera descriptors whose host uniforms are compared with the checker's (test_scene_edges.py); the cases below use most of them
EDGE_CAMERA_DESCS = [((0, 1, 3), 0.0, float(HALF_PI), 1.2), ((0, 1, 3), 0.0, float(-HALF_PI), 1.2), ((0, 1, 3), 0.0, 0.0, 1e-4),
                     ((0, 1, 3), 0.0, 0.0, float(F(np.pi) - F(1e-3))), ((0, 1, 1e6), 0.0, 0.0, 1e-5), ((1.0, 1.2, -1.2), 0.4, -0.2, 1.2),
                     ((0, 0, 2), 0.0, -0.4, 1.2), ((0, 1, 3), float(F(np.pi)), float(HALF_PI), 1.2), ((3e38, -3e38, 1e-42), 1e-42, -1e-42, 1e-42)]

SCALES = [-70, -63, -20, 20, 61, 64]   # 2^k: squared lengths subnormal, just normal, control, control, just finite, inf
SCALE_HIT = {("default", 20), ("default", 61), ("suzanne", 20)}  # the scaled scenes in which the checker still records hits
BOUNCES = [1, 2, 0xffff, 0x10000, 0xffffffff]
SHAPES = [(1, 1), (1, 97), (65, 5), (257, 3)]  # (w, h)
HIGH_BEGIN, HIGH_COUNT = 0xfffffff0, 15  # the last accepted sample index, 0xfffffffe, is used


@functools.lru_cache(maxsize=None)
def cases():
    """Every named edge case (the scenes are built once and shared)."""
    out = []
    env = util.small_env()

    def add(name, family, scene, cam=None, env_=None, mb=4, begin=0, count=2, w=32, h=20):
        cam = scene.camera_uniform() if cam is None else cam
        out.append(Case(name, family, scene, np.array(cam).view(T.CAMERA).reshape(1).copy(), env_ or env, mb, begin, count, w, h))

    for name in ("default", "suzanne"):
        for k in SCALES:
            sky = "" if (name, k) in SCALE_HIT else "_sky"  # (the checker records no hit: what is compared is that every ray misses)
            add("scale_%s_2^%d%s" % (name, k, sky), "scale", scaled_scene(name, k), env_=odd_env() if (name == "suzanne" and k == 20) else None)
    add("cold_rcp_huge_triangle", "cold", huge_triangle_scene(), mb=4, count=2, w=32, h=20)
    for i in range(len(ROUGHNESS)):
        add("materials_r%d" % i, "materials", material_scene(i), mb=6, w=64, h=40)
    add("normals_wall", "normals", normals_scene(), env_=odd_env(), mb=6, count=3, w=48, h=32)
    d = plain("default")
    glow = d.materials.copy()
    glow["emission"][1] = (0.5, 0.3, 0.2)  # the sphere the camera sits in: nothing else could light a closed room
    add("camera_inside_sphere", "camera", rebuilt(d, materials=glow), camera((1.0, 1.2, -1.2), 0.4, -0.2))
    add("camera_on_plane", "camera", d, camera((0, 0, 2), 0.0, -0.4))
    add("camera_pole_up_sky", "camera", d, pole_camera((0, 1, 3), True, 1.2))
    add("camera_pole_down_floor", "camera", d, pole_camera((0, 1, 3), False, 1.2))
    add("camera_fov_1e-4_pole_up", "camera", d, pole_camera((0, 1, 3), True, 1e-4))
    add("camera_fov_1e-4_pole_down", "camera", d, pole_camera((0, 1, 3), False, 1e-4))
    add("camera_fov_1e-4", "camera", d, camera((0, 1, 3), fov_y=1e-4))
    add("camera_fov_pi", "camera", d, camera((0, 1, 3), fov_y=float(F(np.pi) - F(1e-3))))
    add("camera_far_1e6", "camera", d, camera((0, 1, 1e6), fov_y=1e-5))
    add("camera_far_1e6_suzanne", "camera", plain("suzanne"), camera((0, 1, 1e6), fov_y=1e-5), env_=odd_env())
    for mb in BOUNCES:
        add("bounces_0x%x" % mb, "bounces", d, mb=mb, count=1, w=16, h=16)
    add("samples_high", "samples", d, begin=HIGH_BEGIN, count=HIGH_COUNT, w=16, h=16)
    for name in ("house", "suzanne"):
        for w, h in SHAPES:
            add("shape_%s_%dx%d" % (name, w, h), "shapes", plain(name), mb=6, w=w, h=h)
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def family(*names):
    return [c for c in cases() if c.family in names]


# ---------------------------------------------------------------------------------------------------- the checker's view of a case
@functools.lru_cache(maxsize=None)
def reference(name, fast=False):
    """The checker's image sums and counters of case `name` (computed once; callers must not write into it)."""
    c = case(name)
    img, st = oracle.render(util.oracle_scene(c.scene), util.oracle_env(c.env), c.camera.view(oracle.CAMERA), c.w, c.h, c.sample_begin,
                            c.sample_count, c.max_bounces, fast=fast)
    img.setflags(write=False)
    return img, st


@functools.lru_cache(maxsize=None)
def first_hits(name):
    """Origins, directions and the checker's closest hits of the camera rays of the case's first sample, pixel by pixel (row-major)."""
    c = case(name)
    py, px = np.mgrid[0:c.h, 0:c.w]
    o, d = D.camera_rays(c.camera[0], c.w, c.h, px.reshape(-1), py.reshape(-1), c.sample_begin)
    return o, d, oracle.cast_rays(util.oracle_scene(c.scene), o, d, 0, 0)


def centre_ray(cam):
    """rot * (0, 0, -1): the direction of a ray through the middle of the image."""
    return -np.asarray(cam["rot_transform"], np.float32).reshape(3, 4)[2, :3]


def probe_rays(c, n=12):
    """Camera-like rays for rsrt_cast_rays: the first sample's rays of an n-row image, and the exact centre ray."""
    w = max(1, n * 8 // 5)
    py, px = np.mgrid[0:n, 0:w]
    o, d = D.camera_rays(c.camera[0], w, n, px.reshape(-1), py.reshape(-1), c.sample_begin)
    o = np.concatenate([o, np.asarray(c.camera["pos"], np.float32).reshape(1, 3)])
    d = np.concatenate([d, centre_ray(c.camera[0]).reshape(1, 3)])
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def nan_policy(img):
    """(NaN pixels, finite nonzero pixels, all pixels) of image sums [H, W, 4]."""
    rgb = np.asarray(img)[..., :3]
    nan = np.isnan(rgb).any(axis=-1)
    ok = np.isfinite(rgb).all(axis=-1) & (rgb != 0).any(axis=-1)
    return int(nan.sum()), int(ok.sum()), nan.size
