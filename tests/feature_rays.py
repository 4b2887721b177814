"""Rays aimed at the places where the intersection routines decide (shader.wgsl:295-466, oracle/rt_oracle.cpp cast_ray_sphere / _plane /
_triangle): named scenes and named ray classes, in the manner of tests/edge_scenes.py.  Camera-like and random rays never land ON a
triangle's border, a shared edge, a tangent or an epsilon: for them `u == 0`, `u + v == 1`, `ps.x == 1`, `discriminant == 0` and
`t == eps` are events of measure zero.  Here every coordinate of the scene is a multiple of 1/2 (the spheres' radii 1 and 1/2), the rays
are axis-parallel or have small dyadic directions, so the f32 arithmetic of the three routines is exact on the feature itself and the
answer flips exactly there; each feature comes as a SWEEP: the feature value of one origin or direction component and its three f32
neighbours on either side (and, where cancellation blurs the feature, a few coarser steps).  Where the feature value is an epsilon itself
(f32(1e-5) and the like have 24 significant bits, and the spheres' tests of such a ray round), the class carries a pair of rays in small
dyadic numbers on either side of the epsilon as well, which stay exact against every record: the scales of d are free, the probe
normalises nothing.

Scenes (built by the host builder, nothing foreign):
  small = lattice(2), large = lattice(12): an nq x nq grid of half-unit quads in z = 0 over [0, nq / 2]^2, two triangles a quad with
      the quad's vertices repeated per quad; two spheres and three parallelograms beside it (SPHERES, PLANES below).  Triangle k has
      material k mod 60 and the three NORMALS rotated by k; spheres and planes have materials 60 .. 64: the record that won shows in
      material_id and in the normal.
  bare = lattice(16, extras=False): the grid alone, for the BVH builders (equal SAH costs and equal centroid extents).
Quad (i, j) holds triangle A = (p00, p10, p11), u = 2 (x - y), v = 2 y in the quad's coordinates for a ray along -z, and triangle
B = (p00, p11, p01), u = 2 x, v = 2 (y - x): A is the half x >= y, B the half y >= x, and the diagonal belongs to both.

test_feature_rays.py shows without a GPU that every class reaches its edge and holds the checker to an exact second reading on the
sweeps' centres; test_feature_rays_gpu.py holds every probe mode to the checker on all of them."""
import collections
import functools

import numpy as np

import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host, types as T

F = np.float32
HEIGHT = 2.0                      # the axis-parallel rays start two units above what they aim at
DOWN = (0.0, 0.0, -1.0)
NORMALS = [(0.0, 0.0, 1.0), (0.0, 0.6, 0.8), (0.6, 0.0, 0.8)]
# (centre, radius): beside the grid, on the side of negative x
SPHERES = [((-2.0, 1.0, 1.0), 1.0), ((-3.5, -0.5, 0.5), 0.5)]
# (pos, forward, right): an axis-aligned and a sheared parallelogram in z = 0, a third one in z = -1 (the normal flip by the origin)
PLANES = [((0.0, -2.5, 0.0), (0.0, 2.0, 0.0), (2.0, 0.0, 0.0)), ((3.0, -2.5, 0.0), (1.0, 2.0, 0.0), (2.0, 0.0, 0.0)),
          ((-1.0, -5.0, -1.0), (0.0, 2.0, 0.0), (2.0, 0.0, 0.0))]
EPS_SPHERE, EPS_INSIDE, EPS_DENOMINATOR, EPS_PLANE_T, EPS_DET, EPS_TRI_T = F(1e-4), F(1e-6), F(1e-4), F(1e-3), F(1e-8), F(1e-5)
SIZES = {"small": 2, "large": 12}
CLASSES = ["tri_border", "tri_shared_edge", "tri_diagonal", "tri_vertex", "tri_oblique", "tri_det", "tri_t", "sphere_tangent", "sphere_surface",
           "plane_border", "plane_denominator", "plane_side"]

# first ray, number of rays, position of the feature value among them (-1: the sweep has none)
Sweep = collections.namedtuple("Sweep", "first count centre")
# o, d: [n, 3] float32; sweeps: the class's sweeps; exact: the rays that are candidates for the exact second reading (the sweeps' centres,
# and single rays with small dyadic components that belong to no sweep)
RayClass = collections.namedtuple("RayClass", "name o d sweeps exact")


# ---------------------------------------------------------------------------------------------------- scenes
def materials():
    k = np.arange(65)
    m = np.zeros(65, T.MATERIAL)
    m["color"] = np.stack([0.3 + 0.6 * ((k * 7) % 11) / 10, 0.3 + 0.6 * ((k * 5) % 13) / 12, 0.3 + 0.6 * ((k * 3) % 7) / 6], axis=1)
    m["roughness"], m["metallic"] = 0.2 + 0.7 * ((k * 4) % 9) / 8, np.where(k % 4 == 0, 0.8, 0.0)
    m["emission"][k % 16 == 5] = (0.2, 0.1, 0.05)
    return m


def lattice(nq, extras=True):
    """The grid of nq x nq quads (and, with extras, SPHERES and PLANES) under the host builder's tree."""
    ver, tri = np.zeros(4 * nq * nq, T.VEC3), np.zeros(2 * nq * nq, T.TRIANGLE)
    for j in range(nq):
        for i in range(nq):
            q = j * nq + i
            x, y = 0.5 * i, 0.5 * j
            ver["v"][4 * q:4 * q + 4] = [(x, y, 0), (x + 0.5, y, 0), (x + 0.5, y + 0.5, 0), (x, y + 0.5, 0)]
            for half, (b, c) in enumerate(((1, 2), (2, 3))):
                k = 2 * q + half
                tri[k] = (4 * q, 4 * q + b, 4 * q + c, k % 3, (k + 1) % 3, (k + 2) % 3, k % 60)
    nor = np.zeros(3, T.VEC3)
    nor["v"] = NORMALS
    sph, pls = np.zeros(len(SPHERES) if extras else 0, T.SPHERE), np.zeros(len(PLANES) if extras else 0, T.PLANE_DESC)
    if extras:
        sph["pos"], sph["radius"], sph["material_id"] = [s[0] for s in SPHERES], [s[1] for s in SPHERES], [60, 61]
        pls["pos"], pls["forward"], pls["right"] = [p[0] for p in PLANES], [p[1] for p in PLANES], [p[2] for p in PLANES]
        pls["material_id"] = [62, 63, 64]
    cam = host.make_camera_desc((0.25 * nq, 0.25 * nq - 0.5, 2.0 + 0.3 * nq), 0.05, -0.03, 1.2)  # above the grid, looking down -z
    return R.Scene(materials(), sph, pls, ver, nor, tri, cam)


@functools.lru_cache(maxsize=None)
def scene(name):
    return lattice(16, extras=False) if name == "bare" else lattice(SIZES[name])


# ---------------------------------------------------------------------------------------------------- sweeps
def around(v, coarse=False):
    """(values, index of v): f32(v) and its three f32 neighbours on either side, ascending; coarse: v -+ 2^-12 and 2^-8 as well."""
    v = F(v)
    lo, hi = [v], [v]
    for _ in range(3):
        lo.append(np.nextafter(lo[-1], F(-np.inf)))
        hi.append(np.nextafter(hi[-1], F(np.inf)))
    vals = lo[:0:-1] + [v] + hi[1:]
    if coarse:
        vals = [v - F(2.0 ** -8), v - F(2.0 ** -12)] + vals + [v + F(2.0 ** -12), v + F(2.0 ** -8)]
    assert all(a < b for a, b in zip(vals, vals[1:]))
    return vals, vals.index(v)


def around_zero():
    """... around +0.0 with -0.0 in it, and the coarse steps (the nearest neighbours of zero are subnormal)."""
    vals, c = around(0.0, coarse=True)
    return vals[:c] + [F(-0.0)] + vals[c:], c + 1


class _Builder:
    def __init__(self):
        self.o, self.d, self.sweeps, self.exact = [], [], [], []

    def ray(self, o, d, exact=False):
        self.o.append([F(x) for x in o])
        self.d.append([F(x) for x in d])
        if exact:
            self.exact.append(len(self.o) - 1)
        return len(self.o) - 1

    def sweep(self, o, d, part, axis, values, exact=True):
        """The ray (o, d) with component `axis` of its origin (part "o") or direction ("d") taking `values` = (list, feature's index);
        exact: the feature's ray is a candidate for the exact second reading."""
        vals, c = values
        first = len(self.o)
        for i, v in enumerate(vals):
            oo, dd = list(o), list(d)
            (oo if part == "o" else dd)[axis] = v
            self.ray(oo, dd, exact=exact and i == c)
        self.sweeps.append(Sweep(first, len(vals), c))

    def done(self, name):
        return RayClass(name, np.array(self.o, np.float32).reshape(-1, 3), np.array(self.d, np.float32).reshape(-1, 3), list(self.sweeps),
                        list(self.exact))


def _some(n):
    """All of 0 .. n - 1 for the small grid, the first, the middle and the last for the large one."""
    return list(range(n)) if n <= 3 else sorted({0, n // 2, n - 1})


def tri_border(nq):
    """The grid's outer lines: hit <-> miss at u == 0 (B at x = 0), v == 0 (A at y = 0), u + v == 1 (A at x = E, B at y = E), and the grid's
    four corners (u == 1 with v == 0 among them)."""
    b, e = _Builder(), 0.5 * nq
    for j in _some(nq):
        for f in (0.125, 0.375):
            s = 0.5 * j + f
            b.sweep((0, s, HEIGHT), DOWN, "o", 0, around(0.0))
            b.sweep((e, s, HEIGHT), DOWN, "o", 0, around(e))
            b.sweep((s, 0, HEIGHT), DOWN, "o", 1, around(0.0))
            b.sweep((s, e, HEIGHT), DOWN, "o", 1, around(e))
    for x in (0.0, e):
        for y in (0.0, e):
            b.sweep((x, y, HEIGHT), DOWN, "o", 0, around(x))
            b.sweep((x, y, HEIGHT), DOWN, "o", 1, around(y))
    return b.done("tri_border")


def tri_shared_edge(nq):
    """The inner lattice lines: record <-> record, both at the same t on the line itself; and each line continued past the grid's border
    (a miss on either side and on the line)."""
    b = _Builder()
    for i in range(1, nq):
        b.sweep((0.5 * i, -0.125, HEIGHT), DOWN, "o", 0, around(0.5 * i))
        for j in _some(nq):
            for f in (0.125, 0.375):
                b.sweep((0.5 * i, 0.5 * j + f, HEIGHT), DOWN, "o", 0, around(0.5 * i))
                b.sweep((0.5 * j + f, 0.5 * i, HEIGHT), DOWN, "o", 1, around(0.5 * i))
    return b.done("tri_shared_edge")


def tri_diagonal(nq):
    """Points with equal fractional parts: A's u == 0 and B's v == 0, between the two triangles of a quad; and the grid's main diagonal
    continued past both of its ends (misses)."""
    b = _Builder()
    for s in (-0.125, 0.5 * nq + 0.125):
        b.sweep((s, s, HEIGHT), DOWN, "o", 0, around(s))
    for i in _some(nq):
        for j in _some(nq):
            for f in (0.125, 0.25, 0.375):
                b.sweep((0.5 * i + f, 0.5 * j + f, HEIGHT), DOWN, "o", 0, around(0.5 * i + f))
    return b.done("tri_diagonal")


def tri_vertex(nq):
    """Every lattice vertex (up to six records meet there), approached along x or along y."""
    b = _Builder()
    for j in range(nq + 1):
        for i in range(nq + 1):
            axis = (i + j) % 2
            b.sweep((0.5 * i, 0.5 * j, HEIGHT), DOWN, "o", axis, around(0.5 * (i, j)[axis]))
    return b.done("tri_vertex")


OBLIQUE = [(1.0, 0.0, -1.0), (0.0, 1.0, -2.0), (-1.0, -1.0, -4.0), (1.0, -1.0, -2.0)]  # (d.z a power of two: 1 / determinant is exact)


def tri_oblique(nq):
    """Small dyadic directions with three different finite 1 / d components, from origins one d before a lattice vertex or the middle of a
    lattice edge: the arithmetic stays exact, the box test has no infinities to lean on."""
    b = _Builder()
    some = sorted(set(range(nq + 1)) if nq <= 3 else {0, 1, nq // 2, nq - 1, nq})
    targets = [(0.5 * i, 0.5 * j) for j in some for i in some]
    targets += [(0.5 * i + 0.25, 0.5 * j) for j in some for i in some if i < nq] + [(0.5 * i, 0.5 * j + 0.25) for j in some for i in some if j < nq]
    for k, (x, y) in enumerate(targets):
        for d in (OBLIQUE[k % 4], OBLIQUE[(k + 1) % 4]):
            b.sweep((x - d[0], y - d[1], -d[2]), d, "o", 0, around(x - d[0]))
    return b.done("tri_oblique")


DET_DZ = F(4.0) * EPS_DET  # d = (1, 0, -dz) over triangle A: determinant = 0.25 dz, exactly


def tri_det(nq):
    """Rays nearly in the triangles' plane, d = (1, 0, -dz) from 2^-24 above it: |determinant| = 0.25 dz crosses 1e-8 at dz = 4 f32(1e-8).
    They reach z = 0 after about 1.5 units of x, inside triangle A of the quad they are aimed at.  With them the coplanar dz = 0 and -0
    (1 / determinant = +-inf), from above and in the plane, and a pair of rays in small dyadic numbers, which stay exact against every
    record of the scene: d = (s, 0, -s) from one unit above, s = 2^-25 (determinant 2^-27: a miss, the determinant is not normalised)
    and 2^-24 (2^-26: a hit at t = 2^24)."""
    b, h = _Builder(), 2.0 ** -24
    for i in (sorted({2, nq - 1}) if nq > 2 else [1]):
        for j in _some(nq):
            x, y = 0.5 * i + 0.25, 0.5 * j + 0.0625
            o = (x - 1.5, y, h)
            b.sweep(o, (1.0, 0.0, 0.0), "d", 2, ([-v for v in around(DET_DZ)[0]][::-1], 3), exact=False)
            first = len(b.o)
            for s in (2.0 ** -25, 2.0 ** -24):
                b.ray((x - 1.0, y, 1.0), (s, 0.0, -s), exact=True)
            b.sweeps.append(Sweep(first, 2, -1))
            for dz in (0.0, -0.0):
                b.ray(o, (1.0, 0.0, dz), exact=True)
                b.ray((o[0], o[1], 0.0), (1.0, 0.0, dz), exact=True)
    return b.done("tri_det")


def tri_t(nq):
    """Origins at heights around 1e-5 above the grid: t is the height, exactly.  With them a pair of rays in small dyadic numbers, which
    stay exact against every record of the scene: from 2^-4 above with d = (0, 0, -2^13) (t = 2^-17: a miss) and (0, 0, -2^12) (2^-16: a hit)."""
    b = _Builder()
    for i in _some(nq):
        for j in _some(nq):
            for fx, fy in ((0.375, 0.125), (0.125, 0.375)):  # in A, in B
                b.sweep((0.5 * i + fx, 0.5 * j + fy, EPS_TRI_T), DOWN, "o", 2, around(EPS_TRI_T), exact=False)
                first = len(b.o)
                for dz in (-2.0 ** 13, -2.0 ** 12):
                    b.ray((0.5 * i + fx, 0.5 * j + fy, 2.0 ** -4), (0.0, 0.0, dz), exact=True)
                b.sweeps.append(Sweep(first, 2, -1))
    return b.done("tri_t")


GRAZING = [(1.0, 0.0, -2.0), (-1.0, 0.0, -1.0), (1.0, 0.0, -3.0), (-3.0, 0.0, -4.0), (2.0, 0.0, -3.0), (-1.0, 0.0, -3.0), (3.0, 0.0, -2.0), (-2.0, 0.0, -1.0)]


def sphere_tangent(nq):
    """Both spheres, from two units above the centre's height: x (or y) around centre +- radius along -z, where the discriminant is an exact
    0 on the feature and for a few neighbours (f32 cancellation), with coarser steps on either side; and grazing rays with a direction
    component ALONG the swept axis, eleven consecutive f32 values of x around the tangent: there b itself has many bits, the discriminant
    is 0 by rounding only, and the `== 0` branch's t differs from what the general branch would give."""
    b = _Builder()
    for (c, r) in SPHERES:
        for axis in (0, 1):
            for side in (-1.0, 1.0):
                o = [c[0], c[1], c[2] + HEIGHT]
                o[axis] = c[axis] + side * r
                b.sweep(o, DOWN, "o", axis, around(o[axis], coarse=True))
        for d in GRAZING:
            # the tangent in the plane y = centre's: origins (x, cy, cz + 2) with |l x d| = r |d|, l = origin - centre
            n = np.hypot(d[0], d[2])
            for side in (-1.0, 1.0):
                x = c[0] + (side * r * n - HEIGHT * d[0]) / -d[2]
                vals = [F(x)]
                for _ in range(5):
                    vals = [np.nextafter(vals[0], F(-np.inf))] + vals + [np.nextafter(vals[-1], F(np.inf))]
                b.sweep((x, c[1], c[2] + HEIGHT), d, "o", 0, (vals, 5), exact=False)
    return b.done("sphere_tangent")


def sphere_surface(nq):
    """Origins exactly on the surface, entering and leaving, and at the centre; origins at distance r + 1e-4 (t_0 < EPSILON selects t_1 on
    one side only) and at distance r, with r + {2, 4, 6, 8, 12, 16}e-7 (the `< 1e-6` inside test turns the normal)."""
    b = _Builder()
    for (c, r) in SPHERES:
        for axis in (0, 2):
            for side in (-1.0, 1.0):
                o, d = list(c), [0.0, 0.0, 0.0]
                o[axis] = c[axis] + side * r
                for way in (-1.0, 1.0):  # entering, leaving
                    d[axis] = way * side
                    b.ray(o, d, exact=True)
                    b.sweep(o, d, "o", axis, around(o[axis]))
                    far = [c[axis] + side * (F(r) + F(k * 1e-7)) for k in (2, 4, 6, 8, 12, 16)]
                    b.sweep(o, d, "o", axis, (sorted(around(o[axis])[0][3:4] + far), 0 if side > 0 else len(far)), exact=False)
                    b.sweep(o, d, "o", axis, around(c[axis] + side * (F(r) + EPS_SPHERE), coarse=True), exact=False)
        for d in (DOWN, (1.0, 0.0, 0.0), (0.0, -2.0, 0.0)):
            b.ray(c, d, exact=True)
    return b.done("sphere_surface")


def plane_border(nq):
    """ps.x and ps.z at 0 and 1 on the axis-aligned and on the sheared parallelogram, and all eight corners."""
    b = _Builder()
    for (pos, fw, rt) in PLANES[:2]:
        for u in (0.25, 0.75):  # along forward: the lines ps.x == 0 and ps.x == 1, x swept
            y = pos[1] + u * fw[1]
            for s in (0.0, 1.0):
                x = pos[0] + s * rt[0] + u * fw[0]
                b.sweep((x, y, HEIGHT), DOWN, "o", 0, around(x))
        for s in (0.25, 0.75):  # along right: the lines ps.z == 0 and ps.z == 1, y swept
            for u in (0.0, 1.0):
                x, y = pos[0] + s * rt[0] + u * fw[0], pos[1] + u * fw[1]
                b.sweep((x, y, HEIGHT), DOWN, "o", 1, around(y))
        for s in (0.0, 1.0):
            for u in (0.0, 1.0):
                x, y = pos[0] + s * rt[0] + u * fw[0], pos[1] + u * fw[1]
                b.sweep((x, y, HEIGHT), DOWN, "o", 0, around(x))
                b.sweep((x, y, HEIGHT), DOWN, "o", 1, around(y))
    return b.done("plane_border")


def plane_denominator(nq):
    """d = (1, 0, -dz) from 2^-13 above the planes in z = 0, aimed at their interiors: |n . d| = dz crosses 1e-4; rays along -z from heights
    around 0.001: t is the height, exactly.  With them two pairs of rays in small dyadic numbers, which stay exact against every record of
    the scene: d = (s, 0, -s) from one unit above, s = 2^-14 (a miss: the denominator is not normalised) and 2^-13 (a hit at t = 2^13), and
    rays from 2^-4 above with d = (0, 0, -2^6) (t = 2^-10: a miss) and (0, 0, -2^5) (2^-9: a hit)."""
    b, h = _Builder(), 2.0 ** -13
    for x, y in ((1.0, -1.5), (0.5, -2.0), (4.5, -1.5), (4.25, -2.0)):
        b.sweep((x - 1.25, y, h), (1.0, 0.0, 0.0), "d", 2, ([-v for v in around(EPS_DENOMINATOR)[0]][::-1], 3), exact=False)
        b.sweep((x, y, EPS_PLANE_T), DOWN, "o", 2, around(EPS_PLANE_T))
        first = len(b.o)
        for s in (2.0 ** -14, 2.0 ** -13):
            b.ray((x - 1.0, y, 1.0), (s, 0.0, -s), exact=True)
        b.sweeps.append(Sweep(first, 2, -1))
        first = len(b.o)
        for dz in (-2.0 ** 6, -2.0 ** 5):
            b.ray((x, y, 2.0 ** -4), (0.0, 0.0, dz), exact=True)
        b.sweeps.append(Sweep(first, 2, -1))
    return b.done("plane_denominator")


def plane_side(nq):
    """Onto the parallelogram in z = -1 from origins whose z is swept around 0, -0.0 included: dot(origin, n) changes sign, and the shader
    turns the normal by the ORIGIN, not by the origin relative to the plane.  With them origins around the plane's own height (t around 0:
    a hit from 2^-8 above it only) where that sign stays."""
    b = _Builder()
    pos = PLANES[2][0]
    for x, y in ((0.5, 0.5), (1.0, 1.5), (1.5, 0.25), (0.25, 1.75)):
        vals, c = around_zero()
        b.sweep((pos[0] + x, pos[1] + y, 0.0), DOWN, "o", 2, (vals, c))
        b.exact.append(b.sweeps[-1].first + c - 1)  # (-0.0 too)
        b.sweep((pos[0] + x, pos[1] + y, pos[2]), DOWN, "o", 2, around(pos[2], coarse=True))
    return b.done("plane_side")


@functools.lru_cache(maxsize=None)
def classes(name):
    """name -> RayClass, for scene `name` ("small" or "large"), in CLASSES' order."""
    out = collections.OrderedDict((c, globals()[c](SIZES[name])) for c in CLASSES)
    for c in out.values():
        c.o.setflags(write=False)
        c.d.setflags(write=False)
        assert np.isfinite(c.o).all() and np.isfinite(c.d).all() and (c.d != 0).any(axis=1).all()
    return out


@functools.lru_cache(maxsize=None)
def all_rays(name):
    """(origins, directions, {class: slice}) of the classes of `name`, one after another."""
    cl = classes(name)
    at, where = 0, {}
    for c in cl.values():
        where[c.name] = slice(at, at + len(c.o))
        at += len(c.o)
    o, d = np.concatenate([c.o for c in cl.values()]), np.concatenate([c.d for c in cl.values()])
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d, where


@functools.lru_cache(maxsize=None)
def answers(name, kind):
    """The checker's records of all_rays(name) (kind 0: cast_ray, 1: cast_ray_bvh), computed once; callers must not write into them."""
    o, d, _ = all_rays(name)
    out = oracle.cast_rays(util.oracle_scene(scene(name)), o, d, kind, 0)
    out.setflags(write=False)
    return out
