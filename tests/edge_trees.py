"""Edge inputs of the BVH builders (rsrt_build_bvh, rsrt_build_bvh_device): named sets of (spheres, plane descriptors, vertices,
triangles), each with one line saying what it is for — counts at the leaf limit and at the edges of the device builder's 256-item
chunks, chosen class strings for its closed-form partition, equal centroids (leaves of any length), flat centroid boxes and the ties
of max_axis, chains (deep lopsided trees), and ranges: a span that overflows (the empty split side), subnormal extents, a far corner.
tests/bvh_ref.py says what each must give; test_edge_trees.py holds the host builder and the checker to it, test_edge_trees_gpu.py
the device builder, and both take the trees through kernel selection and traversal."""
import collections
import functools

import numpy as np

from rsoderh_raytracing_amd import types as T

F = np.float32
Case = collections.namedtuple("Case", "name why spheres plane_descs vertices triangles")

COUNTS = [1, 2, 5, 6, 7, 255, 256, 257, 511, 512, 513, 1025]
A_X, B_X = 0.0, 100.0  # the two clusters of the `classes` family: x in [0, 1) and [100, 101)


def spheres_at(pos, radius):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    s = np.zeros(len(pos), T.SPHERE)
    s["pos"], s["radius"] = pos, radius
    return s


def planes_at(pos, forward, right):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    p = np.zeros(len(pos), T.PLANE_DESC)
    p["pos"], p["forward"], p["right"] = pos, forward, right
    return p


def soup(corners):
    """corners: [n, 3, 3] -> (vertices, triangles), three vertices of its own per triangle."""
    corners = np.asarray(corners, np.float32).reshape(-1, 3, 3)
    v = np.zeros(3 * len(corners), T.VEC3)
    v["v"] = corners.reshape(-1, 3)
    t = np.zeros(len(corners), T.TRIANGLE)
    t["vertex_0"], t["vertex_1"], t["vertex_2"] = np.arange(len(t)) * 3, np.arange(len(t)) * 3 + 1, np.arange(len(t)) * 3 + 2
    return v, t


NO_S, NO_P = np.zeros(0, T.SPHERE), np.zeros(0, T.PLANE_DESC)
NO_V, NO_T = np.zeros(0, T.VEC3), np.zeros(0, T.TRIANGLE)


def mixed(ns, npl, nt, seed):
    """Random positions in a 10-unit cube, sizes around one unit."""
    rng = np.random.default_rng(seed)
    s = spheres_at(rng.uniform(-5, 5, (ns, 3)), rng.uniform(0.05, 0.8, ns).astype(np.float32))
    p = planes_at(rng.uniform(-5, 5, (npl, 3)), rng.uniform(-1, 1, (npl, 3)), rng.uniform(-1, 1, (npl, 3)))
    v, t = soup(rng.uniform(-5, 5, (nt, 1, 3)) + rng.normal(0, 0.4, (nt, 3, 3)))
    return s, p, v, t


def two_clusters(is_left, seed):
    """One sphere per entry of is_left, in that order: a LEFT item in the cluster at x = 0, a RIGHT item in the one at x = 100; y and z
    spread over 50 units so that both children go on splitting (on y or z) and hand the permuted order down."""
    is_left = np.asarray(is_left, bool)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 50, (len(is_left), 3))
    pos[:, 0] = np.where(is_left, A_X, B_X) + rng.uniform(0, 1, len(is_left))
    return spheres_at(pos, 0.25), NO_P, NO_V, NO_T


def shuffled(n, n_left, seed):
    cls = np.arange(n) < n_left
    np.random.default_rng(seed).shuffle(cls)
    return cls


def concentric(centres, copies):
    """`copies` spheres of distinct radii around each centre: equal centroids (centres on a 1/4 grid, radii on a 1/1024 grid, so that
    (p - r) * 0.5 + (p + r) * 0.5 is p without rounding)."""
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    pos = np.repeat(centres, copies, axis=0)
    radius = np.tile(F(0.5) + np.arange(copies, dtype=np.float32) / F(1024), len(centres))
    return spheres_at(pos, radius), NO_P, NO_V, NO_T


STACK_CENTRES = [(-1.0, 0.0, 0.0), (0.0, 0.5, 0.0), (1.0, 0.0, 0.5)]


def coincident_triangles(distinct, copies, seed=41):
    """`distinct` small triangles, each `copies` times over the SAME three vertices: equal boxes and centroids, copies adjacent."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2.5, 2.5, (distinct, 1, 3)) + rng.normal(0, 0.5, (distinct, 3, 3))
    v = np.zeros(3 * distinct, T.VEC3)
    v["v"] = c.reshape(-1, 3)
    t = np.zeros(distinct * copies, T.TRIANGLE)
    base = np.repeat(np.arange(distinct) * 3, copies)
    t["vertex_0"], t["vertex_1"], t["vertex_2"] = base, base + 1, base + 2
    return NO_S, NO_P, v, t


def line(axis, n=600):
    """n items on a line along `axis` (spheres, every third a triangle): the centroid box is flat on the two other axes."""
    pos = np.zeros((n, 3))
    pos[:, axis] = np.arange(n) * 0.25
    pos += (1.0, 2.0, 3.0)
    tri = np.arange(n) % 3 == 2
    u, w = np.full(3, 0.125), np.zeros(3)
    w[axis] = 0.0625
    v, t = soup(pos[tri][:, None, :] + np.stack([-u, u, w])[None])  # (the box is pos -+ u: its centre is pos, exactly)
    return spheres_at(pos[~tri], 0.125), NO_P, v, t


def tie_box(ex, ey, ez, n=40, seed=5):
    """n spheres (radius 1/4, positions on a 1/64 grid: centres exact) whose centroid box is EXACTLY ex x ey x ez."""
    rng = np.random.default_rng(seed)
    pos = np.round(rng.uniform(0, 1, (n, 3)) * (ex, ey, ez) * 64) / 64
    pos[0], pos[1] = (0, 0, 0), (ex, ey, ez)
    return spheres_at(pos, 0.25), NO_P, NO_V, NO_T


def chain(n):
    """Spheres at x = 2^k with radius 2^k / 4: every split peels a few items off the small end."""
    x = F(2.0) ** np.arange(n, dtype=np.float32)
    pos = np.zeros((n, 3), np.float32)
    pos[:, 0] = x
    return spheres_at(pos, x * F(0.25)), NO_P, NO_V, NO_T


def overflow_spheres():
    pos = np.zeros((8, 3), np.float32)
    pos[:, 0] = np.linspace(-3e38, 3e38, 8).astype(np.float32)
    return spheres_at(pos, 1.0)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, why, arrays):
        s, p, v, t = arrays
        assert 0 < len(s) + len(p) + len(t) <= 2300
        assert (s.dtype, p.dtype, v.dtype, t.dtype) == (T.SPHERE, T.PLANE_DESC, T.VEC3, T.TRIANGLE)  # (with their padding: the builders read raw records)
        for a in (s, p, v, t):
            a.setflags(write=False)
        out.append(Case(name, why, s, p, v, t))

    for n in COUNTS:
        if n < 3:
            add("count_%d_sphere" % n, "%d item(s): the root is a leaf" % n, mixed(n, 0, 0, n))
            add("count_%d_plane" % n, "%d item(s): the root is a leaf" % n, mixed(0, n, 0, 10 + n))
            add("count_%d_triangle" % n, "%d item(s): the root is a leaf" % n, mixed(0, 0, n, 20 + n))
        else:
            ns, npl = n // 3, max(1, n // 6)
            why = {5: "the longest leaf the rule makes on its own", 6: "the shortest range that is split", 7: "one above it"}.get(
                n, "n %s the device builder's chunk of 256" % ("below, at or above a multiple of" if n < 1025 else "= 4 chunks + 1 of"))
            add("count_%d" % n, why, mixed(ns, npl, n - ns - npl, 100 + n))
    n = 513
    add("classes_sorted_%d" % n, "all LEFT first (L = 256): no holes, nothing moves", two_clusters(np.arange(n) < 256, 1))
    add("classes_reversed_%d" % n, "all RIGHT first (L = 256): every item moves", two_clusters(np.arange(n) >= n - 256, 2))
    add("classes_alternating_%d" % n, "L R L R ... (L = 257): every second place a hole", two_clusters(np.arange(n) % 2 == 0, 3))
    add("classes_left_last_%d" % n, "one LEFT item, at the very end (L = 1)", two_clusters(np.arange(n) == n - 1, 4))
    add("classes_right_first_%d" % n, "one RIGHT item, at the very start (L = n - 1)", two_clusters(np.arange(n) != 0, 5))
    for L in (255, 256, 257):
        add("classes_L%d_%d" % (L, n), "a shuffled string with L = %d: pre[L] is read at a chunk edge" % L, two_clusters(shuffled(n, L, 6 + L), 7))
    add("classes_L1_%d" % n, "a shuffled string with L = 1", two_clusters(shuffled(n, 1, 8), 9))
    add("classes_Lnm1_%d" % n, "a shuffled string with L = n - 1", two_clusters(shuffled(n, n - 1, 10), 11))
    for k in (6, 7, 9, 300):
        add("concentric_%d" % k, "%d spheres around one point: a one-node tree, a %d-record leaf" % (k, k), concentric([(0.0, 0.0, 0.0)], k))
    for k in (9, 100):
        add("stacks_%d" % k, "three points, %d concentric spheres each: leaves of %d" % (k, k), concentric(STACK_CENTRES, k))
    add("two_points_32", "two points, 32 concentric spheres each", concentric([(-1.0, 0.0, 0.0), (1.0, 0.25, 0.0)], 32))
    add("coincident_250x8", "250 triangles, 8 coincident copies each: leaves of 8, the most the per-type masks hold", coincident_triangles(250, 8))
    add("coincident_250x9", "250 triangles, 9 coincident copies each: leaves of 9, one more than they hold", coincident_triangles(250, 9))
    for a in range(3):
        add("line_%s_600" % "xyz"[a], "600 items on a line along %s: a centroid box flat on the other two axes" % "xyz"[a], line(a))
    gx, gy = np.meshgrid(np.arange(25) * 0.5, np.arange(24) * 0.5)
    add("grid_xy_600", "a 25 x 24 grid in the plane z = 1: flat on z", (spheres_at(np.stack([gx.ravel(), gy.ravel(), np.ones(600)], axis=1), 0.125), NO_P, NO_V, NO_T))
    add("tie_xy", "dx = dy > dz: x wins", tie_box(4, 4, 2))
    add("tie_xz", "dx = dz > dy: x wins", tie_box(4, 2, 4))
    add("tie_yz", "dy = dz > dx: y wins", tie_box(2, 4, 4))
    add("tie_xyz", "dx = dy = dz: x wins", tie_box(4, 4, 4))
    add("chain_40", "spheres at 2^k, k < 40: a lopsided tree", chain(40))
    add("chain_120", "spheres at 2^k, k < 120: dozens of levels of one or two nodes", chain(120))
    add("span_overflow", "x from -3e38 to 3e38: hi - lo is inf, every item in bucket 0, the empty side", (overflow_spheres(), NO_P, NO_V, NO_T))
    s, p, v, t = mixed(12, 2, 14, 77)
    add("span_overflow_beside", "the same eight beside 28 ordinary items (the span that overflows is still the root's: bvh_ref's docstring)",
        (spheres_at(np.concatenate([s["pos"], overflow_spheres()["pos"]]), np.concatenate([s["radius"], overflow_spheres()["radius"]])), p, v, t))
    pos = np.zeros((64, 3), np.float32)
    pos[:, 0] = np.arange(64, dtype=np.float32) * F(2.0) ** F(-140)
    add("subnormal_line", "x = k * 2^-140, radius 2^-142: every extent is subnormal (a build that flushed them would see one point)",
        (spheres_at(pos, F(2.0) ** F(-142)), NO_P, NO_V, NO_T))
    s, _, v, t = mixed(12, 0, 12, 78)
    add("far_corner", "a plane descriptor whose far corner is 1e30 away, beside unit-sized items",
        (s, planes_at([(0.0, -1.0, 0.0)], (1e30, 0.0, 0.0), (0.0, 0.0, 1e30)), v, t))
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def longest_leaf(nodes):
    return int(nodes["primitives_len"].max())


# ---------------------------------------------------------------------------------------------------- the trees as scenes
MATERIALS = [((0.8, 0.7, 0.6), 0.6, 0.0, (0, 0, 0)), ((0.9, 0.9, 0.9), 0.1, 1.0, (0, 0, 0)), ((0.6, 0.8, 0.9), 1.0, 0.0, (0, 0, 0)),
             ((0.7, 0.9, 0.6), 0.3, 0.5, (0.4, 0.2, 0.1)), ((0.9, 0.5, 0.4), 0.45, 0.0, (0, 0, 0))]  # colour, roughness, metallic, emission

# the scenes taken through the probe and the renders, one per outcome of kernel selection, each with a camera (pos, yaw, pitch,
# fov_y) from which the checker's first hits cover a quarter of the pixels or more (test_edge_trees.py asserts it)
CAMERAS = {
    "concentric_7": ((0.1, 0.05, 1.2), 0.0, 0.0, 1.0),
    "concentric_300": ((0.1, 0.05, 1.6), 0.0, 0.0, 1.0),
    "stacks_9": ((0.0, 0.2, 2.4), 0.0, 0.0, 1.0),
    "stacks_100": ((0.0, 0.2, 2.4), 0.0, 0.0, 1.0),
    "chain_40": ((0.0, 0.06, 0.03), -1.5707964, 0.0, 0.5),   # at the small end, looking up the chain: every sphere the same disc
    "chain_120": ((0.0, 0.06, 0.03), -1.5707964, 0.0, 0.5),
    "coincident_250x9": ((0.2, 0.1, 6.0), 0.0, 0.0, 1.0),
    "count_257": ((0.3, 0.2, 9.0), 0.0, 0.0, 1.1),
}
TRAVERSED = list(CAMERAS)


@functools.lru_cache(maxsize=None)
def scene(name):
    """Case `name` as a scene: five materials dealt out by index — coincident copies get DIFFERENT ones, so which of several equal
    hits wins shows in the picture —, geometric normals for the triangles, the host builder's tree."""
    import rsoderh_raytracing_amd as R
    from rsoderh_raytracing_amd import host
    c = case(name)
    m = np.zeros(len(MATERIALS), T.MATERIAL)
    for i, (col, rough, metal, emit) in enumerate(MATERIALS):
        m[i]["color"], m[i]["roughness"], m[i]["metallic"], m[i]["emission"] = col, rough, metal, emit
    s, p, t = c.spheres.copy(), c.plane_descs.copy(), c.triangles.copy()
    s["material_id"], p["material_id"] = np.arange(len(s)) % len(m), (np.arange(len(p)) + 1) % len(m)
    t["material_id"] = (np.arange(len(t)) + 2) % len(m)
    v = c.vertices["v"].astype(np.float64)
    nor = np.zeros(max(1, len(t)), T.VEC3)
    nor["v"][0] = (0.0, 0.0, 1.0)
    if len(t):
        g = np.cross(v[t["vertex_1"]] - v[t["vertex_0"]], v[t["vertex_2"]] - v[t["vertex_0"]])
        nor["v"] = g / np.linalg.norm(g, axis=1, keepdims=True)
        t["normal_0"] = t["normal_1"] = t["normal_2"] = np.arange(len(t))
    cam = host.make_camera_desc(*CAMERAS.get(name, ((0.0, 0.0, 10.0), 0.0, 0.0, 1.0)))
    return R.Scene(m, s, p, c.vertices.copy(), nor, t, cam)


@functools.lru_cache(maxsize=None)
def probe_rays(name, n=1024):
    """n rays for rsrt_cast_rays: half aimed at primitive centres from outside the primitive, a quarter at a corner of a primitive's
    box scaled by 1 +- 2^-10 about its centre (grazing it), a quarter starting at a primitive's centre (inside the sphere, or on the
    triangle) in a random direction.  Directions are unit vectors rounded to f32."""
    import bvh_ref
    c = case(name)
    _, _, mn, mx = bvh_ref.item_bounds(c.spheres, c.plane_descs, c.vertices, c.triangles)
    mn, mx = mn.astype(np.float64), mx.astype(np.float64)
    centre, half = (mn + mx) / 2, (mx - mn) / 2
    if len(c.triangles):  # a triangle's own centroid, not its box's centre (which may lie beside it)
        v = c.vertices["v"].astype(np.float64)
        centre[len(c.spheres) + len(c.plane_descs):] = (v[c.triangles["vertex_0"]] + v[c.triangles["vertex_1"]] + v[c.triangles["vertex_2"]]) / 3
    rng = np.random.default_rng(len(name) + n)
    near = np.nonzero(np.abs(mx).max(axis=1) < 2.0 ** 40)[0]  # (a chain's far spheres: the shader's squared lengths overflow there, and nothing is hit)
    pick = near[np.arange(n) % len(near)]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    size = np.linalg.norm(half[pick], axis=1, keepdims=True)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    a, b = n // 2, n // 2 + n // 4
    o[:a] = centre[pick[:a]] + u[:a] * (4 * size[:a])
    d[:a] = -u[:a]
    corner = np.where(rng.random((b - a, 3)) < 0.5, -1.0, 1.0) * half[pick[a:b]] * np.where(np.arange(b - a) % 2, 1 + 2.0 ** -10, 1 - 2.0 ** -10)[:, None]
    o[a:b] = centre[pick[a:b]] + u[a:b] * (4 * size[a:b])
    d[a:b] = centre[pick[a:b]] + corner - o[a:b]
    o[b:], d[b:] = centre[pick[b:]], u[b:]
    o, d = o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d
