"""tests/feature_rays.py without a GPU: the scenes qualify for the kernels they are meant for, every ray class reaches its edge in the
checker's own answers, and the checker agrees with an exact second reading of the three intersection routines on the rays whose
arithmetic is exact.  test_feature_rays_gpu.py then holds every probe mode to the checker on the same rays."""
import math
from fractions import Fraction as Q

import numpy as np
import pytest

import feature_rays as FR
import util
from test_scene_image import arrays, build

F = np.float32
SCENES = ("small", "large")
TIE_CLASSES = ("tri_shared_edge", "tri_diagonal", "tri_vertex")


# ---------------------------------------------------------------------------------------------------- the scenes
def test_scenes_qualify_as_intended():
    """small is the flat loop's (at most 32 records, the whole image in LDS) and every walk's; large is the cooperative walk's in
    production: no flat loop, not staged whole.  No leaf holds more than 8 records."""
    info = {name: build(arrays(FR.scene(name)))[1] for name in SCENES}
    s, g = info["small"], info["large"]
    assert s.flat_ok and s.wide_ok and s.coop_ok and s.lds_float4s > 0 and s.n_prims <= 32
    assert not g.flat_ok and g.wide_ok and g.coop_ok and g.lds_float4s == 0
    for name in SCENES + ("bare",):
        assert FR.scene(name).bvh_nodes["primitives_len"].max() <= 8, name
    print({name: (i.n_prims, i.n_nodes, FR.scene(name).bvh_depth) for name, i in info.items()})


# ---------------------------------------------------------------------------------------------------- each class reaches its edge
def _key(h):
    """What a sweep is said to change in: did_hit, material, the normal's signs, the distance."""
    return (int(h["did_hit"]), int(h["material_id"]), tuple(bool(x) for x in np.signbit(h["normal"])), float(h["distance"]))


def sweep_shares(name, kind):
    """class -> (rays, hits, sweeps, sweeps with a change, sweeps with a change between the feature and a direct neighbour)"""
    hits, (_, _, where) = FR.answers(name, kind), FR.all_rays(name)
    out = {}
    for c in FR.classes(name).values():
        r = hits[where[c.name]]
        changed = adjacent = 0
        for s in c.sweeps:
            k = [_key(h) for h in r[s.first:s.first + s.count]]
            changed += len(set(k)) > 1
            if s.centre >= 0:
                adjacent += any(k[s.centre] != k[j] for j in (s.centre - 1, s.centre + 1) if 0 <= j < s.count)
        out[c.name] = (len(r), int(r["did_hit"].sum()), len(c.sweeps), changed, adjacent)
    return out


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_each_class_reaches_its_edge(name, kind):
    """Conditions on the INPUTS, shown by the checker alone: every class has hits and misses, at least half of its sweeps change (did_hit,
    material, a sign of the normal or the distance) and at least one changes between the feature value and a direct neighbour.
    Achieved, cast_ray (kind 0) — rays / hits / sweeps / sweeps with a change / with a change next to the feature (2034 and 5011 rays):
                          small                          large
      tri_border          168 /   99 /  24 /  24 /  21    224 /  128 /  32 /  32 /  32
      tri_shared_edge      63 /   56 /   9 /   8 /   8   1001 /  924 / 143 / 132 / 132
      tri_diagonal         98 /   84 /  14 /  12 /  12    203 /  189 /  29 /  27 /  27
      tri_vertex           63 /   46 /   9 /   9 /   9   1183 / 1105 / 169 / 169 / 169
      tri_oblique         294 /  235 /  42 /  32 /  24    910 /  799 / 130 /  94 /  84
      tri_det              26 /   10 /   4 /   4 /   2     78 /   30 /  12 /  12 /   6
      tri_t                72 /   40 /  16 /  16 /   8    162 /   90 /  36 /  36 /  18
      sphere_tangent      440 /  289 /  40 /  40 /  29    440 /  294 /  40 /  40 /  29
      sphere_surface      422 /  230 /  48 /  30 /  19    the same rays, the same figures: the spheres
      plane_border        224 /  153 /  32 /  24 /  20    and planes do not move with the grid (some of
      plane_denominator    72 /   40 /  16 /  16 /   8    large's grazing tangent rays go on to its grid)
      plane_side           92 /   52 /   8 /   8 /   4
    The sweeps without a change are the lines continued past the grid (all misses), oblique rays and sphere origins whose neighbours
    round to the same answer, and borders where the ray an ulp outside still hits (below).
    cast_ray_bvh (kind 1) has fewer hits in two classes: sphere_tangent 285 (286 in large) and plane_border 137 (125).  There a routine
    accepts a ray that lies an ulp or so OUTSIDE the record's box — 0.5 * -1e-45 rounds to -0, which is not `< 0`; ps.z rounds to 1; the
    blurred tangent — so the walk never tests the record, and only cast_ray's brute-force loop over spheres and planes finds the hit."""
    shares = sweep_shares(name, kind)
    print(name, kind, shares)
    assert list(shares) == FR.CLASSES
    for cname, (rays, hits, sweeps, changed, adjacent) in shares.items():
        assert 0 < hits < rays, (cname, hits, rays)
        assert 2 * changed >= sweeps, (cname, changed, sweeps)
        assert adjacent >= 1, cname


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_ties_go_to_different_records_on_the_two_sides(name, kind):
    """On a shared edge, a diagonal and a vertex the records on the two sides of the feature differ: where both neighbours of the feature
    hit, they hit different materials (a miss on one side at the grid's border is a difference too); in large most sweeps are of that kind."""
    hits, (_, _, where) = FR.answers(name, kind), FR.all_rays(name)
    for cname in TIE_CLASSES:
        c = FR.classes(name)[cname]
        r = hits[where[cname]]
        both = 0
        for s in c.sweeps:
            lo, mid, hi = (r[s.first + s.centre + k] for k in (-1, 0, 1))
            if not mid["did_hit"]:
                assert not lo["did_hit"] and not hi["did_hit"], (cname, s)  # the lines continued past the grid
                continue
            if lo["did_hit"] and hi["did_hit"]:
                both += 1
                assert lo["material_id"] != hi["material_id"], (cname, s)
                assert mid["material_id"] in (lo["material_id"], hi["material_id"]) or cname == "tri_vertex", (cname, s)
            else:
                assert lo["did_hit"] != hi["did_hit"], (cname, s)
        assert both >= 1 and (name == "small" or 2 * both >= len(c.sweeps)), (cname, both)  # (eight of small's nine vertices lie on the border)


def f32_fma(a, b, c):
    """fma in binary32 through binary64: the product of two binary32 numbers is exact there."""
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def f32_dot(a, b):
    return f32_fma(a[2], b[2], f32_fma(a[1], b[1], F(a[0]) * F(b[0])))


@pytest.mark.parametrize("name", SCENES)
def test_a_tangent_ray_takes_the_discriminant_zero_branch(name):
    """At least one sphere_tangent ray returns what ONLY the `discriminant == 0` branch gives: its t is -0.5 * b / a in f32, and the general
    branch's formulae (q, t_0 = q / a, t_1 = c / q, the epsilon selection) give another t for the same ray.  On the axis-parallel
    tangents b and a are powers of two, the discriminant is 0 only where c is exact, and both branches give the same t; the grazing rays
    are the ones that tell (the discriminant is 0 by rounding, and c / q is below q / a by an ulp or so)."""
    c = FR.classes(name)["sphere_tangent"]
    hits = FR.answers(name, 0)[FR.all_rays(name)[2]["sphere_tangent"]]
    zero_branch = same = 0
    with np.errstate(all="ignore"):
        for i in range(len(c.o)):
            for pos, r in FR.SPHERES:
                pos, r, o, d = F(pos), F(r), c.o[i], c.d[i]
                l = o - pos
                a, b, cc = f32_dot(d, d), F(2) * f32_dot(d, l), f32_dot(l, l) - r * r
                disc = b * b - F(4) * a * cc
                if disc != 0:
                    continue
                t = F(-0.5) * b / a
                q = F(-0.5) * (b + F(0)) if b > 0 else F(-0.5) * (b - F(0))
                t0, t1 = q / a, cc / q
                general = t1 if t0 < FR.EPS_SPHERE else (t0 if t1 < FR.EPS_SPHERE else (t1 if t1 < t0 else t0))
                if hits[i]["did_hit"] and hits[i]["distance"] == t:
                    if general != t:
                        zero_branch += 1
                    else:
                        same += 1
    print(name, "discriminant == 0: the branch's own t", zero_branch, "rays; both branches agree", same)
    assert zero_branch >= 1 and same >= 1


# ---------------------------------------------------------------------------------------------------- an exact second reading
class Inexact(Exception):
    """an intermediate that binary32 does not hold: the ray is no exact ray"""


def chk(x):
    """x, if it converts to binary32 and back unchanged (a dyadic rational of at most 24 significant bits within the format's range)."""
    n, d = x.numerator, x.denominator
    if d & (d - 1):
        raise Inexact
    if n:
        n = abs(n)
        low = (n & -n).bit_length() - 1
        if (n >> low).bit_length() > 24 or low - (d.bit_length() - 1) < -149 or n.bit_length() - d.bit_length() > 127:
            raise Inexact
    return x


def q3(v):
    return tuple(Q(float(x)) for x in v)


def vsub(a, b):
    return tuple(chk(x - y) for x, y in zip(a, b))


def dot(a, b):
    p = [chk(x * y) for x, y in zip(a, b)]
    return chk(chk(p[0] + p[1]) + p[2])


def cross(a, b):
    return (chk(chk(a[1] * b[2]) - chk(a[2] * b[1])), chk(chk(a[2] * b[0]) - chk(a[0] * b[2])), chk(chk(a[0] * b[1]) - chk(a[1] * b[0])))


def along(o, d, t):
    return tuple(chk(x + chk(y * t)) for x, y in zip(o, d))


def exact_sqrt(x):
    n, d = x.numerator, x.denominator
    rn, rd = math.isqrt(n), math.isqrt(d)
    if rn * rn != n or rd * rd != d:
        raise Inexact  # (only perfect dyadic squares are kept)
    return chk(Q(rn, rd))


E_SPHERE, E_INSIDE, E_DEN, E_PLANE_T, E_DET, E_TRI_T = (Q(float(F(x))) for x in (1e-4, 1e-6, 0.0001, 0.001, 1e-8, 1e-5))


def read_sphere(o, d, pos, radius):
    """shader.wgsl cast_ray_sphere: None, or (t, whether the normal is turned)."""
    l = vsub(o, pos)
    a = dot(d, d)
    b = chk(2 * dot(d, l))
    rr = chk(radius * radius)
    c = chk(dot(l, l) - rr)
    disc = chk(chk(b * b) - chk(chk(4 * a) * c))
    if disc < 0:
        return None
    if disc == 0:
        t = chk(chk(Q(-1, 2) * b) / a)
    else:
        s = exact_sqrt(disc)
        q = chk(Q(-1, 2) * chk(b + s)) if b > 0 else chk(Q(-1, 2) * chk(b - s))
        if q == 0:
            raise Inexact  # (c / q is no number)
        t0, t1 = chk(q / a), chk(c / q)
        if t0 < E_SPHERE:
            t = t1
        elif t1 < E_SPHERE:
            t = t0
        else:
            t = min(t0, t1)
    if t < E_SPHERE:
        return None
    along(o, d, t)
    co = vsub(pos, o)
    return t, chk(dot(co, co) - rr) < E_INSIDE


def read_plane(o, d, pos, normal, columns):
    """shader.wgsl cast_ray_plane over the uploaded uniform (normal, base-change matrix): None, or (t, whether the normal is turned)."""
    den = dot(normal, d)
    if abs(den) < E_DEN:
        return None
    t = chk(dot(normal, vsub(pos, o)) / den)
    if t < E_PLANE_T:
        return None
    local = vsub(along(o, d, t), pos)
    ps = [chk(chk(chk(columns[0][k] * local[0]) + chk(columns[1][k] * local[1])) + chk(columns[2][k] * local[2])) for k in range(3)]
    if ps[0] < 0 or 1 < ps[0] or ps[2] < 0 or 1 < ps[2]:
        return None
    return t, dot(o, normal) < 0


class Reading:
    """The brute-force loop over a scene's records, in Fractions.  What depends on the triangle alone, or on the triangle and the
    direction alone, is computed once (most rays share the direction (0, 0, -1))."""

    def __init__(self, sc):
        self.spheres = [(q3(s["pos"]), Q(float(s["radius"])), int(s["material_id"])) for s in sc.spheres]
        self.planes = [(q3(p["pos"]), q3(p["normal"]), [q3(col[:3]) for col in p["base_change_matrix"]], int(p["material_id"])) for p in sc.planes]
        v = sc.vertices["v"]
        self.tris = []
        for t in sc.triangles:
            a, b, c = (q3(v[int(t[k])]) for k in ("vertex_0", "vertex_1", "vertex_2"))
            self.tris.append((a, vsub(b, a), vsub(c, a), int(t["material_id"])))
        self.by_direction = {}

    def read_triangle(self, o, d, k):
        """shader.wgsl cast_ray_triangle: None or t."""
        a, e0, e1, _ = self.tris[k]
        if (d, k) not in self.by_direction:
            try:
                p1 = cross(d, e1)
                det = dot(e0, p1)
                self.by_direction[d, k] = (p1, det, None if det == 0 else chk(1 / det))
            except Inexact:
                self.by_direction[d, k] = None
        if self.by_direction[d, k] is None:
            raise Inexact
        p1, det, inv = self.by_direction[d, k]
        if abs(det) < E_DET:
            return None  # (1 / 0 = +-inf has been computed and is not used)
        op = vsub(o, a)
        u = chk(dot(op, p1) * inv)
        if u < 0 or 1 < u:
            return None  # (the shader has computed v by now; nothing reads it)
        p0 = cross(op, e0)
        v = chk(dot(d, p0) * inv)
        if v < 0 or 1 < chk(u + v):
            return None
        t = chk(dot(e1, p0) * inv)
        if t < E_TRI_T:
            return None
        along(o, d, t)
        return t

    def cast(self, o, d):
        """(did_hit, t, materials of the records that share the smallest accepted t, the turned-normal flags of the spheres and planes
        among them); raises Inexact."""
        o, d = q3(o), q3(d)
        found = []
        for pos, r, m in self.spheres:
            h = read_sphere(o, d, pos, r)
            if h:
                found.append((h[0], m, h[1]))
        for pos, n, cols, m in self.planes:
            h = read_plane(o, d, pos, n, cols)
            if h:
                found.append((h[0], m, h[1]))
        for k in range(len(self.tris)):
            t = self.read_triangle(o, d, k)
            if t is not None:
                found.append((t, self.tris[k][3], None))
        if not found:
            return False, None, set(), set()
        t = min(f[0] for f in found)
        return True, t, {f[1] for f in found if f[0] == t}, {f[2] for f in found if f[0] == t and f[2] is not None}


def test_chk_is_the_round_trip_through_binary32():
    for x in (Q(1, 3), Q(1, 2), Q(2 ** 24 - 1), Q(2 ** 24 + 1), Q(2 ** 25 + 2), Q(1, 2 ** 149), Q(1, 2 ** 150), Q(3, 2 ** 149), Q(2 ** 127), Q(2 ** 128),
              Q(float(F(1e-5))), Q(float(F(1e-5))) / 3, Q(-5, 8), Q(0)):
        with np.errstate(over="ignore"):
            back = F(float(x)) if abs(x) < 2 ** 200 else F(np.inf)
        want = bool(np.isfinite(back)) and Q(float(back)) == x
        try:
            chk(x)
            got = True
        except Inexact:
            got = False
        assert got == want, x


LARGE_STRIDE = 5  # of the large scene's classes with more than 30 exact rays every fifth is read (a brute-force loop over 293 records in Fractions)


@pytest.mark.parametrize("name", SCENES)
def test_checker_agrees_with_an_exact_second_reading(name):
    """The three routines read a second time from the WGSL text, in fractions.Fraction, over every record of the scene, on the rays whose
    every intermediate binary32 holds (chk; a ray with one that it does not hold is dropped, and so is a sphere test whose discriminant is
    no perfect dyadic square): the sweeps' centres, the vertices, the oblique rays, the exact single rays.  For them did_hit and the
    distance equal the checker's, bit for bit, the checker's winner is one of the records that share the smallest t, and a sphere's or
    plane's turned normal is turned.
    Both queries are held to it: on these rays cast_ray_bvh finds what the brute-force loop finds.
    Rays that passed, small (all 236 candidates read): tri_border 24, tri_shared_edge 9, tri_diagonal 14, tri_vertex 9, tri_oblique 41,
    tri_det 8, tri_t 16, sphere_tangent 8, sphere_surface 38, plane_border 32, plane_denominator 16, plane_side 12: 227.  Large (every
    fifth candidate of the classes with more than thirty): 7, 29, 29, 34, 26, 6, 8, 8, 8, 7, 16, 12: 190.  What is dropped: the sweeps'
    centres at an epsilon itself (f32(1e-5) - 1 at the spheres needs more than 24 bits; their classes carry pairs of rays in small
    dyadic numbers on either side of the epsilon instead), the coplanar rays from 2^-24 above the grid for the same reason, and one
    oblique ray whose line meets a sphere at an irrational t."""
    sc = FR.scene(name)
    rd = Reading(sc)
    o, d, where = FR.all_rays(name)
    ans = {k: FR.answers(name, k) for k in (0, 1)}
    survived = {}
    for c in FR.classes(name).values():
        survived[c.name] = 0
        for i in (c.exact if name == "small" or len(c.exact) <= 30 else c.exact[::LARGE_STRIDE]):
            try:
                hit, t, ties, turned = rd.cast(c.o[i], c.d[i])
            except Inexact:
                continue
            survived[c.name] += 1
            g = where[c.name].start + i
            for kind in (0, 1):
                h = ans[kind][g]
                assert bool(h["did_hit"]) == hit, (c.name, i, kind, c.o[i], c.d[i])
                if hit:
                    assert util.bits(h["distance"]) == util.bits(F(float(t))), (c.name, i, kind, float(t), h["distance"])
                    assert int(h["material_id"]) in ties, (c.name, i, kind, ties, h["material_id"])
                    if len(ties) == 1 and turned:
                        m = int(h["material_id"])
                        outward = (h["hit_point"] - sc.spheres["pos"][m - 60]) if m < 62 else sc.planes["normal"][m - 62]
                        assert (np.dot(h["normal"].astype(np.float64), outward.astype(np.float64)) < 0) == turned.pop(), (c.name, i, kind)
    print(name, survived, sum(survived.values()))
    assert all(n >= 1 for n in survived.values()), survived
    if name == "small":
        assert sum(survived.values()) >= 200, survived


# ---------------------------------------------------------------------------------------------------- the builder on symmetric input
def _span(nodes, i):
    """[begin, end) of the records under node i (the leaves of a subtree are laid out one after another)."""
    n = nodes[i]
    if n["primitives_len"] > 0:
        return int(n["primitives_or_second_child_index"]), int(n["primitives_or_second_child_index"]) + int(n["primitives_len"])
    return _span(nodes, i + 1)[0], _span(nodes, int(n["primitives_or_second_child_index"]))[1]


def _area(lo, hi):
    d = hi - lo
    return F(2) * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2])


def split_costs(lo, hi):
    """The builder's choice for a node over items with boxes lo, hi [n, 3] float32, recomputed in f32 from its formula
    (csrc/host/bvh_build.cpp): (axis, the centroid box's extents, the eleven costs 0.125 + (n0 SA0 + n1 SA1) / SA)."""
    cen = lo * F(0.5) + hi * F(0.5)
    ext = cen.max(axis=0) - cen.min(axis=0)
    axis = 2 if (ext[2] > ext[0] and ext[2] > ext[1]) else (1 if ext[1] > ext[0] else 0)
    a, b = cen[:, axis].min(), cen[:, axis].max()
    f = F(12) * ((cen[:, axis] - a) / (b - a))
    bucket = np.minimum(np.where(f > 0, f, 0).astype(np.int64), 11)
    total = _area(lo.min(axis=0), hi.max(axis=0))
    costs = []
    for i in range(11):
        left, right = bucket <= i, bucket > i
        sa0 = _area(lo[left].min(axis=0), hi[left].max(axis=0))
        sa1 = _area(lo[right].min(axis=0), hi[right].max(axis=0))
        costs.append(F(0.125) + (F(left.sum()) * sa0 + F(right.sum()) * sa1) / total)
    return axis, ext, np.array(costs, np.float32), int((bucket <= int(np.argmin(costs))).sum())


def test_the_bare_grid_meets_exact_ties_in_the_builder():
    """lattice(16) alone: a square grid of identical quads.  Its root's centroid box is as long in x as in y (7.5 and 7.5): max_axis's
    tie rule decides, for x.  The root's eleven costs have ONE minimum (bucket 5: eight columns a side; the sixteen columns do not fall
    into the twelve buckets symmetrically) and three pairs of equal costs beside it; the exact tie of MINIMAL costs comes at the fifth
    level, at the sixteen nodes over 4 x 4 quads: their four columns fall into buckets 0, 4, 8, 11, so splits 4 .. 7 are the same split,
    four equal minimal costs, and `first minimum wins` decides.  Every interior node's split is the recomputed first minimum."""
    sc = FR.scene("bare")
    nodes, prims = sc.bvh_nodes, sc.primitives
    v = sc.vertices["v"]
    tri = sc.triangles
    corners = np.stack([v[tri["vertex_0"]], v[tri["vertex_1"]], v[tri["vertex_2"]]])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    assert (prims["primitive_type"] == 2).all()
    tied_minimum, tied_axis = [], []
    for i in range(len(nodes)):
        if nodes[i]["primitives_len"] > 0:
            continue
        b, e = _span(nodes, i)
        idx = prims["index"][b:e]
        axis, ext, costs, n_left = split_costs(lo[idx], hi[idx])
        assert axis == int(nodes[i]["split_axis"]), i
        lb, le = _span(nodes, i + 1)
        assert le - lb == n_left, (i, costs)  # the first minimum's split
        if (costs == costs.min()).sum() >= 2:
            tied_minimum.append((i, e - b))
        if ext[0] == ext[1]:
            tied_axis.append(i)
    root = split_costs(lo, hi)
    assert root[1][0] == root[1][1] == F(7.5) and 0 in tied_axis
    assert (root[2] == root[2].min()).sum() == 1 and len(set(root[2].tolist())) < 11  # one minimum, equal costs beside it
    assert len([n for n in tied_minimum if n[1] == 32]) == 16, tied_minimum  # the nodes over 4 x 4 quads (32 triangles)
