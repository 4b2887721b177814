"""The edge cases of tests/edge_scenes.py without a GPU: every case shows from the checker's output that it reaches the edge it is named
for; the strict and the -O3 build of the checker agree on every case (the full-frame GPU test trusts the latter); the NaN policy holds
(at most a quarter of a case's pixels NaN, at least one finite and nonzero); and the host library's preprocessing — scene loader rows,
plane and camera uniforms, the BVH builder — agrees with the checker's on the edge inputs."""
import numpy as np
import pytest

import edge_scenes as E
import oracle
import util
from oracle import scene_py
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host, types as T

F = np.float32
TINY = F(2.0) ** -126  # the smallest normal f32
NAMES = [c.name for c in E.cases()]


def hits_of(name):
    o, d, hit = E.first_hits(name)
    return o, d, hit, hit["did_hit"] != 0


# ---------------------------------------------------------------------------------------------------- each case reaches its edge
def reach_scale(c):
    """The same camera rays (scaling keeps directions) hit the unscaled scene at t0; the scaled scene's first-hit distances are
    t0 * 2^k, and their f32 squares are what the case is named for.  What the checker then records is asserted as well: nothing below
    the shader's epsilons and nothing once dot(l, l) overflows; hits with squares near the format's end at 2^61."""
    name, k = c.name.split("_")[1], int(c.name.split("^")[1].split("_")[0])
    base = E.scaled_scene(name, 0)
    py, px = np.mgrid[0:c.h, 0:c.w]
    o, d = E.D.camera_rays(base.camera_uniform()[0], c.w, c.h, px.reshape(-1), py.reshape(-1), 0)
    _, d_scaled, hit, m = hits_of(c.name)
    assert np.array_equal(util.bits(d), util.bits(d_scaled))
    t0 = oracle.cast_rays(util.oracle_scene(base), o, d, 0, 0)
    t0 = t0["distance"][t0["did_hit"] != 0]
    assert len(t0) > 100
    with np.errstate(over="ignore", under="ignore"):
        t = t0 * F(2.0) ** F(k)
        q = t * t
    if k == -70:
        assert (q < TINY).all() and (q > 0).any() and not m.any()  # subnormal squares (the smallest underflow to 0)
    elif k == -63:
        assert (q >= TINY).all() and (q < TINY * F(2.0) ** 12).all() and not m.any()
    elif k == -20:
        assert (t < F(1e-4)).all() and (q > TINY).all() and not m.any()  # the control: ordinary numbers, all under the shader's epsilons
    elif k == 20:
        assert m.sum() > 100 and np.isfinite(q).all() and (hit["distance"][m] > F(2.0) ** 20).all()  # the control: ordinary hits
    elif k == 61:
        assert (q > F(2.0) ** 120).all() and np.isfinite(q).mean() > 0.9  # the last octaves (suzanne's farthest hits are past them)
        if name == "default":  # its spheres are still hit; their squared distances sit in the format's last octaves
            dist = hit["distance"][m]
            assert len(dist) > 0 and (dist * dist > F(2.0) ** 120).all() and np.isfinite(dist * dist).all()
    else:
        assert k == 64 and np.isinf(q).all() and not m.any()


def reach_cold(c):
    """More than a hundred first hits lie on the huge triangle with a determinant of 2^126 or more (recomputed here in f32 as the
    shader does): an exponent field of 253 or 254, whose reciprocal is subnormal — and their distances are ordinary numbers."""
    _, d, hit, m = hits_of(c.name)
    v = c.scene.vertices["v"]
    e0, e1 = v[1] - v[0], v[2] - v[0]
    with np.errstate(over="ignore"):
        det = (np.cross(d, e1).astype(np.float32) * e0).sum(axis=1, dtype=np.float32)
    floor = m & (hit["material_id"] == 0)
    cold = floor & (np.abs(det) >= F(2.0) ** 126) & np.isfinite(det)
    assert cold.sum() > 100 and (F(1) / np.abs(det[cold]) < TINY).all()
    assert ((hit["distance"][cold] > 1.4) & (hit["distance"][cold] < 4)).all()
    assert (m & (hit["material_id"] == 1)).any() and E.reference(c.name)[1]["shadow_rays"] > 100


def reach_materials(c):
    """Every material of the page is the closest hit of some first-sample camera ray; the sums hold inf (emission 3e38) and nonzero
    values below 2^-126 (emission 1e-42, colour 1e-5); and the page's roughness is where its name puts it against the clamp."""
    _, _, hit, m = hits_of(c.name)
    assert set(hit["material_id"][m].tolist()) == set(range(64))
    rgb = E.reference(c.name)[0][..., :3]
    assert np.isinf(rgb).any() and ((rgb != 0) & (np.abs(rgb) < TINY)).any() and (rgb < 0).any()
    i = int(c.name[-1])
    r = c.scene.materials["roughness"][0]
    assert r == E.ROUGHNESS[i]
    sq, clamp = r * r, F(0.001)
    assert [sq == 0, sq < clamp, sq < clamp, sq > clamp, sq == 1, sq > 1, (r < 0) and sq == F(0.25)][i]
    if i == 2:  # no f32 squares to f32(0.001) exactly (neighbouring squares are two ulps apart there): sqrt(0.001) lands one ulp under the
        assert sq == np.nextafter(clamp, F(0))  # clamp — the last alpha it replaces
    if i == 3:  # ... and its upper neighbour one ulp over it: the first alpha that it lets through unchanged
        assert sq == np.nextafter(clamp, F(1))
    me = c.scene.materials["metallic"]
    assert me.min() < 0 and me.max() > 1


def reach_normals(c):
    """Closest hits whose shading normal is exactly +z, just under and just over make_frame's |n.z| = 0.999, NaN (zero-length and
    cancelling vertex normals), and unit although the vertex normals are 1e-3 or 1e3 long."""
    _, d, hit, m = hits_of(c.name)
    n = hit["normal"][m]
    nz = np.abs(n[:, 2])
    assert (nz == 1).any()
    assert ((nz < F(0.999)) & (nz > F(0.9989))).any() and ((nz >= F(0.999)) & (nz < F(0.9991))).any()
    assert (nz == F(0.999)).any()
    assert np.isnan(n).any()
    # every triangle of the wall is seen: 16 distinct cells among the hit points
    p = hit["hit_point"][m]
    cells = set(zip((p[:, 0] // 2).astype(int).tolist(), (p[:, 1] // 1.25).astype(int).tolist()))
    assert len(cells) == 16
    # opposed normals are turned towards the ray: no finite hit normal points along the ray
    fin = np.isfinite(n).all(axis=1)
    assert ((n[fin] * d[m][fin]).sum(axis=1) <= 0).all()
    assert np.isnan(E.reference(c.name)[0]).any()


def reach_camera(c):
    o, d, hit, m = hits_of(c.name)
    img, st = E.reference(c.name)
    centre = E.centre_ray(c.camera[0])
    if c.name == "camera_inside_sphere":
        s = c.scene.spheres[1]
        assert np.linalg.norm(o[0] - s["pos"]) < s["radius"] and m.all() and st["escapes"] == 0
        assert (hit["material_id"][m] == s["material_id"]).sum() > 100  # seen from inside (the rest: what sticks into it)
    elif c.name == "camera_on_plane":
        assert o[0, 1] == 0 and c.scene.plane_descs["pos"][0, 1] == 0 and (d[:, 1] < 0).sum() > 100
        assert not (hit["material_id"][m] == c.scene.plane_descs["material_id"][0]).any()  # t = 0 < 0.001: the plane is never hit
    elif "pole" in c.name:
        up = "up" in c.name
        assert np.array_equal(centre, F([0, 1 if up else -1, 0]))
        if "fov" in c.name:  # so narrow that the y component of EVERY camera ray rounds to +-1: asin(+-1), the map's first / last row
            assert (np.abs(d[:, 1]) == 1).all() and (d[:, 0] != 0).any()
        assert m.all() != up and m.any() != up  # up: open sky; down: the floor
        probe = oracle.cast_rays(util.oracle_scene(c.scene), c.camera["pos"], centre.reshape(1, 3), 0, 0)
        assert bool(probe["did_hit"][0]) != up
    elif c.name == "camera_fov_1e-4":
        assert c.camera["fov_y"][0] == F(1e-4) and (d[:, 2] == -1).all()
    elif c.name == "camera_fov_pi":
        fov = c.camera["fov_y"][0]  # the image plane's half height is sin(fov_y / 2): within an ulp of its largest value, 1
        assert fov == F(np.pi) - F(1e-3) and 1 - 2e-7 < oracle.detmath("sin", float(fov / F(2))) <= 1
    else:
        assert c.name.startswith("camera_far_1e6") and m.any() and (hit["distance"][m] > 9.9e5).all()


def reach_bounces(c):
    """An open scene: paths end by escape (or by the throughput cut), so the three large limits trace the very same rays, more than the
    small ones do, and far fewer than the limit allows."""
    img, st = E.reference(c.name)
    assert st["escapes"] > 0.4 * st["paths"] and st["ext_rays"] <= st["paths"] * min(c.max_bounces, 50)
    big = [E.reference("bounces_0x%x" % mb)[1] for mb in (0xffff, 0x10000, 0xffffffff)]
    assert big[0] == big[1] == big[2] and big[0]["escapes"] > 0.9 * big[0]["paths"]
    assert E.reference("bounces_0x1")[1]["ext_rays"] < E.reference("bounces_0x2")[1]["ext_rays"] < big[0]["ext_rays"]
    if c.max_bounces >= 0xffff:
        assert util.same_bits_or_nan(img, E.reference("bounces_0xffff")[0])


def reach_samples(c):
    assert c.sample_begin + c.sample_count - 1 == 0xfffffffe
    img = E.reference(c.name)[0]
    low = oracle.render(util.oracle_scene(c.scene), util.oracle_env(c.env), c.camera.view(oracle.CAMERA), c.w, c.h, 0, c.sample_count,
                        c.max_bounces)[0]
    assert not np.array_equal(util.bits(img), util.bits(low))  # the seed does mix the index's high bits
    assert oracle.rng_seed(7, 0xfffffffe) != oracle.rng_seed(7, 0x7ffffffe) != oracle.rng_seed(7, 0xfffe)


def reach_shapes(c):
    img = E.reference(c.name)[0]
    assert img.shape == (c.h, c.w, 4) and (c.w, c.h) in E.SHAPES and (img[..., 3] == 1).all()


REACH = {"cold": reach_cold, "scale": reach_scale, "materials": reach_materials, "normals": reach_normals, "camera": reach_camera, "bounces": reach_bounces,
         "samples": reach_samples, "shapes": reach_shapes}


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge_and_both_checker_builds_agree(name):
    c = E.case(name)
    REACH[c.family](c)
    img, st = E.reference(name)
    fast, fst = E.reference(name, True)
    assert util.same_bits_or_nan(img, fast) and st == fst
    nan, ok, n = E.nan_policy(img)
    assert 4 * nan <= n and ok >= 1, (nan, ok, n)
    assert bool(nan or np.isinf(img).any()) == (name in E.NAN_OR_INF_CASES)  # exactly the cases that edge_scenes' docstring lists


def test_case_list_covers_the_families():
    fam = {f: len(E.family(f)) for f in REACH}
    assert fam == {"cold": 1, "scale": 12, "materials": 7, "normals": 1, "camera": 10, "bounces": 5, "samples": 1, "shapes": 8}
    assert {c.env.width for c in E.cases()} == {64, 100}  # one non-power-of-two environment, on suzanne (a walk kernel) too
    assert any(c.env.width == 100 and len(c.scene.triangles) > 64 for c in E.cases())
    for c in E.cases():
        assert c.w * c.h <= 64 * 40 and c.sample_count <= (15 if c.family == "samples" else 4)
        assert c.max_bounces <= 10 or c.family == "bounces"


# ---------------------------------------------------------------------------------------------------- host preprocessing
def _toml_number(x):
    x = float(x)
    return "nan" if x != x else repr(x)


def test_loader_keeps_edge_material_rows(tmp_path):
    """The material rows of the grid, and NaN roughness / NaN metallic, through the product's TOML loader and the independent reader:
    the same f32 bits (subnormal 1e-42, 3e38, negative values and NaN included), so upload sees what the file says."""
    rows = [E.grid_materials(r) for r in E.ROUGHNESS]
    extra = np.zeros(2, T.MATERIAL)
    extra["color"], extra["roughness"], extra["metallic"] = 0.5, [np.nan, 0.5], [0.5, np.nan]
    mats = np.concatenate(rows + [extra])
    text = []
    for i, m in enumerate(mats):
        text.append("[[material]]\nname = \"m%d\"\ncolor = [%s]\nroughness = %s\nmetallic = %s\nemission = [%s]\n" % (
            i, ", ".join(_toml_number(x) for x in m["color"]), _toml_number(m["roughness"]), _toml_number(m["metallic"]),
            ", ".join(_toml_number(x) for x in m["emission"])))
    text.append("[[object]]\n[object.Sphere]\nmaterial = \"m0\"\npos = [0, 0, 0]\nradius = 1\n[camera]\npos = [0, 0, 3]\nyaw = 0\npitch = 0\nfov_y = 60\n")
    p = tmp_path / "grid.toml"
    p.write_text("".join(text))
    got = R.Scene.load_toml(str(p)).materials
    ref = scene_py.load_toml(str(p))["scene"].materials
    assert len(got) == len(mats) == 7 * 64 + 2
    for key in ("color", "roughness", "metallic", "emission"):
        assert util.same_bits_or_nan(got[key], mats[key]), key
        assert util.same_bits_or_nan(got[key], ref[key]), key
    assert np.isnan(got["roughness"][-2]) and np.isnan(got["metallic"][-1])
    assert (np.abs(got["emission"][got["emission"] != 0]) < TINY).any()


def test_plane_and_camera_uniforms_of_edge_inputs_match_the_checker():
    for pos, yaw, pitch, fov in E.EDGE_CAMERA_DESCS:
        a = R.camera_uniform(host.make_camera_desc(pos, yaw, pitch, fov))
        b = oracle.camera_uniform(F(pos), float(F(yaw)), float(F(pitch)), float(F(fov)))
        for ka, kb in zip(a.dtype.names, b.dtype.names):
            assert util.same_bits_or_nan(a[ka], b[kb]), (pos, yaw, pitch, fov, ka)
    # a rounded pi / 2 does not give the exact pole (the reason for edge_scenes.pole_camera)
    up = R.camera_uniform(host.make_camera_desc((0, 1, 3), 0.0, float(E.HALF_PI), 1.2))
    c = E.centre_ray(up[0])
    assert c[1] == 1 and c[2] != 0 and abs(c[2]) < 1e-7
    seen = set()
    for name in ("default", "house"):
        for k in E.SCALES + [0, 40, -40]:
            if name == "house" and k not in (-70, 64):
                continue
            sc = E.scaled_scene(name, k)
            want = oracle.plane_to_uniform(sc.plane_descs.view(oracle.PLANE_SRC))
            for ka, kb in zip(sc.planes.dtype.names, want.dtype.names):
                assert util.same_bits_or_nan(sc.planes[ka], want[kb]), (name, k, ka)
            m = sc.planes["base_change_matrix"][:, :, :3]
            seen |= {"nan"} if np.isnan(sc.planes["normal"]).any() else set()
            seen |= {"inf"} if np.isinf(m).any() else set()
    assert seen == {"nan", "inf"}, seen  # what the scaled planes do reach: forward x right under- or overflows, 0 * inf, 1 / 0


@pytest.mark.parametrize("name", ["default", "suzanne", "house"])
def test_host_bvh_of_scaled_scenes_matches_the_checker_node_for_node(name):
    """Surface areas overflow or vanish at these scales, so the SAH comparisons see inf, 0 and NaN."""
    for k in E.SCALES:
        sc = E.scaled_scene(name, k)
        p, n, depth = oracle.build_bvh(sc.spheres.view(oracle.SPHERE), sc.plane_descs.view(oracle.PLANE_SRC), sc.vertices.view(oracle.VEC3),
                                       sc.triangles.view(oracle.TRIANGLE))
        assert util.fields_equal(sc.primitives, p) and sc.bvh_depth == depth, (name, k)
        assert len(sc.bvh_nodes) == len(n)
        for ka, kb in zip(sc.bvh_nodes.dtype.names, n.dtype.names):
            assert util.same_bits_or_nan(sc.bvh_nodes[ka].astype(np.float32), n[kb].astype(np.float32)), (name, k, ka)
            assert np.array_equal(sc.bvh_nodes[ka], n[kb]) or ka.startswith("bounds"), (name, k, ka)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            e = sc.bvh_nodes["bounds_max"][0] - sc.bvh_nodes["bounds_min"][0]
            area = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
        # the root box's area, about 2^7 * 4^k: subnormal, barely normal, inf, inf
        assert {-70: 0 < area < TINY, -63: TINY <= area < TINY * F(2.0) ** 16, 61: np.isinf(area), 64: np.isinf(area)}.get(k, np.isfinite(area) and area > TINY), (name, k, area)
