"""The BVH builders at degenerate inputs, without a GPU: tests/bvh_ref.py — a numpy restatement of the reference's build_bvh that
knows where the median fallback is reached — against the host builder and the checker's, field for field, on the shipped scenes, the
25 random scenes of test_host_preprocess.py and every case of tests/edge_trees.py that does not fall back; the fallback flag on the
ones that do; and what kernel selection (rsrt_scene_image_build) makes of the trees these inputs give."""
import numpy as np
import pytest

import bvh_ref
import edge_trees as ET
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host, types as T

FALLBACK = {"span_overflow", "span_overflow_beside"}  # (asserted from bvh_ref below, not assumed)
NAMES = [c.name for c in ET.cases()]


def three_builders(sph, pls, verts, tri):
    ref = bvh_ref.build(sph, pls, verts, tri)
    h = host.build_bvh(sph, pls, verts, tri)
    o = oracle.build_bvh(sph.view(oracle.SPHERE), pls.view(oracle.PLANE_SRC), verts.view(oracle.VEC3), tri.view(oracle.TRIANGLE))
    return ref, h, o


def assert_same(ref, other, what):
    p, n, d, fb = ref
    assert fb == 0, what
    assert util.fields_equal(p, other[0]), what
    assert util.fields_equal(n, other[1]), what
    assert d == other[2], what


@pytest.mark.parametrize("name", ["house", "default", "cube", "suzanne", "spheres_only"])
def test_restatement_on_the_shipped_scenes(name):
    sc = R.Scene.load_toml(util.scene_path(name))
    ref, h, o = three_builders(sc.spheres, sc.plane_descs, sc.vertices, sc.triangles)
    assert_same(ref, h, "host")
    assert_same(ref, o, "checker")
    assert_same(ref, (sc.primitives, sc.bvh_nodes, sc.bvh_depth), "loader")


def test_restatement_on_the_random_scenes():
    rng = np.random.default_rng(7)  # the 25 scenes of test_host_preprocess.py::test_bvh_random_scenes_match_oracle
    for trial in range(25):
        ns, npl, nt = rng.integers(0, 12), rng.integers(0, 4), rng.integers(0, 60)
        if ns + npl + nt == 0:
            ns = 1
        sph = np.zeros(ns, T.SPHERE)
        sph["pos"] = rng.uniform(-5, 5, (ns, 3))
        sph["radius"] = rng.uniform(0.05, 1.5, ns)
        pls = np.zeros(npl, T.PLANE_DESC)
        pls["pos"] = rng.uniform(-5, 5, (npl, 3))
        pls["forward"] = rng.uniform(-3, 3, (npl, 3))
        pls["right"] = rng.uniform(-3, 3, (npl, 3))
        verts = np.zeros(max(3, nt), T.VEC3)
        verts["v"] = np.round(rng.uniform(-4, 4, (len(verts), 3)) * (2 if trial % 2 else 64)) / (2 if trial % 2 else 64)
        tri = np.zeros(nt, T.TRIANGLE)
        for k in ("vertex_0", "vertex_1", "vertex_2"):
            tri[k] = rng.integers(0, len(verts), nt)
        ref, h, o = three_builders(sph, pls, verts, tri)
        assert_same(ref, h, ("host", trial))
        assert_same(ref, o, ("checker", trial))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_on_the_catalogue(name):
    c = ET.case(name)
    ref = bvh_ref.build(c.spheres, c.plane_descs, c.vertices, c.triangles)
    if name in FALLBACK:
        assert ref[3] > 0 and ref[0] is None
        return
    _, h, o = three_builders(c.spheres, c.plane_descs, c.vertices, c.triangles)
    assert_same(ref, h, "host")
    assert_same(ref, o, "checker")


# nodes, depth and longest leaf of every built case: bvh_ref's trees (the device builder's report, test_edge_trees_gpu.py, shows the same)
SHAPE = {
    "count_1_sphere": (1, 0, 1), "count_1_plane": (1, 0, 1), "count_1_triangle": (1, 0, 1), "count_2_sphere": (1, 0, 2),
    "count_2_plane": (1, 0, 2), "count_2_triangle": (1, 0, 2), "count_5": (1, 0, 5), "count_6": (3, 1, 4), "count_7": (3, 1, 4),
    "count_255": (143, 7, 5), "count_256": (139, 8, 5), "count_257": (143, 8, 5), "count_511": (277, 9, 5), "count_512": (281, 9, 5),
    "count_513": (285, 9, 5), "count_1025": (561, 10, 5), "classes_sorted_513": (273, 8, 5), "classes_reversed_513": (285, 8, 5),
    "classes_alternating_513": (281, 9, 5), "classes_left_last_513": (283, 9, 5), "classes_right_first_513": (277, 9, 5),
    "classes_L255_513": (281, 8, 5), "classes_L256_513": (283, 8, 5), "classes_L257_513": (281, 8, 5), "classes_L1_513": (283, 10, 5),
    "classes_Lnm1_513": (289, 10, 5), "concentric_6": (1, 0, 6), "concentric_7": (1, 0, 7), "concentric_9": (1, 0, 9),
    "concentric_300": (1, 0, 300), "stacks_9": (5, 2, 9), "stacks_100": (5, 2, 100), "two_points_32": (3, 1, 32),
    "coincident_250x8": (499, 11, 8), "coincident_250x9": (499, 11, 9), "line_x_600": (255, 7, 5), "line_y_600": (255, 7, 5),
    "line_z_600": (255, 7, 5), "grid_xy_600": (399, 8, 4), "tie_xy": (21, 4, 5), "tie_xz": (21, 4, 5), "tie_yz": (21, 5, 5),
    "tie_xyz": (21, 4, 5), "chain_40": (31, 15, 5), "chain_120": (75, 37, 5), "subnormal_line": (49, 23, 5), "far_corner": (13, 4, 5),
}


def test_catalogue_cases_are_what_they_say():
    """The shapes the catalogue's lines promise, read off bvh_ref's trees."""
    tree = {c.name: bvh_ref.build(c.spheres, c.plane_descs, c.vertices, c.triangles) for c in ET.cases()}
    assert {n for n, t in tree.items() if t[3]} == FALLBACK
    for n in ET.COUNTS:
        for c in [c for c in ET.cases() if c.name == "count_%d" % n or c.name.startswith("count_%d_" % n)]:
            assert len(tree[c.name][0]) == n and (len(tree[c.name][1]) == 1) == (n <= 5)
    for c in ET.cases():  # the class string is the input order, and the root cuts between the clusters
        if c.name.startswith("classes_"):
            is_left = c.spheres["pos"][:, 0] < 50
            assert bvh_ref.root_split(c.spheres, c.plane_descs, c.vertices, c.triangles) == int(is_left.sum()), c.name
            assert tree[c.name][1][0]["split_axis"] == 0
    for name, L in (("classes_sorted_513", 256), ("classes_reversed_513", 256), ("classes_alternating_513", 257), ("classes_left_last_513", 1),
                    ("classes_right_first_513", 512), ("classes_L255_513", 255), ("classes_L256_513", 256), ("classes_L257_513", 257),
                    ("classes_L1_513", 1), ("classes_Lnm1_513", 512)):
        c = ET.case(name)
        assert int((c.spheres["pos"][:, 0] < 50).sum()) == L
    x = ET.case("classes_sorted_513").spheres["pos"][:, 0] < 50
    assert x[:256].all() and not x[256:].any()
    x = ET.case("classes_reversed_513").spheres["pos"][:, 0] < 50
    assert x[-256:].all() and not x[:-256].any()
    x = ET.case("classes_left_last_513").spheres["pos"][:, 0] < 50
    assert x[-1] and not x[:-1].any()
    x = ET.case("classes_right_first_513").spheres["pos"][:, 0] < 50
    assert not x[0] and x[1:].all()
    shape = {n: (len(t[1]), t[2], ET.longest_leaf(t[1])) for n, t in tree.items() if not t[3]}  # nodes, depth, longest leaf
    assert shape == SHAPE
    assert shape["concentric_6"] == (1, 0, 6) and shape["concentric_7"] == (1, 0, 7) and shape["concentric_9"] == (1, 0, 9)
    assert shape["concentric_300"] == (1, 0, 300)
    assert shape["stacks_9"] == (5, 2, 9) and shape["stacks_100"] == (5, 2, 100) and shape["two_points_32"] == (3, 1, 32)
    assert shape["coincident_250x8"][2] == 8 and shape["coincident_250x9"][2] == 9
    for a in "xyz":
        assert tree["line_%s_600" % a][1][0]["split_axis"] == "xyz".index(a) and shape["line_%s_600" % a][2] <= 5
    assert tree["grid_xy_600"][1][0]["split_axis"] == 0
    assert [int(tree[n][1][0]["split_axis"]) for n in ("tie_xy", "tie_xz", "tie_yz", "tie_xyz")] == [0, 0, 1, 0]
    assert shape["chain_40"][1] == 15 and shape["chain_120"][1] == 37
    sub = ET.case("subnormal_line")
    assert np.all(sub.spheres["pos"][1:, 0] < np.finfo(np.float32).tiny) and shape["subnormal_line"][0] > 1 and shape["subnormal_line"][2] <= 5
    assert shape["far_corner"][0] > 1
    print("\n".join("%-24s %5d nodes, depth %2d, longest leaf %3d" % ((n,) + s) for n, s in shape.items()))


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_host_builder_takes_the_median_where_the_restatement_falls_back(name):
    """Below the median split the order is the standard library's, so there is no tree to compare with: the host builder's is a valid
    one — every item in exactly one leaf, boxes that hold their items, the root split in halves on x."""
    c = ET.case(name)
    a = (c.spheres, c.plane_descs, c.vertices, c.triangles)
    prims, nodes, depth = host.build_bvh(*a)
    typ, idx, mn, mx = bvh_ref.item_bounds(*a)
    n = len(typ)
    assert sorted(zip(prims["primitive_type"].tolist(), prims["index"].tolist())) == sorted(zip(typ.tolist(), idx.tolist()))
    leaves = nodes[nodes["primitives_len"] > 0]
    leaves = leaves[np.argsort(leaves["primitives_or_second_child_index"])]  # ranges that tile [0, n)
    ends = np.cumsum(leaves["primitives_len"].astype(np.int64))
    assert ends[-1] == n and np.array_equal(leaves["primitives_or_second_child_index"], np.r_[0, ends[:-1]])
    row = {(int(t), int(i)): k for k, (t, i) in enumerate(zip(typ, idx))}
    for lf in leaves:
        for r in prims[int(lf["primitives_or_second_child_index"]):][:int(lf["primitives_len"])]:
            k = row[int(r["primitive_type"]), int(r["index"])]
            assert (lf["bounds_min"] <= mn[k]).all() and (mx[k] <= lf["bounds_max"]).all()
    second = int(nodes[0]["primitives_or_second_child_index"])
    assert nodes[0]["primitives_len"] == 0 and nodes[0]["split_axis"] == 0 and int(nodes["primitives_len"][1:second].sum()) == n // 2
    if name == "span_overflow":
        assert (len(nodes), depth) == (3, 1)


def test_closed_form_partition_on_the_catalogue_s_class_strings():
    """test_bvh_device.py checks the device builder's closed form of the two-pointer partition on random strings of at most 40 items;
    here on the chosen ones, 513 long, whose L sits on the edges of the builder's 256-item chunks."""
    from test_bvh_device import closed_form_partition, sequential_partition
    n = 0
    for c in ET.cases():
        if c.name.startswith("classes_"):
            cls = (c.spheres["pos"][:, 0] < 50).tolist()
            assert closed_form_partition(cls) == sequential_partition(cls), c.name
            n += 1
    assert n == 10


# ---------------------------------------------------------------------------------------------------- kernel selection
# What rsrt_scene_image_build reports for each built case as a scene (ET.scene): n_nodes, flat_ok, typed_leaves, wide_ok, wide_deep,
# coop_ok, lds_float4s != 0 — produced by that function and written down here, not computed by the test.
SELECTION = {
    "count_1_sphere": (1, 1, 1, 0, 0, 0, 1),
    "count_1_plane": (1, 1, 1, 0, 0, 0, 1),
    "count_1_triangle": (1, 1, 1, 0, 0, 0, 1),
    "count_2_sphere": (1, 1, 1, 0, 0, 0, 1),
    "count_2_plane": (1, 1, 1, 0, 0, 0, 1),
    "count_2_triangle": (1, 1, 1, 0, 0, 0, 1),
    "count_5": (1, 1, 1, 0, 0, 0, 1),
    "count_6": (3, 1, 1, 1, 0, 1, 1),
    "count_7": (3, 1, 1, 1, 0, 1, 1),
    "count_255": (143, 0, 1, 1, 0, 1, 0),
    "count_256": (139, 0, 1, 1, 0, 1, 0),
    "count_257": (143, 0, 1, 1, 0, 1, 0),
    "count_511": (277, 0, 1, 1, 0, 1, 0),
    "count_512": (281, 0, 1, 1, 0, 1, 0),
    "count_513": (285, 0, 1, 1, 0, 1, 0),
    "count_1025": (561, 0, 1, 1, 0, 1, 0),
    "classes_sorted_513": (273, 0, 1, 1, 0, 1, 0),
    "classes_reversed_513": (285, 0, 1, 1, 0, 1, 0),
    "classes_alternating_513": (281, 0, 1, 1, 0, 1, 0),
    "classes_left_last_513": (283, 0, 1, 1, 0, 1, 0),
    "classes_right_first_513": (277, 0, 1, 1, 0, 1, 0),
    "classes_L255_513": (281, 0, 1, 1, 0, 1, 0),
    "classes_L256_513": (283, 0, 1, 1, 0, 1, 0),
    "classes_L257_513": (281, 0, 1, 1, 0, 1, 0),
    "classes_L1_513": (283, 0, 1, 1, 0, 1, 0),
    "classes_Lnm1_513": (289, 0, 1, 1, 0, 1, 0),
    "concentric_6": (1, 1, 1, 0, 0, 0, 1),
    "concentric_7": (1, 1, 1, 0, 0, 0, 1),      # a one-node tree: no wide walk (it wants three nodes); the flat loop, typed leaves
    "concentric_9": (1, 1, 0, 0, 0, 0, 1),
    "concentric_300": (1, 0, 0, 0, 0, 0, 0),    # nothing but the generic tree walk, its one leaf's 300 records read from memory
    "stacks_9": (5, 1, 0, 0, 0, 0, 1),          # the flat loop over leaves of 9
    "stacks_100": (5, 0, 0, 0, 0, 0, 0),
    "two_points_32": (3, 1, 0, 0, 0, 0, 1),
    "coincident_250x8": (499, 0, 1, 1, 0, 1, 0),
    "coincident_250x9": (499, 0, 0, 0, 0, 0, 0),
    "line_x_600": (255, 0, 1, 1, 0, 1, 0),
    "line_y_600": (255, 0, 1, 1, 0, 1, 0),
    "line_z_600": (255, 0, 1, 1, 0, 1, 0),
    "grid_xy_600": (399, 0, 1, 1, 0, 1, 0),
    "tie_xy": (21, 1, 1, 1, 0, 1, 1),
    "tie_xz": (21, 1, 1, 1, 0, 1, 1),
    "tie_yz": (21, 1, 1, 1, 0, 1, 1),
    "tie_xyz": (21, 1, 1, 1, 0, 1, 1),
    "chain_40": (31, 1, 1, 1, 0, 1, 1),
    "chain_120": (75, 0, 1, 1, 1, 1, 1),        # a wide tree deeper than the walk's stack registers
    "subnormal_line": (49, 1, 1, 1, 0, 1, 1),
    "far_corner": (13, 1, 1, 1, 0, 1, 1),
}


def image_info(name):
    from test_scene_image import arrays, build
    built = build(arrays(ET.scene(name)))
    assert not isinstance(built, str), (name, built)
    return built[1]


def test_selection_table_covers_every_built_case():
    assert set(SELECTION) == set(NAMES) - FALLBACK


@pytest.mark.parametrize("name", sorted(SELECTION))
def test_kernel_selection_of_the_builder_s_trees(name):
    from test_wide_tree import wide_tree
    i = image_info(name)
    assert (i.n_nodes, i.flat_ok, i.typed_leaves, i.wide_ok, i.wide_deep, i.coop_ok, int(i.lds_float4s != 0)) == SELECTION[name]
    assert (wide_tree(ET.scene(name)) is None) == (not i.wide_ok)  # rsrt_wide_tree_build refuses exactly the trees the image has no wide nodes for


# ---------------------------------------------------------------------------------------------------- the probe's rule, the cameras
REFUSALS = {"lds": "this scene is not staged in LDS by the production kernel", "coop": "the cooperative walk needs", "wide": "the wide walk needs",
            "typed": "typed leaf loops need", "flat": "the flat traversal needs"}


def probe_refusal(i, mode):
    """Which documented message rsrt_cast_rays must refuse `mode` with for a scene whose image info is `i` (a key of REFUSALS), or
    None: include/rsrt.h's rule, from the info alone.  The LDS forms come first: a scene whose whole image is not in LDS is staged
    per traversal — the wide walks the head of the wide nodes (none without a wide tree), the fixed-order walk its top block, the tree
    walks nodes + escape links when they take at most 40 KiB and fit beside the stack walk's stack."""
    sel = mode >> 1 & 7  # 0 threaded, 1 stack, 2 typed leaf loops, 3 flat, 4 fixed-order, 5 wide, 6 cooperative
    staged_per_traversal = False
    if mode & 16 and not i.lds_float4s:
        if sel >= 5:
            staged = i.wimg_nodes > 0
        elif sel == 4:
            staged = i.top_elems > 0
        else:
            room = 160 * 1024 // 16 - (i.stack_entries * 256 * 4 + 15) // 16 * (sel == 1)
            staged = 0 < i.traversal_head_f4 <= min(40 * 1024 // 16, room)
        if not staged:
            return "lds"
        staged_per_traversal = True
    if sel == 6 and not (i.wide_ok and i.coop_ok):
        return "coop"
    if sel == 5 and not i.wide_ok:
        return "wide"
    if sel in (2, 4) and not i.typed_leaves:
        return "typed"
    if sel == 3 and (not i.flat_ok or staged_per_traversal):
        return "flat"
    return None


W, H, SPP, BOUNCES = 48, 32, 2, 4


def reference(name):
    """The checker's answers for a traversed scene, computed once and shared (callers must not write into them): image sums, counters,
    AOV records, and the probe rays' closest hits for cast_ray and cast_ray_bvh."""
    import denoise_ref as D
    if name not in reference.cache:
        sc, env = ET.scene(name), util.small_env()
        osc, cam = util.oracle_scene(sc), sc.camera_uniform()
        img, ost = oracle.render(osc, util.oracle_env(env), cam.view(oracle.CAMERA), W, H, 0, SPP, BOUNCES)
        aov = D.aov_records(sc, osc, cam[0], W, H, 0, SPP)
        o, d = ET.probe_rays(name)
        hits = [oracle.cast_rays(osc, o, d, b, 0) for b in (0, 1)]
        for a in [img, aov] + hits:
            a.setflags(write=False)
        reference.cache[name] = (img, ost, aov, hits)
    return reference.cache[name]


reference.cache = {}


@pytest.mark.parametrize("name", ET.TRAVERSED)
def test_traversed_scenes_are_seen_and_hit(name):
    """The conditions of test_edge_trees_gpu.py's comparisons, from the checker's own answers: its first hits cover a quarter of the
    pixels or more, at least half of the probe's rays hit, light is sampled, and everything is finite (so bits can be compared)."""
    img, ost, aov, hits = reference(name)
    assert np.isfinite(img).all() and np.isfinite(aov).all()
    assert 4 * int((aov[..., 3] > 0).sum()) >= W * H
    assert ost["shadow_rays"] > 0
    for h in hits:
        hit = h["did_hit"] != 0
        assert 2 * int(hit.sum()) >= len(h)
        assert np.isfinite(h["distance"][hit]).all() and np.isfinite(h["hit_point"][hit]).all()


def test_traversed_scenes_cover_the_outcomes_of_selection():
    """One scene per way production takes a tree: the flat loop with typed and with long leaves, the generic tree walk over long leaves
    (one node; five nodes; hundreds), the walks of a shallow and of a deep wide tree from a whole image, and of a tree too big for one."""
    got = {n: SELECTION[n][1:] for n in ET.TRAVERSED}
    assert got == {"concentric_7": (1, 1, 0, 0, 0, 1), "concentric_300": (0, 0, 0, 0, 0, 0), "stacks_9": (1, 0, 0, 0, 0, 1),
                   "stacks_100": (0, 0, 0, 0, 0, 0), "chain_40": (1, 1, 1, 0, 1, 1), "chain_120": (0, 1, 1, 1, 1, 1),
                   "coincident_250x9": (0, 0, 0, 0, 0, 0), "count_257": (0, 1, 1, 0, 1, 0)}
    # equal hits inside one long leaf: the nine copies of a triangle carry different materials, so which of them wins shows in every
    # record and pixel (the checker keeps the first of equals in leaf order; the GPU tests compare with it bit for bit)
    sc = ET.scene("coincident_250x9")
    assert all(len({int(m) for m in sc.triangles["material_id"][k:k + 9]}) == len(ET.MATERIALS) for k in range(0, len(sc.triangles), 9))
    hit = reference("coincident_250x9")[3][0]
    assert len({int(m) for m in hit["material_id"][hit["did_hit"] != 0]}) > 1
