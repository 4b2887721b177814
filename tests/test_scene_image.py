"""The scene's device image (csrc/hip/rt_scene_image.h build_scene_image; rsrt_upload_scene copies it to the device, and
rsrt_scene_image_build hands it out on the CPU): every byte of it and of its layout struct against digests recorded from the
verbatim builder (tests/golden/scene_image_digests.json), and the Python restatements the other tests carry — the flat loop's octant
tables, its cull groups, the wide tree, a near-child-first walk for the ranks and escape links — against what the library really
builds.  No GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import test_flat_oriented as FO
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import state, types as T
from test_flat_shade_gen_gpu import cull_groups
from test_wide_tree import wide_tree

RT_END = 0x1FFFFFF  # rt_device.h: the traversal cursor's end mark
GOLDEN = ("cube", "default", "house", "spheres_only", "suzanne")
FLAT = ("cube", "default", "house", "spheres_only")  # the golden scenes the flat loop takes
DIGESTS = os.path.join(util.ROOT, "tests", "golden", "scene_image_digests.json")


def arrays(sc):
    return [sc.materials, sc.spheres, sc.planes, sc.vertices, sc.normals, sc.triangles, sc.primitives, sc.bvh_nodes]


def build(a, flat_oriented=1, n_nodes=None):
    """rsrt_scene_image_build over the eight arrays `a`: (image as (n, 4) float32, info), or the refusal's message."""
    L = state.lib()
    a = [np.ascontiguousarray(x) for x in a]
    args = []
    for x in a:
        args += [x.ctypes.data_as(C.c_void_p) if x.size else None, len(x)]
    if n_nodes is not None:
        args[-1] = n_nodes
    n, info = C.c_size_t(0), state.SceneImageInfo()
    if L.rsrt_scene_image_build(*args, flat_oriented, None, C.byref(n), C.byref(info)) != 0:
        return L.rsrt_last_error(None).decode()
    img = np.zeros((n.value, 4), np.float32)
    assert n.value == info.n_float4
    assert L.rsrt_scene_image_build(*args, flat_oriented, img.ctypes.data_as(C.c_void_p), C.byref(n), None) == 0
    return img, info


def golden_scene(name):
    """The scene of tests/golden/scene_<name>.npz: the arrays of its .toml under the tree the file pins."""
    sc = R.Scene.load_toml(util.scene_path(name))
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "scene_%s.npz" % name))
    prims = np.ascontiguousarray(g["bvh_prims"]).view(T.PRIMITIVE_INFO).reshape(-1)
    nodes = np.ascontiguousarray(g["bvh_nodes"]).view(T.BVH_NODE).reshape(-1)
    return R.Scene(sc.materials, sc.spheres, sc.plane_descs, sc.vertices, sc.normals, sc.triangles, sc.camera_desc, planes=sc.planes,
                   primitives=prims, bvh_nodes=nodes, bvh_depth=int(g["depth"]))


def with_tree(sc, prims, nodes):
    return R.Scene(sc.materials, sc.spheres, sc.plane_descs, sc.vertices, sc.normals, sc.triangles, sc.camera_desc, planes=sc.planes,
                   primitives=prims, bvh_nodes=nodes, bvh_depth=1)


def one_node_scene():
    """spheres_only under a single leaf that holds every record"""
    sc = golden_scene("spheres_only")
    nodes = sc.bvh_nodes[:1].copy()
    nodes["primitives_or_second_child_index"], nodes["primitives_len"] = 0, len(sc.primitives)
    return with_tree(sc, sc.primitives, nodes)


def shared_record_scene():
    """Three records of default under a root and two leaves of two records each: record 1 is in both."""
    sc = golden_scene("default")
    nodes = np.zeros(3, T.BVH_NODE)
    nodes["bounds_min"], nodes["bounds_max"] = sc.bvh_nodes[0]["bounds_min"], sc.bvh_nodes[0]["bounds_max"]
    nodes["primitives_or_second_child_index"], nodes["primitives_len"] = [2, 0, 1], [0, 2, 2]
    return with_tree(sc, sc.primitives[:3].copy(), nodes)


CASES = {name: (lambda tmp, name=name: golden_scene(name), 1) for name in GOLDEN}
CASES.update({
    "grid": (lambda tmp: R.Scene.load_toml(util.big_scene(tmp, 4)), 1),
    "deck": (lambda tmp: util.deck_scene(), 1),
    "deck_deep": (lambda tmp: util.deck_scene(42), 1),  # more wide levels than the walk has stack registers
    "fan": (lambda tmp: util.fan_scene(), 1),
    "long_leaf": (lambda tmp: util.long_leaf_scene(), 1),
    "house_unoriented": (lambda tmp: golden_scene("house"), 0),
    "house_without_room": (lambda tmp: FO._house_without_room(), 1),
    "one_node": (lambda tmp: one_node_scene(), 1),
    "shared_record": (lambda tmp: shared_record_scene(), 1),
})


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """case -> (scene, image, info), each built once"""
    out = {}
    for name, (make, oriented) in CASES.items():
        sc = make(tmp_path_factory.mktemp(name))
        img, info = build(arrays(sc), oriented)
        out[name] = (sc, img, info)
    return out


def digests(img, info):
    return {"image": hashlib.sha256(img.tobytes()).hexdigest(), "info": hashlib.sha256(bytes(info)).hexdigest()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_and_layout_are_the_recorded_ones(name, built):
    with open(DIGESTS) as f:
        want = json.load(f)
    _, img, info = built[name]
    assert digests(img, info) == want[name]


def test_cases_take_the_paths_they_are_there_for(built):
    """Each table's special paths occur in a digest case: the flat loop with and without octant tables, twin records, jump elements and a
    hybrid head, a deep wide tree, long leaves, a one-node tree, a shared record."""
    info = {k: v[2] for k, v in built.items()}
    assert C.sizeof(state.SceneImageInfo) == 14 * 8 + 84 * 4
    assert all(info[k].flat_ok and info[k].flat_ostride == 2 * (info[k].n_leaves | 1) and info[k].lds_float4s for k in FLAT)
    assert info["house_unoriented"].flat_ok and info["house_unoriented"].flat_ostride == 0
    assert info["house_unoriented"].n_float4 == info["house"].n_float4 - 8 * info["house"].flat_ostride
    small = info["house"].small_image_bytes
    assert small == FO.SMALL_IMAGE_BYTES
    assert info["house_without_room"].flat_ok and info["house_without_room"].flat_ostride == 0
    assert 0 < info["house_without_room"].lds_float4s * 16 <= small < (info["house_without_room"].lds_float4s + 8 * 2 * (info["house_without_room"].n_leaves | 1)) * 16
    assert not info["suzanne"].flat_ok and info["suzanne"].wide_ok and info["suzanne"].coop_ok and info["suzanne"].lds_float4s == 0
    g = info["grid"]
    assert g.lds_float4s == 0 and g.wide_ok and g.wimg_nodes == g.n_wnodes
    assert g.n_pnodes > g.n_nodes and 2 * g.top_elems <= g.hybrid_room_f4 and g.top_elems < g.n_pnodes  # jump elements, more than the top block
    assert g.traversal_head_f4 == 2 * g.n_nodes + (8 * g.n_nodes + 3) // 4
    assert info["deck"].wide_ok and not info["deck"].wide_deep and info["deck_deep"].wide_ok and info["deck_deep"].wide_deep
    assert info["fan"].wide_ok and not info["fan"].flat_ok
    assert not info["long_leaf"].typed_leaves and not info["long_leaf"].wide_ok and all(info[k].typed_leaves for k in GOLDEN)
    o = info["one_node"]
    # (the leaf and a jump element to the end: the last leaf's successor is never "the next element")
    assert (o.n_nodes, o.n_leaves, o.n_pnodes, o.stack_entries, o.wide_ok, o.n_wnodes) == (1, 1, 2, 1, 0, 0) and o.flat_ok and o.n_cull == 0 and o.cull_always == 1
    s = info["shared_record"]
    assert not s.flat_ok and not s.wide_ok and s.cull_always == 0xFFFFFFFF and s.stack_entries == 2
    for k, i in info.items():
        sc = built[k][0]
        assert (i.n_nodes, i.n_prims, i.n_tris, i.n_materials, i.n_spheres, i.n_planes) == tuple(len(x) for x in (
            sc.bvh_nodes, sc.primitives, sc.triangles, sc.materials, sc.spheres, sc.planes))
        assert i.stack_entries == sc.bvh_depth + 1 or k not in GOLDEN + ("grid",)  # (the hand-made scenes state no exact depth)
        assert i.nodes == 0 and i.escape == 2 * i.n_nodes and i.prims == i.traversal_head_f4 and i.wnodes + 8 * i.n_wnodes == i.n_float4


def near_first_walk(nodes, q):
    """The reference's near-child-first walk for sign octant q, every box hit: {record: rank of its first visit}, {node: escape link}."""
    rank, esc, pos, stack = {}, {}, 0, [(0, RT_END)]
    while stack:
        i, e = stack.pop()
        esc[i] = e
        first, n = int(nodes[i]["primitives_or_second_child_index"]), int(nodes[i]["primitives_len"])
        for r in range(first, first + n):
            rank.setdefault(r, pos)
            pos += 1
        if n == 0:
            near, far = (first, i + 1) if (q >> int(nodes[i]["split_axis"])) & 1 else (i + 1, first)
            stack += [(far, e), (near, far)]
    return rank, esc


def words(img, at, n):
    """n u32 words of the image from float4 `at`"""
    return img.view(np.uint32).reshape(-1)[4 * at:4 * at + n]


def test_ranks_and_escape_links_are_the_near_first_walks(built):
    sc, img, info = built["default"]
    _, oon = wide_tree(sc)  # the image numbers the records as the wide tree does
    n_p, n_n = info.n_prims, info.n_nodes
    prim_rank = words(img, info.prim_rank, 8 * n_p).reshape(8, n_p)
    escape = words(img, info.escape, 8 * n_n).reshape(8, n_n)
    flat_rank = words(img, info.flat_rank, 8 * 16).view(np.uint8).reshape(8, 64)
    for q in range(8):
        rank, esc = near_first_walk(sc.bvh_nodes, q)
        assert sorted(rank.values()) == list(range(n_p))
        assert prim_rank[q].tolist() == [rank[int(oon[r])] for r in range(n_p)]
        assert flat_rank[q, :n_p].tolist() == prim_rank[q].tolist() and not flat_rank[q, n_p:].any()
        assert escape[q].tolist() == [esc[i] for i in range(n_n)]
    assert len({tuple(r) for r in prim_rank.tolist()}) > 1  # the octants differ


def test_shared_record_keeps_its_first_rank_and_uncovered_records_have_none(built):
    sc, img, info = built["shared_record"]
    prim_rank = words(img, info.prim_rank, 8 * 3).reshape(8, 3)
    for q in range(8):
        rank, _ = near_first_walk(sc.bvh_nodes, q)
        assert prim_rank[q].tolist() == [rank[r] for r in range(3)]
    assert {tuple(r) for r in prim_rank.tolist()} == {(0, 1, 3), (2, 0, 1)}  # record 1 met at position 1 and again at 2, or at 0 and 3
    # a record no leaf names: rank 0xffffffff in prim_rank, byte 0 in flat_rank
    base = golden_scene("cube")
    nodes = base.bvh_nodes.copy()
    leaf = max(i for i in range(len(nodes)) if nodes[i]["primitives_len"] > 1)
    nodes["primitives_len"][leaf] -= 1
    lost = int(nodes[leaf]["primitives_or_second_child_index"]) + int(nodes[leaf]["primitives_len"])
    img, info = build(arrays(with_tree(base, base.primitives, nodes)))
    assert info.flat_ok and not info.wide_ok  # (the wide tree wants every record covered: no permutation)
    prim_rank = words(img, info.prim_rank, 8 * info.n_prims).reshape(8, -1)
    flat_rank = words(img, info.flat_rank, 8 * 16).view(np.uint8).reshape(8, 64)
    assert (prim_rank[:, lost] == 0xFFFFFFFF).all() and (flat_rank[:, lost] == 0).all()
    keep = [r for r in range(info.n_prims) if r != lost]
    assert (flat_rank[:, keep] == prim_rank[:, keep]).all()


@pytest.mark.parametrize("name", FLAT)
def test_octant_tables_are_the_restated_ones(name, built):
    """test_flat_oriented.build_tables against the tables behind the leaf list, and the leaf list's masks: a leaf's records, without
    those that repeat an earlier record of the leaf (the records the cooperative walk's r2.w word marks)."""
    sc, img, info = built[name]
    n = info.n_leaves
    leaves = img[info.flat_leaves:info.flat_leaves + 2 * n]
    lo, hi = leaves[0::2, :3], leaves[1::2, :3]
    ml, mh = leaves[0::2, 3].copy().view(np.uint32), leaves[1::2, 3].copy().view(np.uint32)
    t, stride = FO.build_tables(lo, hi, ml, mh)
    assert stride == info.flat_ostride
    got = img[info.flat_leaves + 2 * n:info.flat_leaves + 2 * n + 8 * stride]
    used = np.zeros(8 * stride, bool)
    for q in range(8):
        used[q * stride:q * stride + 2 * n] = True
    assert np.array_equal(got[used].view(np.uint32), t[used].view(np.uint32)) and not got[~used].view(np.uint32).any()
    assert info.flat_rank == info.flat_leaves + 2 * n + 8 * stride == info.lds_float4s
    marks = words(img, info.prims, 16 * info.n_prims).reshape(-1, 16)[:, 11]  # r2.w
    assert set(marks.tolist()) <= {0, 1} and (marks.sum() > 0) == (name == "house")  # house lists its ground plane twice
    node_words = words(img, info.nodes, 8 * info.n_nodes).reshape(-1, 8)
    leaf_nodes = [i for i in range(info.n_nodes) if sc.bvh_nodes[i]["primitives_len"] > 0]
    assert len(leaf_nodes) == n
    for k, i in enumerate(leaf_nodes):
        first, ln = int(node_words[i, 3]), int(node_words[i, 7]) & 0xFFFF
        want = sum(1 << r for r in range(first, first + ln) if not marks[r])
        assert (int(mh[k]) << 32 | int(ml[k])) == want, (name, k)
        assert np.array_equal(lo[k], sc.bvh_nodes[i]["bounds_min"][:3]) and np.array_equal(hi[k], sc.bvh_nodes[i]["bounds_max"][:3])


def test_unoriented_image_is_the_oriented_one_without_its_tables(built):
    a, b = built["house"], built["house_unoriented"]
    cut, n = a[2].flat_leaves + 2 * a[2].n_leaves, 8 * a[2].flat_ostride
    assert np.array_equal(np.delete(a[1], np.s_[cut:cut + n], axis=0).view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("name", FLAT + ("one_node",))
def test_cull_groups_are_the_restated_ones(name, built):
    sc, _, info = built[name]
    always, groups, n_leaves = cull_groups(sc)
    assert (info.cull_always, info.n_cull, info.n_leaves) == (always, len(groups), n_leaves)
    for k, (lo, hi, m) in enumerate(groups):
        assert info.cull_mask[k] == m
        assert np.array_equal(np.array(info.cull_min[k][:], np.float32), lo[:3]) and np.array_equal(np.array(info.cull_max[k][:], np.float32), hi[:3])
    for k in range(len(groups), 8):
        assert info.cull_mask[k] == 0 and not any(info.cull_min[k][:]) and not any(info.cull_max[k][:])


@pytest.mark.parametrize("name", ["default", "suzanne", "grid"])
def test_wide_section_is_what_the_wide_tree_entry_point_returns(name, built):
    sc, img, info = built[name]
    wn, _ = wide_tree(sc)
    assert info.wide_ok and info.n_wnodes == len(wn)
    assert np.array_equal(img[info.wnodes:info.wnodes + 8 * len(wn)].view(np.uint32), wn.reshape(-1, 4).view(np.uint32))


def test_refusals_say_why():
    sc = golden_scene("default")
    n_m, n_v, n_n, n_nodes = len(sc.materials), len(sc.vertices), len(sc.normals), len(sc.bvh_nodes)

    def refused(**changed):
        a = dict(zip(("materials", "spheres", "planes", "vertices", "normals", "triangles", "primitives", "bvh_nodes"), arrays(sc)))
        a.update(changed)
        r = build(list(a.values()))
        assert isinstance(r, str), "not refused"
        return r

    def edited(arr, i, field, value):
        arr = arr.copy()
        arr[field][i] = value
        return arr

    assert len(sc.spheres) and len(sc.planes) and len(sc.triangles)
    assert refused(spheres=edited(sc.spheres, 0, "material_id", n_m)) == "sphere 0: material_id %d out of range" % n_m
    assert refused(planes=edited(sc.planes, 0, "material_id", n_m + 1)) == "plane 0: material_id %d out of range" % (n_m + 1)
    assert refused(triangles=edited(sc.triangles, 2, "material_id", n_m)) == "triangle 2: material_id %d out of range" % n_m
    assert refused(triangles=edited(sc.triangles, 0, "vertex_1", n_v)) == "triangle 0: vertex index out of range"
    assert refused(triangles=edited(sc.triangles, 0, "normal_2", n_n)) == "triangle 0: normal index out of range"
    ty = int(sc.primitives[3]["primitive_type"])
    assert refused(primitives=edited(sc.primitives, 3, "index", 1 << 20)) == "primitive 3: type %d index %d out of range" % (ty, 1 << 20)
    assert refused(bvh_nodes=edited(sc.bvh_nodes, 0, "primitives_or_second_child_index", n_nodes)) == "bvh interior node 0: bad child index / axis"
    leaf = next(i for i in range(n_nodes) if sc.bvh_nodes[i]["primitives_len"] > 0)
    assert refused(bvh_nodes=edited(sc.bvh_nodes, leaf, "primitives_len", len(sc.primitives) + 1)) == "bvh leaf %d: primitive range out of bounds" % leaf
    four = np.zeros(4, T.BVH_NODE)  # 0 -> (1, 2), 1 -> (2, 3): node 2 is the second child of 0 and the first of 1
    four["primitives_or_second_child_index"], four["primitives_len"] = [2, 3, 0, 1], [0, 0, 1, 1]
    assert refused(bvh_nodes=four) == "bvh node 2 reachable twice"
    four["primitives_or_second_child_index"], four["primitives_len"] = [3, 0, 1, 2], [0, 1, 1, 1]  # 0 -> (1, 3): nobody names node 2
    assert refused(bvh_nodes=four) == "bvh node 2 is not reachable from the root"
    r = build(arrays(sc), n_nodes=RT_END)  # (refused by the count alone: the array is not read)
    assert r == "bvh_nodes: %d nodes exceed the 25-bit traversal cursor" % RT_END
    assert build(arrays(sc)[:7] + [sc.bvh_nodes[:0]]) == "bvh_nodes is empty"
    assert not isinstance(build(arrays(sc)), str)  # and the scene itself is taken


def test_capacity_is_checked_before_the_image_is_written():
    sc = golden_scene("cube")
    L = state.lib()
    args = []
    for x in arrays(sc):
        args += [x.ctypes.data_as(C.c_void_p) if x.size else None, len(x)]
    n = C.c_size_t(0)
    assert L.rsrt_scene_image_build(*args, 1, None, C.byref(n), None) == 0 and n.value > 0
    guard = np.full((n.value, 4), 7.0, np.float32)
    short = C.c_size_t(n.value - 1)
    assert L.rsrt_scene_image_build(*args, 1, guard.ctypes.data_as(C.c_void_p), C.byref(short), None) != 0
    assert short.value == n.value and (guard == 7.0).all()
