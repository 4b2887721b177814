"""Shared helpers of the test-suite: product <-> oracle array views, small environments, metrics."""
import os
import sys

import numpy as np

import oracle
import rsoderh_raytracing_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "assets")


def scene_path(name):
    return os.path.join(ASSETS, "scenes", name + ".toml")


def big_scene(out_dir, n=4):
    """tools/make_big_scene.py's suzanne grid (n x n instances), written into `out_dir` — a test's own tmp_path, never a fixed
    shared directory that another user or another run may hold."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_big_scene
    return make_big_scene.make(n, str(out_dir))


def oracle_scene(scene):
    """oracle.Scene over the product Scene's arrays (identical encase layouts)."""
    return oracle.Scene(materials=scene.materials.view(oracle.MATERIAL), spheres=scene.spheres.view(oracle.SPHERE),
                        planes=scene.planes.view(oracle.PLANE), vertices=scene.vertices.view(oracle.VEC3),
                        normals=scene.normals.view(oracle.VEC3), triangles=scene.triangles.view(oracle.TRIANGLE),
                        prims=scene.primitives.view(oracle.PRIM_INFO), nodes=scene.bvh_nodes.view(oracle.BVH_NODE))


def oracle_env(env):
    return oracle.Env(env.rgba, env.alias.view(oracle.ALIAS_ENTRY))


def fields_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[n], b[m]) for n, m in zip(a.dtype.names, b.dtype.names))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_nan(a, b):
    """Bit for bit where a NaN's payload is left out (x86 and gfx950 make different default NaNs): the same elements are NaN, every
    other element has the same bits.  For tests/test_scene_edges*.py only; elsewhere results are finite and compared with bits()."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def probe_modes(name, flat=None, wide=True):
    """Every way rsrt_cast_rays can run a query (include/rsrt.h): traversal 0 threaded / 1 stack / 2 typed leaf loops /
    3 flat (what house, default and cube run in production; suzanne's 968 triangles do not qualify) / 4 fixed-order walk
    / 5 wide walk (4-wide nodes, one ray a lane) / 6 cooperative wide walk (the same nodes, a wave's rays as work items on two LDS stacks: what
    suzanne and anything bigger run), x scene read from global memory or from LDS as the production kernel stages
    it for that traversal (bit 4), x cast_ray / cast_ray_bvh (bit 0).  flat: whether the scene qualifies for traversal 3 (default: by name).
    wide: whether it qualifies for traversals 5 and 6."""
    flat = (name != "suzanne") if flat is None else flat
    # 5, 6: the wide walks take the trees of the shipped scenes, not every tree the builder makes: equal centroids give leaves of any
    # length (more than the 8 records a wide node's leaf slot holds), and a tree of one node has no wide tree (tests/edge_trees.py)
    sels = [0, 1, 2, 4] + ([5, 6] if wide else []) + ([3] if flat else [])
    return [(sel << 1) | lds | bvh_only for sel in sels for lds in (0, 16) for bvh_only in (0, 1)]


def rmse_per_channel(a, b, spp):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) / spp
    return np.sqrt((d * d).mean(axis=(0, 1)))


_env_cache = {}


def small_env(w=64, h=32):
    if (w, h) not in _env_cache:
        _env_cache[(w, h)] = R.Environment.synthetic(w, h)
    return _env_cache[(w, h)]


def long_leaf_scene():
    """A foreign BVH over scene `default`: a root and two leaves of ~11 primitives each — more than the 8 the per-type leaf masks and
    the wide nodes hold, so neither the typed leaf loops nor the wide walks take it."""
    base = R.Scene.load_toml(scene_path("default"))
    nodes, prims = base.bvh_nodes, base.primitives
    leaves = [n for n in nodes if n["primitives_len"] > 0]
    leaves.sort(key=lambda n: int(n["primitives_or_second_child_index"]))
    half = len(prims) // 2
    cut = min((int(n["primitives_or_second_child_index"]) for n in leaves), key=lambda i: abs(i - half))
    assert 8 < cut < len(prims) - 8

    def union(sel):
        return (np.min([n["bounds_min"] for n in sel], axis=0), np.max([n["bounds_max"] for n in sel], axis=0))

    new = np.zeros(3, nodes.dtype)
    new[0]["bounds_min"], new[0]["bounds_max"] = union(leaves)
    new[0]["primitives_or_second_child_index"], new[0]["primitives_len"], new[0]["split_axis"] = 2, 0, 0
    a = [n for n in leaves if int(n["primitives_or_second_child_index"]) < cut]
    b = [n for n in leaves if int(n["primitives_or_second_child_index"]) >= cut]
    new[1]["bounds_min"], new[1]["bounds_max"] = union(a)
    new[1]["primitives_or_second_child_index"], new[1]["primitives_len"] = 0, cut
    new[2]["bounds_min"], new[2]["bounds_max"] = union(b)
    new[2]["primitives_or_second_child_index"], new[2]["primitives_len"] = cut, len(prims) - cut
    return R.Scene(base.materials, base.spheres, base.plane_descs, base.vertices, base.normals, base.triangles, base.camera_desc,
                   planes=base.planes, primitives=prims, bvh_nodes=new, bvh_depth=2)


def deck_scene(levels=14):
    """A hand-built scene whose WIDE tree is deeper than the wide walk's eight stack registers, with few nodes: `levels` pairs of
    triangles stacked along z (a deck of cards, seen edge-on by the camera), and a binary BVH that is one long chain — node N_k has
    the small interior node R_k (the two cards of level k) and the chain's next node N_k+1 as children.  Collapsed to four children
    a node, every third chain node becomes a wide node with FOUR interior children (the chain and three R's); a ray along the deck
    hits every box, descends the chain first, and leaves three pending siblings behind at every level: its stack grows by a word a
    level — `levels` // 3 of them.  Boxes nest, leaves hold one record each and share none: the tree qualifies for the wide walk."""
    from rsoderh_raytracing_amd import types as T
    base = R.Scene.load_toml(scene_path("default"))
    verts, tris = [], []
    for k in range(levels):
        z = -float(k)
        s = 1.0 + 0.01 * k  # (slightly different cards: no two records alike)
        for half in range(2):
            v0 = len(verts)
            if half == 0:
                verts += [(-s, -s, z), (s, -s, z), (s, s, z - 0.25)]
            else:
                verts += [(-s, -s, z - 0.5), (s, s, z - 0.5), (-s, s, z - 0.75)]
            tris.append((v0, v0 + 1, v0 + 2))
    vertices = np.zeros(len(verts), T.VEC3)
    vertices["v"] = np.asarray(verts, np.float32)
    normals = np.zeros(1, T.VEC3)
    normals["v"][0] = (0.0, 0.0, 1.0)
    triangles = np.zeros(len(tris), T.TRIANGLE)
    for i, (a, b, c) in enumerate(tris):
        triangles[i] = (a, b, c, 0, 0, 0, i % max(1, len(base.materials)))
    prims = np.zeros(len(tris), T.PRIMITIVE_INFO)
    prims["primitive_type"], prims["index"] = 2, np.arange(len(tris))

    def tri_box(i):
        p = vertices["v"][[tris[i][0], tris[i][1], tris[i][2]]]
        return p.min(axis=0), p.max(axis=0)

    # pre-order with the CHAIN as every node's first child (the wide walk takes a node's children lowest slot first, and only a child
    # that is entered while siblings still wait pushes a word): N_0 N_1 ... N_(levels-2), R_(levels-1), R_(levels-2) ... R_0
    n_chain = levels - 1
    nodes = np.zeros(n_chain + 3 * levels, T.BVH_NODE)
    r_at = {}
    at = n_chain
    for k in range(levels - 1, -1, -1):
        r_at[k] = at
        lo0, hi0 = tri_box(2 * k)
        lo1, hi1 = tri_box(2 * k + 1)
        nodes[at]["bounds_min"], nodes[at]["bounds_max"] = np.minimum(lo0, lo1), np.maximum(hi0, hi1)
        nodes[at]["primitives_or_second_child_index"], nodes[at]["primitives_len"], nodes[at]["split_axis"] = at + 2, 0, 2
        for j, (lo, hi) in enumerate(((lo0, hi0), (lo1, hi1))):
            nodes[at + 1 + j]["bounds_min"], nodes[at + 1 + j]["bounds_max"] = lo, hi
            nodes[at + 1 + j]["primitives_or_second_child_index"], nodes[at + 1 + j]["primitives_len"] = 2 * k + j, 1
        at += 3
    assert at == len(nodes)
    for k in range(n_chain - 1, -1, -1):  # N_k: first child = k + 1 (the chain's next node, or R_(levels-1) behind the last), second = R_k
        a, b = k + 1, r_at[k]
        nodes[k]["primitives_or_second_child_index"], nodes[k]["primitives_len"], nodes[k]["split_axis"] = b, 0, 2
        nodes[k]["bounds_min"] = np.minimum(nodes[a]["bounds_min"], nodes[b]["bounds_min"])
        nodes[k]["bounds_max"] = np.maximum(nodes[a]["bounds_max"], nodes[b]["bounds_max"])
    cam = np.zeros(1, T.CAMERA_DESC)
    cam["pos"], cam["yaw"], cam["pitch"], cam["fov_y"] = (0.15, 0.1, 3.0), 0.03, -0.02, 0.9  # (radians) looking down the deck
    return R.Scene(base.materials, np.zeros(0, T.SPHERE), np.zeros(0, T.PLANE_DESC), vertices, normals, triangles, cam,
                   planes=np.zeros(0, T.PLANE), primitives=prims, bvh_nodes=nodes, bvh_depth=levels + 1)


def fan_scene(quads=256):
    """A hand-built scene whose rays along -z hit EVERY box of the tree: `quads` large squares (two triangles each, one leaf each), all
    facing the camera at distinct z, under a balanced binary BVH over them in z order — so every box spans the whole square and a ray
    seen head-on meets every node.  Its wide tree is short and broad: a batch of rays fans out to every node of a level at once, the case
    that fills the cooperative walk's node queue (tests/coop_lists.py, rt_coop.h).  Boxes nest, records are distinct: it qualifies."""
    from rsoderh_raytracing_amd import types as T
    base = R.Scene.load_toml(scene_path("default"))
    verts, tris = [], []
    for q in range(quads):
        z, s = -0.02 * q, 4.0 + 0.001 * q
        v0 = len(verts)
        verts += [(-s, -s, z), (s, -s, z), (s, s, z), (-s, s, z)]
        tris += [(v0, v0 + 1, v0 + 2), (v0, v0 + 2, v0 + 3)]
    vertices = np.zeros(len(verts), T.VEC3)
    vertices["v"] = np.asarray(verts, np.float32)
    normals = np.zeros(1, T.VEC3)
    normals["v"][0] = (0.0, 0.0, 1.0)
    triangles = np.zeros(len(tris), T.TRIANGLE)
    for i, (a, b, c) in enumerate(tris):
        triangles[i] = (a, b, c, 0, 0, 0, (i // 2) % max(1, len(base.materials)))
    prims = np.zeros(len(tris), T.PRIMITIVE_INFO)
    prims["primitive_type"], prims["index"] = 2, np.arange(len(tris))
    v = vertices["v"]
    lo_q = np.minimum.reduce([v[0::4], v[1::4], v[2::4], v[3::4]])
    hi_q = np.maximum.reduce([v[0::4], v[1::4], v[2::4], v[3::4]])
    nodes = np.zeros(2 * quads - 1, T.BVH_NODE)
    at = [0]

    def build(a, b):  # quads a..b-1, pre-order: the first child follows its parent, the second's index is stored
        i = at[0]
        at[0] += 1
        nodes[i]["bounds_min"], nodes[i]["bounds_max"] = lo_q[a:b].min(axis=0), hi_q[a:b].max(axis=0)
        if b - a == 1:
            nodes[i]["primitives_or_second_child_index"], nodes[i]["primitives_len"] = 2 * a, 2
            return
        m = (a + b) // 2
        build(a, m)
        nodes[i]["primitives_or_second_child_index"], nodes[i]["primitives_len"], nodes[i]["split_axis"] = at[0], 0, 2
        build(m, b)

    build(0, quads)
    assert at[0] == len(nodes)
    cam = np.zeros(1, T.CAMERA_DESC)
    cam["pos"], cam["yaw"], cam["pitch"], cam["fov_y"] = (0.15, 0.1, 3.0), 0.03, -0.02, 0.9
    return R.Scene(base.materials, np.zeros(0, T.SPHERE), np.zeros(0, T.PLANE_DESC), vertices, normals, triangles, cam,
                   planes=np.zeros(0, T.PLANE), primitives=prims, bvh_nodes=nodes, bvh_depth=int(np.ceil(np.log2(quads))) + 1)
