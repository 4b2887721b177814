"""Hand-edited BVHs over scene `default`: trees a host may upload but no builder makes, each breaking one thing the faster walks
rely on.  test_gpu_parity.py takes them through the render kernels, tests/edge_fog.py through the fog march.  Every constructor
returns the edited scene; base() is the scene they start from."""
import numpy as np

import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import types as T


def base():
    return R.Scene.load_toml(util.scene_path("default"))


def shrunken_box_scene():
    """An interior node's box shrunk to half its size about its middle, so that its children stick out: the boxes do not nest, and a
    ray that misses the shrunken box skips the subtree although it would hit a child."""
    base_ = base()
    nodes = base_.bvh_nodes.copy()
    interior = [i for i in range(1, len(nodes)) if nodes[i]["primitives_len"] == 0]
    i = interior[0]
    mid = (nodes[i]["bounds_min"] + nodes[i]["bounds_max"]) * np.float32(0.5)
    nodes[i]["bounds_min"] = mid + (nodes[i]["bounds_min"] - mid) * np.float32(0.5)
    nodes[i]["bounds_max"] = mid + (nodes[i]["bounds_max"] - mid) * np.float32(0.5)
    return R.Scene(base_.materials, base_.spheres, base_.plane_descs, base_.vertices, base_.normals, base_.triangles, base_.camera_desc,
                   planes=base_.planes, primitives=base_.primitives, bvh_nodes=nodes, bvh_depth=base_.bvh_depth)


def shared_record_scene():
    """A leaf that also holds its left neighbour's last record (boxes untouched: they still nest, only the sharing disqualifies)."""
    base_ = base()
    nodes = base_.bvh_nodes.copy()
    leaves = [i for i in range(len(nodes)) if nodes[i]["primitives_len"] > 1]
    b_ = next(i for i in leaves[1:] if nodes[i]["primitives_or_second_child_index"] > 0)
    nodes[b_]["primitives_or_second_child_index"] -= 1
    nodes[b_]["primitives_len"] += 1
    return R.Scene(base_.materials, base_.spheres, base_.plane_descs, base_.vertices, base_.normals, base_.triangles, base_.camera_desc,
                   planes=base_.planes, primitives=base_.primitives, bvh_nodes=nodes, bvh_depth=base_.bvh_depth)


def twin_sphere_scene():
    """A sphere exists twice, with two materials, and its copies sit in DIFFERENT leaves: the copy is appended to the last leaf, whose
    box and whose ancestors' boxes grow to hold it."""
    base_ = base()
    nodes, prims = base_.bvh_nodes.copy(), base_.primitives
    k = next(i for i, p in enumerate(prims) if int(p["primitive_type"]) == 0)  # a sphere record ...
    src = int(prims[k]["index"])
    last = max((i for i in range(len(nodes)) if nodes[i]["primitives_len"] > 0), key=lambda i: int(nodes[i]["primitives_or_second_child_index"]))
    assert not (int(nodes[last]["primitives_or_second_child_index"]) <= k < int(nodes[last]["primitives_or_second_child_index"]) + int(nodes[last]["primitives_len"]))  # ... of another leaf
    spheres = np.zeros(len(base_.spheres) + 1, T.SPHERE)  # (np.concatenate would drop the struct's padding)
    spheres[:-1] = base_.spheres
    spheres[-1] = base_.spheres[src]
    spheres[-1]["material_id"] = (int(spheres[src]["material_id"]) + 1) % len(base_.materials)
    new_prims = np.concatenate([prims, np.array([(0, len(spheres) - 1)], prims.dtype)])
    lo = np.asarray(spheres[-1]["pos"], np.float32) - np.float32(spheres[-1]["radius"])
    hi = np.asarray(spheres[-1]["pos"], np.float32) + np.float32(spheres[-1]["radius"])
    nodes[last]["primitives_len"] += 1
    parent = {}
    for i in range(len(nodes)):
        if nodes[i]["primitives_len"] == 0:
            parent[i + 1] = i
            parent[int(nodes[i]["primitives_or_second_child_index"])] = i
    i = last
    while True:
        nodes[i]["bounds_min"] = np.minimum(nodes[i]["bounds_min"], lo)
        nodes[i]["bounds_max"] = np.maximum(nodes[i]["bounds_max"], hi)
        if i == 0:
            break
        i = parent[i]
    return R.Scene(base_.materials, spheres, base_.plane_descs, base_.vertices, base_.normals, base_.triangles, base_.camera_desc,
                   planes=base_.planes, primitives=new_prims, bvh_nodes=nodes, bvh_depth=base_.bvh_depth)


HIDDEN_FIRST, HIDDEN_COUNT = 10, 70  # hidden_spheres_scene: spheres 10 .. 69 are in no leaf


def hidden_sphere_positions():
    """Where hidden_spheres_scene puts spheres 10 .. 69: a rising row behind the scene."""
    return [(-6.0 + 0.2 * i, 2.5 + 0.03 * i, -4.0) for i in range(HIDDEN_FIRST, HIDDEN_COUNT)]


def hidden_spheres_scene(positions=None):
    """70 spheres, of which the BVH (and so `primitives`) knows only the first 10: cast_ray's brute-force loop still visits all 70
    after a BVH miss, and nothing else ever sees spheres 10 .. 69 (at `positions`, default hidden_sphere_positions())."""
    base_ = base()
    spheres = np.zeros(HIDDEN_COUNT, T.SPHERE)
    spheres[:HIDDEN_FIRST] = base_.spheres
    for i, pos in zip(range(HIDDEN_FIRST, HIDDEN_COUNT), hidden_sphere_positions() if positions is None else positions):
        spheres[i]["pos"] = pos
        spheres[i]["radius"] = 0.12
        spheres[i]["material_id"] = i % len(base_.materials)
    return R.Scene(base_.materials, spheres, base_.plane_descs, base_.vertices, base_.normals, base_.triangles, base_.camera_desc,
                   planes=base_.planes, primitives=base_.primitives, bvh_nodes=base_.bvh_nodes, bvh_depth=base_.bvh_depth)
