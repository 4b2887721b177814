"""The flat kernel's SHADE and GEN at the places where their work is shared or skipped, on small frames, every one the checker's bit for
bit with the checker's ray counts.  SHADE forms G1(wo) once for the NEE evaluation and the evaluation of the sampled direction, and an
evaluation forms its D once (rt_wavepool.h, rt_device.h ONE_D): both lobes, the debug-colour exits of the BSDF sample, paths that end
with a shadow ray out, picks that cast no shadow ray (no NEE evaluation: the shared term serves the sample alone), materials that always
/ never take the diffuse lobe.  GEN's fused trace reads only the leaves of the cull groups its batch hits (rt_device.h trace_flat,
`coherent`): leaf sets of every size modulo four, the empty one included, worked out here from the box tests on each batch's rays."""
import functools
import os

import numpy as np
import pytest

import denoise_ref as D
import edge_envs as EE
import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import types as T

pytestmark = pytest.mark.gpu

F = np.float32


@functools.lru_cache(maxsize=None)
def golden_env():
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "env_64x32.npz"))
    return R.Environment(g["rgba"], g["alias"].view(T.ALIAS_ENTRY).reshape(-1))


def check(sc, env, w, h, spp, mb, cam=None):
    """One frame through the flat kernel against the checker: the same bits, the same rays.  Returns the checker's counters."""
    cam = sc.camera_uniform() if cam is None else cam
    ref, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(env), np.asarray(cam).view(oracle.CAMERA), w, h, 0, spp, mb)
    st = R.State.new(sc, env, w, h, camera=cam)
    try:
        st.max_bounces = mb
        st.render_range(0, spp)
        img, s = st.download(), st.stats()
    finally:
        st.close()
    same = util.bits(img) == util.bits(ref)
    assert same.all(), int((~same).any(axis=2).sum())
    assert (s["paths"], s["ext_rays"], s["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"])
    assert s["traversal_steps"] == 0  # the flat kernel ran (the tree walks count their steps)
    return ost


# ---------------------------------------------------------------------------------------------------- SHADE
@pytest.mark.parametrize("mb", [1, 2, 8])
@pytest.mark.parametrize("name", ["default", "house", "spheres_only"])
def test_shade_keeps_the_bits(name, mb):
    """default, house (mirror and rough metal: the specular lobe and its wi.z <= 0 exit) and spheres_only at 1, 2 and 8 bounces: at the
    bounce limit every path ends in SHADE with its shadow ray still out (FINISH adds the parked term)."""
    ost = check(E.plain(name), golden_env(), 48, 32, 4, mb)
    assert ost["shadow_rays"] > 0


def test_picks_that_cast_no_shadow_ray():
    """`spike`: black but for one texel — the bilinear radiance around it is not zero, the pdf of every other texel is: picks with
    es.pdf == 0 (no shadow ray, no NEE term) next to picks with one."""
    env = EE.case("spike").env
    assert (env.alias["pmf"] == 0).sum() >= 10
    ost = check(E.plain("default"), env, 48, 32, 4, 6)
    assert 0 < ost["shadow_rays"]


def lobe_scene(colour):
    """default with every material a metal of one grey: f0 = colour, so the specular lobe is picked with probability saturate(luminance)"""
    base = E.plain("default")
    m = base.materials.copy()
    m["color"], m["metallic"], m["roughness"], m["emission"] = colour, 1.0, 0.5, 0.0
    f0 = (F(1.0) - F(1.0)) * F(0.04) + F(1.0) * F(colour)
    ps = min(max(F(0.2126) * f0 + F(0.7152) * f0 + F(0.0722) * f0, F(0.0)), F(1.0))  # rsrt_api.hip make_material_record
    return E.rebuilt(base, materials=m), F(1.0) - ps


@pytest.mark.parametrize("colour,diff_prob", [(2.0, 0.0), (0.0, 1.0)])
def test_materials_of_one_lobe(colour, diff_prob):
    """diff_prob 0: every BSDF sample is a GGX half vector (s < 0 never holds); diff_prob 1: every one a cosine sample."""
    sc, dp = lobe_scene(colour)
    assert dp == F(diff_prob)
    check(sc, golden_env(), 48, 32, 4, 6)


# ---------------------------------------------------------------------------------------------------- GEN's fused trace
def cull_groups(sc):
    """The scene image's two-level cull (rt_scene_image.h fill_cull_groups; test_scene_image.py compares the two) of a scene the flat loop takes: (always, [(box min, box max, leaf mask)]) — the leaves above
    the cull depth, and the interior nodes two levels below the root with the leaves under each; leaves numbered in node order."""
    nodes = sc.bvh_nodes
    leaf_index = {i: k for k, i in enumerate(i for i in range(len(nodes)) if nodes[i]["primitives_len"] > 0)}
    always, groups, stack = 0, [], [(0, 0)]
    while stack:
        i, d = stack.pop()
        if nodes[i]["primitives_len"] != 0:
            always |= 1 << leaf_index[i]
            continue
        if d == 2 and len(groups) < 8:
            m, sub = 0, [i]
            while sub:
                j = sub.pop()
                if nodes[j]["primitives_len"] != 0:
                    m |= 1 << leaf_index[j]
                else:
                    sub += [j + 1, int(nodes[j]["primitives_or_second_child_index"])]
            groups.append((np.asarray(nodes[i]["bounds_min"], F), np.asarray(nodes[i]["bounds_max"], F), m))
            continue
        stack += [(i + 1, d + 1), (int(nodes[i]["primitives_or_second_child_index"]), d + 1)]
    return always, groups, len(leaf_index)


def box_hit(lo, hi, o, d):
    """the slab test of trace_flat / cast_ray_bvh, one f32 operation at a time (1 / d is finite for these rays)"""
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        a, b = (lo - o) * inv, (hi - o) * inv
    t0 = np.maximum(np.minimum(a, b).max(axis=1), F(0.0))
    t1 = np.maximum(a, b).min(axis=1)
    return ~(t0 > t1)


def active_popcounts(sc, cam, w, h):
    """Set bits of `active` for every 16 x 4 patch of the first sample: the batch of camera rays a wave's first GEN trip on a tile traces
    together (16 x 16 tiles, 64 consecutive pixels of a tile a trip)."""
    always, groups, n_leaves = cull_groups(sc)
    out = []
    for ty in range(0, h, 4):
        for tx in range(0, w, 16):
            py, px = np.mgrid[ty:min(ty + 4, h), tx:min(tx + 16, w)]
            o, d = D.camera_rays(np.asarray(cam).view(T.CAMERA)[0], w, h, px.reshape(-1), py.reshape(-1), 0)
            assert np.isfinite(F(1.0) / d).all()
            active = always
            for lo, hi, m in groups:
                if box_hit(lo, hi, o, d).any():
                    active |= m
            out.append(bin(active & ((1 << n_leaves) - 1)).count("1"))
    return out, n_leaves


@pytest.mark.parametrize("name,want", [("cube", {2, 5}), ("default", {2, 4, 6, 8})])
def test_leaf_groups_on_small_leaf_sets(name, want):
    """cube: 5 leaves (2 above the cull depth, one group of 3); default: 8 (2, and groups of 2 and 4) — batches of fewer than four leaves,
    of four, and of four and one or two more."""
    sc = E.plain(name)
    counts, n_leaves = active_popcounts(sc, sc.camera_uniform(), 50, 35)
    assert n_leaves == max(want) and set(counts) == want, (n_leaves, sorted(set(counts)))
    check(sc, golden_env(), 50, 35, 4, 6)


# house: 20 leaves — the ground's leaf above the cull depth (always read), and groups of 3, 8 and 8 leaves; so a batch reads 1, 4, 9, 12, 17
# or 20 boxes.  From high above, looking up: no group is hit (1 leaf); from above the roofs, down at the ground: every kind of batch, 17
# (a multiple of four and one more) among them; level, from the scene's own place: 4, 12, 20 (multiples of four only).
HOUSE_CAMERAS = {"sky": ((0.0, 40.0, 3.0), 1.2, {1}), "ground": ((0.0, 6.0, 12.0), -0.6, {1, 4, 17, 20}), "level": ((0.0, 1.0, 3.0), 0.0, {4, 12, 20})}


@pytest.mark.parametrize("view", ["sky", "ground", "level"])
def test_leaf_groups_on_house_from_three_cameras(view):
    """50 x 35: edge tiles in both directions.  What each camera's batches hold is worked out first, from the box tests on each patch's rays."""
    pos, pitch, want = HOUSE_CAMERAS[view]
    sc = E.plain("house")
    cam = E.camera(pos, 0.0, pitch, 1.2)
    always, groups, n_leaves = cull_groups(sc)
    assert (bin(always).count("1"), sorted(bin(m).count("1") for _, _, m in groups), n_leaves) == (1, [3, 8, 8], 20)
    counts, _ = active_popcounts(sc, cam, 50, 35)
    assert set(counts) == want, sorted(set(counts))
    check(sc, golden_env(), 50, 35, 4, 8, cam=cam)


def test_the_house_cameras_give_short_full_and_mixed_leaf_sets():
    """(the three sets above, taken together: 1 - 3 leaves, multiples of four, and five or more that are none)"""
    seen = set().union(*(want for _, _, want in HOUSE_CAMERAS.values()))
    assert any(1 <= c <= 3 for c in seen) and any(c >= 5 and c % 4 == 0 for c in seen) and any(c >= 5 and c % 4 != 0 for c in seen)


@functools.lru_cache(maxsize=None)
def clusters_scene():
    """64 small spheres in eight clusters: 17 leaves, every one of them under one of four cull groups (no leaf above the cull depth), so
    a batch whose rays miss every group reads no box at all."""
    base = E.plain("default")
    rng = np.random.default_rng(3)
    sph = np.zeros(64, T.SPHERE)
    centres = [(x, y, z) for x in (-4, 4) for y in (1, 5) for z in (-4, -12)]
    for k in range(64):
        sph[k]["pos"] = np.array(centres[k // 8]) + rng.uniform(-1, 1, 3)
        sph[k]["radius"], sph[k]["material_id"] = 0.3, k % len(base.materials)
    return E.rebuilt(base, spheres=sph, plane_descs=np.zeros(0, T.PLANE_DESC), triangles=np.zeros(0, T.TRIANGLE))


def test_leaf_groups_when_no_leaf_is_always_read():
    sc = clusters_scene()
    cam = E.camera((0.0, 3.0, 4.0), 0.4, 0.3, 1.0)
    always, groups, n_leaves = cull_groups(sc)
    assert always == 0 and len(groups) == 4 and n_leaves == 17
    counts, _ = active_popcounts(sc, cam, 50, 35)
    assert set(counts) == {0, 4, 5, 8}, sorted(set(counts))  # nothing to read; four; four and one; eight
    check(sc, golden_env(), 50, 35, 4, 6, cam=cam)
