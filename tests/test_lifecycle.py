"""The cases of tests/lifecycle_cases.py reach what they aim at — shown without a GPU, from the library's host arithmetic, the host
tree builder and the checker's images.  test_lifecycle_gpu.py then holds one living context to them."""
import numpy as np
import pytest

import coop_lists as M
import lifecycle_cases as L
import test_wide_tree
import util
from rsoderh_raytracing_amd import partition


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return L.scene("big", tmp_path_factory.mktemp("big"))


# ---------------------------------------------------------------------------------------------------- tiles
@pytest.mark.parametrize("frame", L.FRAMES, ids=["%dx%d" % f for f in L.FRAMES])
def test_library_partition_agrees_with_the_formula_at_every_new_tile_shape(frame):
    w, h = frame
    for tw, th in L.tiles_of(frame):
        for world, skew in L.WORLDS.items():
            assert partition.skew(world) == skew
            owner = partition.tile_owner_map(w, h, world, tw, th)
            for rank in range(world):
                assert np.array_equal(partition.owned_mask(w, h, rank, world, tw, th), owner == rank), (frame, tw, th, world, rank)
                assert np.array_equal(partition.tile_slots(w, h, rank, world, tw, th), partition.tile_slots_numpy(w, h, rank, world, tw, th))


def test_tile_cases_hold_a_padding_slot_a_small_frame_and_an_idle_rank():
    padding = small = idle = 0
    for frame in L.FRAMES:
        w, h = frame
        for tw, th, world, rank in L.tile_cases(frame):
            slots = partition.tile_slots_numpy(w, h, rank, world, tw, th)
            padding += bool((slots[:, 0] < 0).any() and (slots[:, 0] >= 0).any())  # beside tiles of its own
            small += w < tw and h < th
            idle += not (partition.tile_owner_map(w, h, world, tw, th) == rank).any()
    assert padding and small and idle, (padding, small, idle)
    assert all(tw * th % 64 == 0 and tw * th <= 4096 for tw, th in L.TILES) and max(tw * th for tw, th in L.TILES) == 4096
    assert {(tw != th) for tw, th in L.TILES} == {True, False}  # square and not
    for tw, th in L.REJECTED_TILES:  # the library's own arithmetic refuses them too
        with pytest.raises(ValueError):
            partition.owned_mask(64, 64, 0, 1, tw, th)


# ---------------------------------------------------------------------------------------------------- the checker's images
def a_picture(img):
    rgb = np.asarray(img)[..., :3]
    return bool(np.isfinite(img).all() and len(np.unique(rgb)) > 1)


def test_consecutive_scenes_of_the_chain_give_different_images(big):
    refs = [L.step_reference(s)[0] for s in L.CHAIN]
    assert all(a_picture(r) for r in refs)
    for a, b, s in zip(refs, refs[1:], L.CHAIN[1:]):
        assert not np.array_equal(a, b), s.scene
    assert L.CHAIN[0].scene == L.CHAIN[-1].scene and L.CHAIN[0].env_index != L.CHAIN[-1].env_index
    kinds = [s.klass for s in L.CHAIN]
    assert kinds == ["flat", "coop", "generic", "coop", "coop", "flat", "flat", "flat"]  # every boundary, both ways
    assert {(a, b) for a, b in zip(kinds, kinds[1:])} >= {("flat", "coop"), ("coop", "generic"), ("generic", "coop"), ("coop", "flat")}


def test_environments_give_different_images_and_samples_do_not_repeat():
    for name in ("default", "suzanne"):
        imgs = [L.reference(name, e, L.W, L.H, 0, 3)[0] for e in ("small", "odd", "tiny")]
        assert all(a_picture(i) for i in imgs)
        assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2]) and not np.array_equal(imgs[0], imgs[2])
    for en in L.SIZE_ENVS:
        for w, h in L.SIZES:
            r1, r2, r4 = (L.reference("default", en, w, h, 0, n)[0] for n in (1, 2, 4))
            assert a_picture(r1) and a_picture(r2) and a_picture(r4), (en, w, h)
            assert not np.array_equal(r2[..., :3], r4[..., :3] / np.float32(2)), (en, w, h)  # a buffer that kept [0, 2) would show
            assert not np.array_equal(r2, r1 + r1)


def test_tile_and_two_context_images_are_pictures():
    for name in L.TILE_SCENES:
        for w, h in L.FRAMES:
            a, b = (L.reference(name, "small", w, h, *r)[0] for r in L.RANGES)
            assert a_picture(a) and a_picture(b) and not np.array_equal(a * np.float32(L.RANGES[1][1]), b)
    assert a_picture(L.reference("default", "small", 64, 40, 0, 6)[0])
    s6, s7 = L.reference("suzanne", "small", 48, 32, 0, 6), L.reference("suzanne", "small", 48, 32, 0, 7)
    assert a_picture(s6[0]) and a_picture(s7[0]) and L.counters(s7[1]) > L.counters(s6[1])
    big_frame, st = L.reference("default", "small", 1024, 512, 0, 24, L.MB, True)
    assert a_picture(big_frame) and st["paths"] == 1024 * 512 * 24
    assert 1024 * 512 * 9 > 4 << 20 >= 1024 * 512  # nine samples a call are an ordinary job, one is a small one (rsrt_api.hip kSmallPaths)


# ---------------------------------------------------------------------------------------------------- scene classes
def flat_eligible(sc):
    """The counts rsrt_upload_scene asks of the flat loop (the boxes of these trees nest, no record is shared)."""
    leaves = int((sc.bvh_nodes["primitives_len"] > 0).sum())
    return len(sc.primitives) <= 64 and len(sc.spheres) <= 64 and len(sc.planes) <= 64 and leaves <= 32


def test_long_leaf_scene_has_long_leaves_and_needs_the_bounce_limit_to_leave_the_flat_loop():
    sc = L.scene("long_leaf")
    assert int(sc.bvh_nodes["primitives_len"].max()) > 8
    assert test_wide_tree.wide_tree(sc) is None  # no wide tree: neither wide walk
    assert flat_eligible(sc)
    step = next(s for s in L.CHAIN if s.scene == "long_leaf")
    assert step.max_bounces == L.header_define("RT_FLAT_MAX_BOUNCES", "rt_wavepool.h") + 1
    with_limit, plain = L.step_reference(step), L.reference("long_leaf", L.CHAIN_ENVS[step.env_index], L.W, L.H, 0, L.SPP, 64)
    assert np.array_equal(with_limit[0], plain[0]) and L.counters(with_limit[1]) == L.counters(plain[1])  # (paths end long before)


def test_deck_scene_is_deeper_than_the_register_stack_and_no_flat_scene():
    sc = L.scene("deck")
    wn, _ = test_wide_tree.wide_tree(sc)
    registers = L.header_define("RT_WSTACK", "rt_device.h")
    assert registers == 8 and M.Tree(wn).depth > registers + 1  # rsrt_upload_scene's wide_deep
    assert not flat_eligible(sc)
    assert flat_eligible(util.deck_scene()) and M.Tree(test_wide_tree.wide_tree(util.deck_scene())[0]).depth <= registers + 1  # (why not the default deck)
    too_deep = util.deck_scene(L.TOO_DEEP_LEVELS)
    assert (too_deep.bvh_depth + 1) * 256 * 4 > 128 * 1024 and len(too_deep.bvh_nodes) < 1 << 25


def test_big_scene_has_more_wide_nodes_than_the_staged_prefix(big):
    wn, _ = test_wide_tree.wide_tree(big)
    room = L.coop_room_float4s()
    assert room == 1280  # 160 KiB - 16 waves x 4 x (12 x 128 + 320 + 320 + 64) bytes, in float4
    assert len(wn) > room // 8
    n = len(big.bvh_nodes)
    assert (2 * n + (8 * n + 3) // 4) * 16 > 40 * 1024  # nodes + escape links: not staged for the tree walks (lifecycle_cases.BIG_LDS_REFUSED)
    step = next(s for s in L.CHAIN if s.scene == "big")
    assert not set(L.BIG_LDS_REFUSED) & set(L.probe_modes(step)) and set(L.BIG_LDS_REFUSED) | set(L.probe_modes(step)) == set(util.probe_modes("suzanne"))
    suz, _ = test_wide_tree.wide_tree(L.scene("suzanne"))
    assert 0 < len(suz) and not flat_eligible(L.scene("suzanne")) and not flat_eligible(big)
    for name in ("default", "cube", "spheres_only"):
        assert flat_eligible(L.scene(name)), name


def test_probe_rays_and_mode_lists():
    for step in L.CHAIN[:4]:
        o, d, want = L.probe(step.scene)
        assert 24 <= len(o) <= 96 and want[0][:, 0].any(), step.scene
    assert len(L.probe_modes(L.CHAIN[0])) == 28 and set(L.probe_modes(L.CHAIN[0])) == set(util.probe_modes("default"))
    assert set(L.probe_modes(L.CHAIN[1])) == set(util.probe_modes("suzanne"))
    bad = L.out_of_range_copy(L.scene("suzanne"))
    assert int(bad.triangles["vertex_0"][0]) == len(bad.vertices) and int(L.scene("suzanne").triangles["vertex_0"][0]) < len(bad.vertices)
