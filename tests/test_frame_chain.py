"""tests/frame_chain.py without a GPU: the step table reaches every entry point of include/rsrt.h that takes a stream, the frames'
cameras differ, and the two frames of the HDR levels test (tests/test_hdr_gpu.py) reach the edges they are for — a sum past 2^32, and a
maximum that only the last of 272 workgroups holds."""
import numpy as np

import frame_chain as FC
import hdr_ref
import rsoderh_raytracing_amd as R
import util


def test_the_step_table_reaches_every_entry_point_that_takes_a_stream():
    header = FC.header_stream_entry_points()
    assert "rsrt_comm_reduce" in header and "rsrt_render" in header and len(header) == 20
    assert FC.entry_points() == header - {"rsrt_comm_reduce"}  # (the exchange has tests of its own: tests/test_multi_gpu.py)
    for variant in FC.VARIANTS:
        names = [s.name for s in FC.steps(variant)]
        assert len(names) == len(set(names)) and names[0] == "clear" and names[1] == "render"  # one chain, the load at its head
    reached = {v: {s.entry for s in FC.steps(v)} for v in FC.VARIANTS}
    assert len(reached["moments"]) == 18  # (rsrt_render twice, the clears none)
    assert reached["plain"] - reached["moments"] == {"rsrt_temporal_accumulate", "rsrt_fog_apply"}
    assert all(FC.variant_of(e) == ("plain" if e in ("rsrt_temporal_accumulate", "rsrt_fog_apply") else "moments") for e in FC.entry_points())


def test_the_frames_cameras_differ_by_a_turn():
    cams = FC.cameras(R.Scene.load_toml(util.scene_path("house")))
    assert len(cams) == 4
    for i, a in enumerate(cams):
        for b in cams[i + 1:]:
            assert np.array_equal(a["pos"], b["pos"]) and a["fov_y"] == b["fov_y"]          # a turn, not a move
            assert not np.array_equal(a["rot_transform"], b["rot_transform"])
    for a, b in zip(cams, cams[1:]):  # about 0.03 rad a frame: a few pixels at 352 wide, under the motion pass's radius of 8
        cos = float(np.dot(a["rot_transform"][0][2, :3].astype(np.float64), b["rot_transform"][0][2, :3].astype(np.float64)))
        assert 0.02 < np.arccos(min(cos, 1.0)) < 0.05


def test_the_bright_levels_frame_sums_past_32_bits():
    sums = FC.levels_bright()
    assert sums.shape == (136, 512, 4) and FC.workgroup_of(135, 511) == 271
    for enc in (hdr_ref.PQ10, hdr_ref.SCRGB16F):
        q = FC.level_q_of(sums, 3, 1.0, encoding=enc, **FC.LEVELS_BRIGHT).astype(np.uint64)
        assert (q == 640000).all() and int(q.sum()) == 69632 * 640000 > 2 ** 32
        _, lv = hdr_ref.display(sums, 3, 1.0, encoding=enc, **FC.LEVELS_BRIGHT)
        assert lv["sum_q"] == 69632 * 640000 and lv["max_cll"] == lv["max_fall"] == 10000.0
        # every workgroup's own sum still fits 32 bits, as the kernel's first stage assumes
        assert 256 * 640000 < 2 ** 32


def test_the_lognormal_levels_frames_brightest_pixel_lies_in_the_last_workgroup():
    sums, (y, x) = FC.levels_lognormal()
    assert FC.workgroup_of(y, x) == 271 == 17 * 16 - 1
    for enc in (hdr_ref.PQ10, hdr_ref.SCRGB16F):
        q = FC.level_q_of(sums, 1, 1.0, encoding=enc)
        assert q[y, x] == 64000 and int((q == q.max()).sum()) == 1 and np.unravel_index(int(q.argmax()), q.shape) == (y, x)
        rest = q.copy()
        rest[y, x] = 0
        assert rest.max() < 64000 - 64  # far brighter than every other: more than a cd/m^2
        # the pairs differ from workgroup to workgroup: 272 sums, (nearly) all distinct
        wg = q.astype(np.uint64).reshape(17, 8, 16, 32).sum(axis=(1, 3)).reshape(-1)
        assert wg.size == 272 and len(set(wg.tolist())) >= 270 and wg.max() < 2 ** 32
