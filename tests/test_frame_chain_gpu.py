"""A frame's whole pass chain on the GPU (tests/frame_chain.py has the chain as data).

Part 1, the chain against the restatements.  house at 67 x 37 — one past a tile both ways for every pass's tile (16 x 16 render, noise and
motion tiles, 32 x 8 display tiles, cells of 16) — guide and upsampled image 134 x 74, fog records 34 x 19, 2 + 2 samples, two frames
(the warm-up camera, then a turn of 0.15 rad, some 3 pixels: the temporal pass reprojects and the shutter has a previous camera).
The chain runs synchronously and after every step the step's download is compared, bit for bit, with the numpy restatement the pass's
own suite uses, applied to the downloaded inputs of that step.  What is new is the inputs: the variance-guided filter of a temporal frame feeds the upsampler and the fog
rebuild, the lens reads that fog image, the shutter the lens image, and every meter, the bloom pyramid, the grid and the four displays
read "motion".  The path tracer's own outputs (accumulator, AOV buffer, guide) are inputs here, not re-checked.
Consumer x source pairs compared here (* held by another suite before: test_motion_gpu.py, test_fog_upsample_gpu.py, test_colour_gpu.py):
  on "motion":  exposure_meter*, white_meter, bloom*, local_exposure*, display_finished_srgb8, display_hdr (both encodings, with levels),
                display_colour_srgb8 with grid, bloom image and LUT
  on "fog":     exposure_meter*, white_meter, bloom, local_exposure, display_finished_srgb8, display_hdr, display_colour_srgb8
  on "lens":    exposure_meter, white_meter, bloom, local_exposure, display_finished_srgb8, display_hdr, display_colour_srgb8*
  and the passes: rsrt_upsample and rsrt_fog_apply_upsampled of a variance-guided "denoised", rsrt_dof of that fog image, rsrt_motion_blur
  of that lens image with the AOV buffer as its records.
The refusals of a source a pass may not take are pinned word for word, and leave every result as it was.

Part 2, pipelined equals synchronous.  house at 352 x 200 (275 display workgroups: display_hdr's levels take the second trip of their
reduction too), 8 bounces.  The head of every frame is a render of S = 512 samples: everything behind it in the chain waits for it, so
a call that did not wait would read the frame before — another camera's picture.  The second render of a frame has 128 samples: 73216 slots
x 128 is above the 4 Mi paths under which rsrt_render pipelines a call over its lanes with the small kernel form, a path a synchronous
run never takes.  That the load is real is asserted, not assumed: right behind the last enqueue of a frame hipStreamQuery on the stream
of the last call must say hipErrorNotReady — the head render was still running and no call of the warm chain synchronised the host.
Where the last call is on the context's own stream, whose handle the library does not give out (the one-foreign-stream cases), the probe
is one more rsrt_exposure_meter of "motion" on a caller stream of its own, which rebuilds the histogram the frame already has.
Every frame's end calls rsrt_get_stats, which takes the pending render events back: rsrt_render synchronises when 32 passes are pending
(it bounds its event pool; INTEGRATION.md §4 says so), which a frame loop that never asks for statistics meets every sixteenth frame of
this chain.  No other entry point was found to synchronise in the warm chain, and none to miss it.

S as used: 512 (never doubled).  Seen on an MI355X over the 42 pipelined frames of one run of this file (host clock around the frame's
enqueues; kernel_ms of rsrt_get_stats for the frame's two renders, 640 samples): enqueueing took 0.73 to 1.84 ms, the renders' kernels
10.4 to 23.0 ms (22.8 ms for most), and hipStreamQuery said hipErrorNotReady every time.  test_frames_pipelined_on_caller_streams
and the cases behind it print the three figures of every frame (pytest -s).

That the tests have teeth was shown once with a build of the library whose begin_work does not wait (the hipStreamWaitEvent line taken
out; not committed): both tests of TestPipelinedEqualsSynchronous and all 38 cases of TestOneForeignStreamAtATime failed, the first
with temporal, moments, denoised, upsampled, the noise estimate and everything behind them differing from the synchronous run.  In
that build the library's own lane streams go unordered too, so every case also lost the noise estimate and, through the probe, the
exposure histogram; each case's own image (lens for rsrt_dof, grid for rsrt_local_exposure, ...) was among the differences where the
entry point reads anything the chain wrote (rsrt_colour_lut_build reads nothing)."""
import ctypes as C
import time

import numpy as np
import pytest

import bloom_ref
import colour_ref
import dof_ref
import exposure_ref
import finish_ref
import fog_ref
import fog_upsample_ref
import frame_chain as FC
import hdr_ref
import local_ref
import motion_ref
import noise_ref
import temporal_ref
import upsample_ref
import util
import variance_ref
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import state as S
from test_denoise_gpu import DeviceArray

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
F = np.float32


def refused(call, status, text):
    """The call is refused with `status` and the library's error text is `text`, word for word (as tests/test_image_buffers_gpu.py pins its)."""
    with pytest.raises(R.RsrtError) as e:
        call()
    assert (e.value.status, str(e.value).split("): ", 1)[1]) == (status, text)


# ---------------------------------------------------------------------------------------------------- part 1
SMALL = FC.Config(67, 37, 2, 2, "moments")
SMALL_TURN = 5.0  # 0.15 rad a frame: about 3 pixels at 67 wide, as 0.03 rad is at 352


def expected_displays(img, grid, b, lut, seed):
    """The restatements of frame_chain.displays over the downloaded grid, bloom image and LUT."""
    gain = local_ref.gains(img, 1, FC.EXPOSURE, grid, FC.CELL, **FC.LOCAL)
    out = {"finished": finish_ref.display(img, 1, FC.EXPOSURE, FC.WHITE, lut, FC.LUT_STRENGTH, gain, FC.BLOOM_INTENSITY, b, seed=seed, **FC.FINISH),
           "colour": colour_ref.display(img, 1, FC.EXPOSURE, FC.WHITE, lut, FC.LUT_STRENGTH, gain, FC.BLOOM_INTENSITY, b)}
    for enc, kw in FC.HDR.items():
        words, lv = hdr_ref.display(img, 1, FC.EXPOSURE, FC.WHITE, gain, FC.BLOOM_INTENSITY, b, encoding=hdr_ref.ENCODINGS[enc], seed=seed, **kw)
        out["hdr_" + enc] = words
        out["hdr_" + enc + "_levels"] = FC._result(lv, FC.LEVEL_KEYS)
    return out


def expected_consumers(img):
    """The restatements of both meters, the bloom image and the grid of `img`, a colour image (total 1)."""
    eh, wh = exposure_ref.histogram(img, 1), colour_ref.histogram(img, 1)
    return {"exposure_histogram": eh, "exposure_result": FC._result(exposure_ref.from_histogram(eh), FC.EXPOSURE_KEYS),
            "white_histogram": wh, "white_result": FC._result(colour_ref.from_histogram(wh), FC.WHITE_KEYS),
            "bloom": bloom_ref.bloom(img, 1, FC.EXPOSURE, FC.BLOOM["levels"], FC.BLOOM["threshold"]), "grid": local_ref.grid_of(img, 1, FC.CELL)}


def colour_only(want, got):
    """A restatement that returns [h, w, 3] against a download with an alpha of 1."""
    assert got.shape[:2] == want.shape[:2] and (got[..., 3] == 1).all()
    return np.concatenate([np.asarray(want, F)[..., :3], np.ones(want.shape[:2] + (1,), F)], axis=-1)


class Restated:
    """The chain's restatement, frame after frame: expected(step name, have) gives what the step's downloads must be, from `have`, the
    downloads of the steps before it in the frame; the temporal history is the restatement's own, carried from frame to frame."""

    def __init__(self, scene, cfg):
        self.osc, self.cfg, self.seq = util.oracle_scene(scene), cfg, variance_ref.MomentSequence()

    def expected(self, step, have, frame):
        c, n = self.cfg, self.cfg.samples
        cam, prev = temporal_ref.Camera.from_record(frame.camera), temporal_ref.Camera.from_record(frame.previous)
        if step == "temporal":
            col, mom, _ = self.seq.frame(have["head"], have["aov"], n, n, cam)
            return {"temporal": col, "moments": mom}
        if step == "denoise":
            want = variance_ref.denoise(have["temporal"], have["aov"], 1, n, 5, variance_ref.SIGMA_L, 0.5, 0.3, True, True, True, have["moments"])
            return {"denoised": colour_only(want, have["denoised"])}
        if step == "upsample":
            return {"upsampled": colour_only(upsample_ref.upsample(have["denoised"], have["aov"], have["guide"], 1, n, n), have["upsampled"])}
        if step == "noise_estimate":
            tiles, s = noise_ref.estimate(have["head"], n, have["accumulator"], n + c.more, FC.NOISE_TILE)
            return {"noise_tiles": tiles, "noise_summary": FC._result(s, FC.NOISE_KEYS)}
        if step == "fog_render":
            rec, lit = fog_ref.records(self.osc, frame.camera[0], FC.half(c.w), FC.half(c.h), frame.begin, FC.FOG_SAMPLES, fog_ref.params(**FC.fog_params()))
            assert 0.02 < 1.0 - lit.mean() < 0.98  # lit and shaded march points
            return {"fog_records": rec}
        if step == "fog":
            k = fog_ref.prepare(fog_ref.params(**FC.fog_params()))
            return {"fog": fog_upsample_ref.rebuild(fog_ref.source_colour(have["denoised"], 1), have["fog_records"], FC.FOG_SAMPLES, have["aov"], n, k)[0]}
        if step == "dof":
            lens, r = dof_ref.dof(have["fog"], 1, have["aov"], cam, FC.DOF["focus_distance"], FC.DOF["aperture"], FC.DOF["max_radius"])
            return {"lens": lens, "coc": r}
        if step == "motion":
            img, uvl, tiles = motion_ref.motion(have["lens"], 1, have["aov"], cam, prev, FC.MOTION["shutter"], FC.MOTION["max_radius"], FC.MOTION["taps"])
            return {"motion": img, "velocity": uvl, "motion_tiles": tiles}
        if step in ("exposure_meter", "white_meter", "bloom", "local_exposure"):
            want = expected_consumers(have["motion"])
            return {k: want[k] for k in {"exposure_meter": ("exposure_histogram", "exposure_result"), "white_meter": ("white_histogram", "white_result"),
                                         "bloom": ("bloom",), "local_exposure": ("grid",)}[step]}
        if step == "colour_lut":
            return {"lut": colour_ref.bake(FC.LUT_SIZE, *FC.cdl(frame.index))}
        if step == "displays":
            return expected_displays(have["motion"], have["grid"], have["bloom"], have["lut"], frame.index)
        return {}  # the path tracer's own outputs and the snapshot: inputs


@pytest.fixture(scope="class")
def small():
    """The chain run synchronously at 67 x 37 for two frames: (the state, left at the second frame's end; the scene; the cameras; per frame
    the list of (step name, that step's downloads, taken right behind the step), the displays as a last step)."""
    sc, st = FC.new_state("house", SMALL)
    try:
        cams = FC.cameras(sc, SMALL_TURN)
        log = []
        for i in range(2):
            rows = []
            FC.enqueue(st, FC.frame_of(cams, i, SMALL), after=lambda s: (st.synchronize(), rows.append((s.name, s.downloads(st)))))
            rows.append(("displays", FC.displays(st, "motion", i)))
            log.append(rows)
        yield st, sc, cams, log
    finally:
        st.close()


class TestTheChainAgainstTheRestatements:
    def test_every_step_equals_its_restatement_on_the_downloaded_inputs_of_that_step(self, small):
        st, sc, cams, log = small
        ref = Restated(sc, SMALL)
        compared = set()
        for i, rows in enumerate(log):
            frame, have = FC.frame_of(cams, i, SMALL), {}
            for name, got in rows:
                have.update(got)
                if name == "render":
                    have["head"] = got["accumulator"]
                want = ref.expected(name, have, frame)
                for k, w in want.items():
                    assert FC.same(got[k], np.asarray(w, got[k].dtype)), (i, name, k)
                    compared.add(k)
            assert have["fog"].shape == (37, 67, 4) and have["upsampled"].shape == (74, 134, 4) and have["fog_records"].shape == (19, 34, 4)
            if i:  # the turn gave the passes something to do
                assert (have["velocity"][..., 2] >= 2.0).any() and not FC.same(have["motion"], have["lens"]) and not FC.same(have["lens"], have["fog"])
                assert have["moments"][..., 2].max() >= 2  # reprojected history
        everything = set().union(*(got for rows in log for _, got in rows))
        assert everything - compared == {"accumulator", "aov", "guide"}, everything - compared
        assert not FC.differing(dict(log[0][-1][1]), dict(log[0][-1][1])) and FC.differing(dict(log[0][-1][1]), dict(log[1][-1][1]))  # (another picture a frame)

    @pytest.mark.parametrize("source", ["fog", "lens"])
    def test_the_consumers_on_the_later_sources(self, small, source):
        st, sc, cams, log = small
        have = {}
        for _, got in log[1]:
            have.update(got)
        img = have[source]
        st.frame = FC.frame_of(cams, 1, SMALL)
        st.exposure_meter(source)
        st.white_meter(source)
        st.bloom(source, FC.EXPOSURE, **FC.BLOOM)
        st.local_exposure(source, FC.CELL)
        got = {}
        for step in FC.steps("moments"):
            if step.name in ("exposure_meter", "white_meter", "bloom", "local_exposure"):
                got.update(step.downloads(st))
        assert not FC.differing(got, {k: np.asarray(w, got[k].dtype) for k, w in expected_consumers(img).items()})
        shown = FC.displays(st, source, 1)
        want = expected_displays(img, got["grid"], got["bloom"], have["lut"], 1)
        assert not FC.differing(shown, {k: np.asarray(w, shown[k].dtype) for k, w in want.items()})
        assert FC.differing(shown, dict(log[1][-1][1]))  # not the motion image's
        st.exposure_meter("motion")  # (what the frame left)
        st.white_meter("motion")
        st.bloom("motion", FC.EXPOSURE, **FC.BLOOM)
        st.local_exposure("motion", FC.CELL)

    def test_the_refusals_of_a_source_a_pass_may_not_take(self, small):
        st, sc, cams, log = small
        st.frame = FC.frame_of(cams, 1, SMALL)
        before = FC.downloads(st)
        L, cam = st._L, S._p(st.camera)
        dp, mp = S.DofParams(3.0, 0.05, 6, 0), S.MotionParams(0.5, 8, 8, 0)
        fp = S.FogParams.of(**FC.fog_params())
        dof = lambda s: st._check(L.rsrt_dof(st._ctx, s, 1, cam, C.byref(dp), None, None), "rsrt_dof")  # noqa: E731
        motion = lambda s: st._check(L.rsrt_motion_blur(st._ctx, s, 1, cam, cam, C.byref(mp), None, None), "rsrt_motion_blur")  # noqa: E731
        fog = lambda s: st._check(L.rsrt_fog_apply(st._ctx, s, 1, 1, None, None), "rsrt_fog_apply")  # noqa: E731
        fog_up = lambda s: st._check(L.rsrt_fog_apply_upsampled(st._ctx, s, 1, 1, 1, C.byref(fp), None, None), "rsrt_fog_apply_upsampled")  # noqa: E731
        # the lens goes before the shutter, the fog before both; no pass reads its own image
        refused(lambda: dof(4), INVALID, "dof: the lens image is not a source of its own pass")
        refused(lambda: dof(5), INVALID, "dof: unknown source 5")
        refused(lambda: motion(5), INVALID, "motion_blur: the motion image is not a source of its own pass")
        for name, call in (("fog_apply", fog), ("fog_apply_upsampled", fog_up)):
            refused(lambda: call(4), INVALID, "%s: the fog goes before the lens and the shutter (source 4)" % name)
            refused(lambda: call(5), INVALID, "%s: the fog goes before the lens and the shutter (source 5)" % name)
            refused(lambda: call(6), INVALID, "%s: the fog image is not a source of its own pass" % name)
            refused(lambda: call(7), INVALID, "%s: unknown source 7" % name)
        # one past the last source
        refused(lambda: dof(7), INVALID, "dof: unknown source 7")
        refused(lambda: motion(7), INVALID, "motion_blur: unknown source 7")
        refused(lambda: st.exposure_meter(7), INVALID, "exposure_meter: unknown source 7")
        refused(lambda: st.white_meter(7), INVALID, "white_meter: unknown source 7")
        refused(lambda: st.bloom(7, FC.EXPOSURE), INVALID, "bloom: unknown source 7")
        refused(lambda: st.local_exposure(7, FC.CELL), INVALID, "local_exposure: unknown source 7")
        assert not FC.differing(FC.downloads(st), before)  # no refused call wrote anything or dropped an image


# ---------------------------------------------------------------------------------------------------- part 2
W, H, SAMPLES, MORE = 352, 200, 512, 128
CANARY = 64  # floats behind a caller's buffer


def big(variant):
    return FC.Config(W, H, SAMPLES, MORE, variant)


def frame_end(st, variant):
    """downloads() and the statistics of the frame's renders (rsrt_get_stats also takes the pending render events back)."""
    d = FC.downloads(st, variant)
    return d, st.stats()


def run_synchronously(variant, last):
    """Frames 0 (the warm-up) .. last with st.synchronize() behind every call: {frame: downloads}."""
    cfg = big(variant)
    sc, st = FC.new_state("house", cfg)
    try:
        cams = FC.cameras(sc)
        out = {}
        for i in range(last + 1):
            FC.enqueue(st, FC.frame_of(cams, i, cfg), after=lambda s: st.synchronize())
            out[i], _ = frame_end(st, variant)
        return out
    finally:
        st.close()


_sync = {}


def synchronous(variant):
    """The synchronous run's downloads, computed once per variant (the "plain" chain is only ever asked for frame 1)."""
    if variant not in _sync:
        _sync[variant] = run_synchronously(variant, 3 if variant == "moments" else 1)
    return _sync[variant]


def warm_up(st, cams, cfg, outs=None):
    """One frame synchronously, so that every buffer exists: a new allocation waits for everything in flight by design."""
    FC.enqueue(st, FC.frame_of(cams, 0, cfg, outs), after=lambda s: st.synchronize())
    return frame_end(st, cfg.variant)[0]


def pipelined(st, cams, cfg, index, streams, stream_of, probe=None, outs=None):
    """Frame `index` enqueued with no host synchronisation; the evidence is taken before anything is downloaded.  Returns the frame's
    downloads."""
    t0 = time.perf_counter()
    last = FC.enqueue(st, FC.frame_of(cams, index, cfg, outs), stream_of)
    if probe is not None:
        st.exposure_meter("motion", stream=probe)
        last = probe
    t1 = time.perf_counter()
    status = streams.query(last)
    d, stats = frame_end(st, cfg.variant)
    print("frame %d (%s): enqueued in %.3f ms; the two renders' kernels took %.3f ms; hipStreamQuery behind the last enqueue: %d"
          % (index, cfg.variant, 1e3 * (t1 - t0), stats["kernel_ms"], status))
    assert last is not None and status == FC.NOT_READY_HIP, "the chain had finished, or a call waited for it, before the frame's last call was enqueued"
    return d


class TestPipelinedEqualsSynchronous:
    def test_frames_pipelined_on_caller_streams(self):
        """Frames 1 to 3, consecutive calls never on the same stream: three blocking caller streams, a non-blocking one and the
        context's own, round robin."""
        want = synchronous("moments")
        assert FC.differing(want[0], want[1]) and FC.differing(want[1], want[2]) and FC.differing(want[2], want[3])
        cfg = big("moments")
        sc, st = FC.new_state("house", cfg)
        streams = None
        try:
            streams = FC.Streams()
            slots = streams.blocking + [streams.non_blocking, None]
            n = len(FC.steps("moments"))
            assert slots[(n - 1) % len(slots)] is not None  # the frame's last call is on a stream that can be asked
            cams = FC.cameras(sc)
            assert not FC.differing(warm_up(st, cams, cfg), want[0])
            for i in (1, 2, 3):
                got = pipelined(st, cams, cfg, i, streams, lambda k, step: slots[k % len(slots)])
                assert not FC.differing(got, want[i]), (i, FC.differing(got, want[i]))
        finally:
            st.close()
            if streams:
                streams.close()

    def test_a_callers_output_buffers_in_a_pipelined_frame(self):
        """denoise, upsample, fog, depth_of_field and motion_blur into DeviceArrays of the caller's, each pass reading the one before it
        from there: the synchronous run's bits, and the words behind every buffer untouched."""
        want = synchronous("moments")
        cfg = big("moments")
        sc, st = FC.new_state("house", cfg)
        streams = None
        try:
            streams = FC.Streams()
            slots = streams.blocking + [streams.non_blocking, None]
            canary = np.uint32(0xdeadbeef).view(F)
            sizes = {"denoise": (H, W), "upsample": (2 * H, 2 * W), "fog": (H, W), "dof": (H, W), "motion": (H, W)}
            mine = {k: DeviceArray(np.full(h * w * 4 + CANARY, canary, F)) for k, (h, w) in sizes.items()}
            outs = {k: a.data_ptr() for k, a in mine.items()}
            cams = FC.cameras(sc)
            assert not FC.differing(warm_up(st, cams, cfg, outs), want[0])
            got = pipelined(st, cams, cfg, 1, streams, lambda k, step: slots[k % len(slots)], outs=outs)
            st.synchronize()
            assert not FC.differing(got, want[1]), FC.differing(got, want[1])
            for k, name in (("denoise", "denoised"), ("upsample", "upsampled"), ("fog", "fog"), ("dof", "lens"), ("motion", "motion")):
                (h, w), a = sizes[k], mine[k].numpy()
                assert FC.same(a[:h * w * 4].reshape(h, w, 4), want[1][name]), k
                assert (util.bits(a[h * w * 4:]) == 0xdeadbeef).all(), k
        finally:
            st.close()
            if streams:
                streams.close()


class Pipe:
    """One context for the one-foreign-stream cases of a variant, with its streams; asking for the other variant closes it first."""

    def __init__(self):
        self.variant = self.st = self.streams = self.cams = None

    def get(self, variant):
        if variant != self.variant:
            self.close()
            sc, self.st = FC.new_state("house", big(variant))
            self.variant, self.cams, self.streams = variant, FC.cameras(sc), FC.Streams(blocking=2)
        return self.st, self.cams, self.streams

    def close(self):
        if self.st is not None:
            self.st.close()
        if self.streams is not None:
            self.streams.close()
        self.variant = self.st = self.streams = None


@pytest.fixture(scope="class")
def pipe():
    p = Pipe()
    try:
        yield p
    finally:
        p.close()


ENTRY_POINTS = sorted(FC.entry_points(), key=lambda e: (FC.variant_of(e) != "moments", e))  # ("moments" first: one context after the other)


class TestOneForeignStreamAtATime:
    @pytest.mark.parametrize("kind", ["blocking", "non_blocking"])
    @pytest.mark.parametrize("entry", ENTRY_POINTS)
    def test_one_entry_point_on_a_caller_stream(self, pipe, entry, kind):
        """Frame 1 pipelined, every call on the context's own stream but `entry`'s.  The warm-up before it has another camera: a call
        that did not wait for the chain would run long before the head render's resolve and read the warm-up frame's data."""
        variant = FC.variant_of(entry)
        want = synchronous(variant)
        st, cams, streams = pipe.get(variant)
        cfg = big(variant)
        foreign = streams.blocking[0] if kind == "blocking" else streams.non_blocking
        assert any(s.entry == entry for s in FC.steps(variant))
        assert not FC.differing(warm_up(st, cams, cfg), want[0])
        got = pipelined(st, cams, cfg, 1, streams, lambda k, step: foreign if step.entry == entry else None, probe=streams.blocking[1])
        assert not FC.differing(got, want[1]), (entry, kind, FC.differing(got, want[1]))
