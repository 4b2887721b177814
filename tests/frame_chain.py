"""A frame's whole pass chain as data: the steps of tests/test_frame_chain.py (no GPU: the table reaches every entry point that takes a
stream) and tests/test_frame_chain_gpu.py (the chain against the restatements, and pipelined on caller streams against itself run
synchronously), in the manner of tests/lifecycle_cases.py.  Nearly every other GPU test calls one pass and downloads, which synchronises;
a frame loop enqueues some twenty calls back to back, on streams of its own choosing, and each pass reads what the pass before it left.

A frame (DESIGN.md §1's order), every call enqueued only:
  clear         the accumulator, the AOV buffer, the guide and the fog records (the context's own stream: the clears take none)
  render, aov   samples [begin, begin + S) of the frame's camera and their first hits
  temporal      rsrt_temporal_accumulate_ex with moments                        | variant "plain": rsrt_temporal_accumulate
  denoise       of the temporal colour, variance-guided, with the clamp         | variant "plain": of the temporal colour, fixed levels
  guide, upsample   the side branch: the guide at twice the size, the denoised image upsampled to it
  noise_snapshot, render_more, noise_estimate   S2 more samples and the estimate between the two sums
  fog_render    the fog records at half size                                    | variant "plain": at the frame's size
  fog           rsrt_fog_apply_upsampled of "denoised"                          | variant "plain": rsrt_fog_apply of "denoised"
  dof           of "fog", an explicit focus distance
  motion        of "lens", after the camera of the frame before
  exposure_meter, white_meter   of "motion"
  colour_lut    a CDL that differs from frame to frame
  bloom, local_exposure         of "motion", at an explicit exposure
and the frame's end, downloads(): every download and the four displays of "motion", all synchronous.

Two variants, because two pairs of entry points exclude each other in one context's steady state: a MOMENTS toggle drops the temporal
history, and rsrt_fog_apply wants records of the source's size where rsrt_fog_apply_upsampled is given smaller ones (records of another
size are a new allocation, which waits for everything in flight).  "moments" is the main chain; "plain" swaps the four
steps named above and is run for the two entry points "moments" cannot reach.

Exposure and white point are numbers, as a frame loop takes last frame's; the focus distance is a number too (focus_at downloads)."""
import collections
import ctypes as C
import os
import re

import numpy as np

import hdr_ref
import local_ref
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import state as S, types as T

F = np.float32
NOT_READY_HIP = 600  # hipErrorNotReady

# ---------------------------------------------------------------------------------------------------- settings of every frame
EXPOSURE = 1.7
WHITE = (1.2, 1.0, 0.8)
LOCAL = {"shadows": 1.0, "highlights": 0.25, "key": 0.1, "max_stops": 2.0}
CELL = 16
BLOOM = {"levels": 3, "threshold": 0.5}
BLOOM_INTENSITY = 0.5
LUT_SIZE, LUT_STRENGTH = 17, 0.5
DOF = {"focus_distance": 3.0, "aperture": 0.05, "max_radius": 6}
MOTION = {"shutter": 0.5, "max_radius": 8, "taps": 8}
FOG_LIGHT = (0.4, 0.6, -0.7)
FOG = dict(light_irradiance=(4.0, 3.0, 2.0), ambient=(0.02, 0.03, 0.05), albedo=(0.9, 0.8, 0.7), max_distance=20.0, steps=8, flags=1, density=0.2)
FOG_SAMPLES = 2
NOISE_TILE = (16, 16)
FINISH = {"sharpness": 0.5, "grain": 0.25, "dither": 1.0}
HDR = {"pq10": {"dither": 1.0}, "scrgb16f": {}}
VARIANTS = ("moments", "plain")
# the camera of frame i against the scene's own: (yaw, pitch) in radians.  Frame 0 is the warm-up.
TURNS = [(0.0, 0.0), (0.03, 0.0), (0.06, 0.01), (0.09, -0.01)]


def fog_params():
    import fog_ref
    return dict(FOG, light_dir=fog_ref.unit(FOG_LIGHT))


def cdl(frame):
    """The frame's grade: slope, offset, power, saturation."""
    return (1.1 + 0.05 * frame, 0.01 * frame, 0.9, 1.2)


def cameras(scene, scale=1.0):
    """The rsrt_camera records of the frames: the scene's camera turned by `scale` times TURNS (a frame a fifth as wide wants five times
    the turn for the same velocity in pixels)."""
    out = []
    for yaw, pitch in TURNS:
        desc = np.array(scene.camera_desc).view(T.CAMERA_DESC).reshape(1).copy()
        desc["yaw"] += F(scale * yaw)
        desc["pitch"] += F(scale * pitch)
        out.append(np.array(R.camera_uniform(desc)).view(T.CAMERA).reshape(1).copy())
    return out


Config = collections.namedtuple("Config", "w h samples more variant")
Config.__doc__ = """A chain's sizes: the frame is w x h, the guide twice that; `samples` in the head render, `more` in the second."""


def half(n):
    return (n + 1) // 2


# ---------------------------------------------------------------------------------------------------- the steps
# st.frame: the frame being enqueued — index, begin (its first sample), camera, previous (last frame's camera), cfg, outs (caller
# buffers by step name, or nothing)
Frame = collections.namedtuple("Frame", "index begin camera previous cfg outs")


def new_state(scene_name, cfg, bounces=8):
    sc = R.Scene.load_toml(util.scene_path(scene_name))
    st = R.State.new(sc, R.Environment.synthetic(256, 128), cfg.w, cfg.h)
    st.max_bounces = bounces
    st.frame = None
    return sc, st


def _out(st, name):
    return (st.frame.outs or {}).get(name)


def _clear(st, stream):
    f = st.frame
    st.camera = f.camera.copy()
    st.clear()
    if st._has_aov:
        st.clear_aov()
    if st.guide_width:
        st.clear_guide()
    if st.fog_width:
        st.clear_fog()
    if f.index == 0:
        st.temporal_reset()  # (host only) the warm-up is a first frame whatever ran before


def _render(st, stream):
    f = st.frame
    st.render_range(f.begin, f.cfg.samples, stream=stream)
    st.sample_count = f.cfg.samples


def _aov(st, stream):
    st.render_aov(st.frame.begin, st.frame.cfg.samples, stream=stream)


def _temporal(flags):
    def call(st, stream):
        n = st.frame.cfg.samples
        p = S.TemporalParams(**S.TEMPORAL_DEFAULTS)
        on = C.c_void_p(stream) if stream else None
        if flags is None:
            st._check(st._L.rsrt_temporal_accumulate(st._ctx, S._p(st.camera), n, n, C.byref(p), on), "rsrt_temporal_accumulate")
        else:
            st._check(st._L.rsrt_temporal_accumulate_ex(st._ctx, S._p(st.camera), n, n, C.byref(p), flags, on), "rsrt_temporal_accumulate_ex")
    return call


def _denoise(guided):
    def call(st, stream):
        st.denoise(temporal=True, variance=guided, clamp=guided, download=False, stream=stream, out_ptr=_out(st, "denoise"))
    return call


def _guide(st, stream):
    f = st.frame
    st.render_guide(2 * f.cfg.w, 2 * f.cfg.h, f.begin, f.cfg.samples, stream=stream)


def _upsample(st, stream):
    st.upsample("denoised", download=False, stream=stream, out_ptr=_out(st, "upsample"))


def _render_more(st, stream):
    f = st.frame
    st.render_range(f.begin + f.cfg.samples, f.cfg.more, stream=stream)
    st.sample_count = f.cfg.samples + f.cfg.more


def _fog_render(full):
    def call(st, stream):
        c = st.frame.cfg
        st.render_fog(FOG_SAMPLES, st.frame.begin, stream=stream, size=(c.w, c.h) if full else (half(c.w), half(c.h)), **fog_params())
    return call


def _fog(upsample):
    def call(st, stream):
        st.fog("denoised", upsample=upsample, stream=stream, out_ptr=_out(st, "fog"))
    return call


def _dof(st, stream):
    st.depth_of_field("fog", DOF["focus_distance"], DOF["aperture"], DOF["max_radius"], stream=stream, out_ptr=_out(st, "dof"))


def _motion(st, stream):
    st.motion_blur("lens", st.frame.previous, MOTION["shutter"], MOTION["max_radius"], MOTION["taps"], stream=stream, out_ptr=_out(st, "motion"))


def raw_floats(st, fn, shape):
    out = np.empty(shape, F)
    st._check(getattr(st._L, fn)(st._ctx, S._p(out), out.size), fn)
    return out


def denoised(st):
    return raw_floats(st, "rsrt_denoised_download", (st.height, st.width, 4))


def upsampled(st):
    return raw_floats(st, "rsrt_upsampled_download", (st.guide_height, st.guide_width, 4))


def _result(r, keys):
    """A download's result dict as one float64 array (tuples flattened, in `keys` order)."""
    return np.array([x for k in keys for x in np.ravel(r[k])], np.float64)


EXPOSURE_KEYS = ("exposure", "target", "average_luminance", "metered", "skipped")
WHITE_KEYS = ("white", "target", "illuminant", "eu", "ev", "gated", "counted", "skipped", "estimated")
NOISE_KEYS = ("max_error", "mean_error", "tiles_x", "tiles_y", "tiles_above")
LEVEL_KEYS = ("max_cll", "max_fall", "max_q", "sum_q")


def _noise(st):
    tiles, s = st.noise_download()
    return {"noise_tiles": tiles, "noise_summary": _result(s, NOISE_KEYS)}


def _exposure(st):
    hist, r = st.exposure_download()
    return {"exposure_histogram": hist, "exposure_result": _result(r, EXPOSURE_KEYS)}


def _white(st):
    hist, r = st.white_download()
    return {"white_histogram": hist, "white_result": _result(r, WHITE_KEYS)}


Step = collections.namedtuple("Step", "name entry call downloads variants")
Step.__doc__ = """name; entry: the C entry point the step reaches that takes a stream (None: it takes none); call(st, stream): enqueues only;
downloads(st): {name: array}, what shows the step's result; variants: the chains the step belongs to."""
BOTH = VARIANTS
STEPS = [
    Step("clear", None, _clear, lambda st: {}, BOTH),
    Step("render", "rsrt_render", _render, lambda st: {"accumulator": st.download()}, BOTH),
    Step("aov", "rsrt_aov_render", _aov, lambda st: {"aov": st.download_aov()}, BOTH),
    Step("temporal", "rsrt_temporal_accumulate_ex", _temporal(S.TEMPORAL_MOMENTS),
         lambda st: {"temporal": st.download_temporal(), "moments": st.download_temporal_moments()}, ("moments",)),
    Step("temporal", "rsrt_temporal_accumulate", _temporal(None), lambda st: {"temporal": st.download_temporal()}, ("plain",)),
    Step("denoise", "rsrt_denoise", _denoise(True), lambda st: {"denoised": denoised(st)}, ("moments",)),
    Step("denoise", "rsrt_denoise", _denoise(False), lambda st: {"denoised": denoised(st)}, ("plain",)),
    Step("guide", "rsrt_guide_render", _guide, lambda st: {"guide": st.download_guide()}, BOTH),
    Step("upsample", "rsrt_upsample", _upsample, lambda st: {"upsampled": upsampled(st)}, BOTH),
    Step("noise_snapshot", "rsrt_noise_snapshot", lambda st, stream: st.noise_snapshot(stream=stream), lambda st: {}, BOTH),
    Step("render_more", "rsrt_render", _render_more, lambda st: {"accumulator": st.download()}, BOTH),
    Step("noise_estimate", "rsrt_noise_estimate", lambda st, stream: st.noise_estimate(NOISE_TILE, stream=stream, download=False), _noise, BOTH),
    Step("fog_render", "rsrt_fog_render", _fog_render(False), lambda st: {"fog_records": st.download_fog()}, ("moments",)),
    Step("fog_render", "rsrt_fog_render", _fog_render(True), lambda st: {"fog_records": st.download_fog()}, ("plain",)),
    Step("fog", "rsrt_fog_apply_upsampled", _fog(True), lambda st: {"fog": st.fog_download()}, ("moments",)),
    Step("fog", "rsrt_fog_apply", _fog(False), lambda st: {"fog": st.fog_download()}, ("plain",)),
    Step("dof", "rsrt_dof", _dof, lambda st: {"lens": st.dof_download(), "coc": st.dof_coc()}, BOTH),
    Step("motion", "rsrt_motion_blur", _motion,
         lambda st: {"motion": st.motion_download(), "velocity": st.motion_velocity(), "motion_tiles": st.motion_tiles()}, BOTH),
    Step("exposure_meter", "rsrt_exposure_meter", lambda st, stream: st.exposure_meter("motion", stream=stream), _exposure, BOTH),
    Step("white_meter", "rsrt_white_meter", lambda st, stream: st.white_meter("motion", stream=stream), _white, BOTH),
    Step("colour_lut", "rsrt_colour_lut_build", lambda st, stream: st.colour_lut(*cdl(st.frame.index), size=LUT_SIZE, stream=stream),
         lambda st: {"lut": st.colour_lut_download()}, BOTH),
    Step("bloom", "rsrt_bloom", lambda st, stream: st.bloom("motion", EXPOSURE, stream=stream, **BLOOM), lambda st: {"bloom": st.bloom_download()}, BOTH),
    Step("local_exposure", "rsrt_local_exposure", lambda st, stream: st.local_exposure("motion", CELL, stream=stream),
         lambda st: {"grid": st.local_exposure_download()[0]}, BOTH),
]


def steps(variant):
    return [s for s in STEPS if variant in s.variants]


def entry_points():
    """The entry points the table reaches, over both variants."""
    return {s.entry for s in STEPS if s.entry}


def variant_of(entry):
    """The chain that reaches `entry`: "moments" where it can."""
    return next(v for v in VARIANTS if any(s.entry == entry for s in steps(v)))


def header_stream_entry_points():
    """The prototypes of include/rsrt.h with a `void *hip_stream` parameter."""
    text = open(os.path.join(util.ROOT, "include", "rsrt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1) for m in re.finditer(r"rsrt_status\s+(rsrt_\w+)\s*\(([^;{]*)\)\s*;", text) if re.search(r"void\s*\*\s*hip_stream\b", m.group(2))}


# ---------------------------------------------------------------------------------------------------- the frame's end
def displays(st, source, seed):
    """The four displays of `source` with everything on: the grid and the bloom image the context holds, the LUT, the white point."""
    chain = dict(white=WHITE, bloom_intensity=BLOOM_INTENSITY, **LOCAL)
    out = {"finished": st.display_finished_srgb8(source, EXPOSURE, lut_strength=LUT_STRENGTH, seed=seed, **FINISH, **chain),
           "colour": st.display_colour_srgb8(source, EXPOSURE, lut_strength=LUT_STRENGTH, **chain)}
    for enc, kw in HDR.items():
        img, lv = st.display_hdr(source, EXPOSURE, encoding=enc, seed=seed, levels=True, **kw, **chain)
        out["hdr_" + enc] = img.view(np.uint16) if enc == "scrgb16f" else img
        out["hdr_" + enc + "_levels"] = _result(lv, LEVEL_KEYS)
    return out


def downloads(st, variant="moments"):
    """Everything a frame leaves, as arrays by name: every step's downloads, then the displays of "motion".  All synchronous."""
    out = {}
    for s in steps(variant):
        out.update(s.downloads(st))
    out.update(displays(st, "motion", st.frame.index if st.frame else 0))
    return out


def same(a, b):
    """Bit for bit (float32: where a NaN's payload is left out, util.same_bits_or_nan)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return util.same_bits_or_nan(a, b) if a.dtype == F else a.tobytes() == b.tobytes()


def differing(got, want):
    """The names whose arrays differ."""
    return sorted(set(got) ^ set(want)) + [k for k in got if k in want and not same(got[k], want[k])]


# ---------------------------------------------------------------------------------------------------- running a frame
def frame_of(cams, index, cfg, outs=None):
    """Frame `index` along the camera path: fresh sample indices, and the camera of the frame before (the warm-up: its own)."""
    return Frame(index, 1000 * index, cams[index], cams[max(index - 1, 0)], cfg, outs)


def enqueue(st, frame, stream_of=lambda i, step: None, after=None):
    """Enqueues the frame's steps, step i on stream_of(i, step) (None: the context's own); after(step), if given, runs behind each
    call (the synchronous run synchronises there).  Returns the stream of the last call."""
    st.frame = frame
    last = None
    for i, s in enumerate(steps(frame.cfg.variant)):
        last = stream_of(i, s) if s.entry else None
        s.call(st, last)
        if after:
            after(s)
    return last


class Streams:
    """Caller streams from the HIP runtime the library uses: `blocking` made with hipStreamCreate, one more with
    hipStreamCreateWithFlags(hipStreamNonBlocking) — the null stream does not order that one.  close() destroys them."""

    def __init__(self, blocking=3):
        from test_denoise_gpu import hip_runtime_path
        S.lib()
        self.hip = C.CDLL(hip_runtime_path())
        self.handles = []
        try:
            for _ in range(blocking):
                self._make(lambda p: self.hip.hipStreamCreate(p))
            self.non_blocking = self._make(lambda p: self.hip.hipStreamCreateWithFlags(p, C.c_uint(1)))  # hipStreamNonBlocking
        except Exception:
            self.close()
            raise
        self.blocking = self.handles[:blocking]

    def _make(self, create):
        s = C.c_void_p()
        assert create(C.byref(s)) == 0 and s.value
        self.handles.append(s.value)
        return s.value

    def query(self, stream):
        """hipStreamQuery: 0 when everything enqueued on `stream` is done, NOT_READY_HIP while it is not."""
        return self.hip.hipStreamQuery(C.c_void_p(stream))

    def close(self):
        for s in self.handles:
            assert self.hip.hipStreamDestroy(C.c_void_p(s)) == 0
        self.handles = []


# ---------------------------------------------------------------------------------------------------- the HDR levels' frames
LEVELS_H, LEVELS_W = 136, 512  # 17 x 16 = 272 workgroups of 8 x 32: the smallest count past 256 that leaves the last trip partial
LEVELS_TILE_H, LEVELS_TILE_W = 8, 32
LEVELS_BRIGHT = dict(paper_white=10000.0, peak=10000.0)


def workgroup_of(y, x, w=LEVELS_W):
    """The display workgroup (row-major over the grid of 32 x 8 tiles) pixel (y, x) of a frame w wide belongs to."""
    return (y // LEVELS_TILE_H) * ((w + LEVELS_TILE_W - 1) // LEVELS_TILE_W) + x // LEVELS_TILE_W


def levels_bright():
    """Sums that put every pixel at the peak whatever the exposure: 2^70 in every channel (the sanitiser caps it at 2^64, the shoulder
    brings it to the peak exactly)."""
    s = np.full((LEVELS_H, LEVELS_W, 4), F(2.0 ** 70), F)
    s[..., 3] = 1
    return s


def levels_lognormal():
    """local_ref.synthetic's lognormal frame without its special pixels and with its bright dots capped at 8, so that at the default
    settings every pixel stays under the peak — and one pixel of the last workgroup, 271, at 3e38: the frame's only pixel at the peak.
    Returns (sums, (y, x) of that pixel)."""
    s, _ = local_ref.synthetic(LEVELS_H, LEVELS_W, seed=2000 * LEVELS_H + LEVELS_W, specials=False)
    s[..., :3] = np.minimum(s[..., :3], F(8.0))
    y, x = LEVELS_H - 3, LEVELS_W - 7
    s[y, x, :3] = F(3e38)
    return s, (y, x)


def level_q_of(sums, total, exposure, **hdr):
    """hdr_ref's q of every pixel, [h, w] uint32."""
    kw = dict(hdr_ref.DEFAULTS, **hdr)
    return hdr_ref.level_q(hdr_ref.nits_of(hdr_ref.linear(sums, total, exposure), kw["paper_white"], kw["peak"], kw["knee"], kw["encoding"]))
