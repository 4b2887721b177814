"""`State` — the host render state of the reference (src/state.rs:29-834) over librsrt.so.

    State.new(scene, environments)   State::new   (state.rs:60-649): uploads the eight scene
                                     buffers and the environment maps + alias tables
    state.resize(w, h)               State::resize (state.rs:651-666): accumulator follows the size
    state.update(camera=..)          State::update (state.rs:722-758): per-frame uniforms
    state.render()                   State::render (state.rs:760-833): one progressive frame —
                                     scene-hash reset, sample_count += 1, one dispatch
    state.render_samples(n)          the batched form the C-ABI adds: n samples in one call

No CPU fallback: constructing a State without librsrt.so / a gfx950 GPU raises RsrtError.
"""
import ctypes as C

import numpy as np

from . import _build, types as T

FLAG_REFERENCE_TRAVERSAL = 1  # shadow query runs to the end too (literal shader.wgsl:1249)
# rsrt_get_walk_counters, in order (rt_coop.h CoopCount)
WALK_COUNTERS = ("node_trips", "leaf_trips", "spills", "refills", "lifo_trips", "narrow_trips", "overflows", "peak")
FLAG_PRUNE = 2                # opt-in t-pruning; NOT exactly result-preserving (include/rsrt.h)

_SYMBOLS = ["rsrt_context_create", "rsrt_context_destroy", "rsrt_last_error", "rsrt_upload_scene",
            "rsrt_upload_environment", "rsrt_set_partition", "rsrt_accumulator_resize", "rsrt_accumulator_bind",
            "rsrt_accumulator_clear", "rsrt_accumulator_download", "rsrt_resolve_mean_f16", "rsrt_debug_view_f16", "rsrt_render",
            "rsrt_synchronize", "rsrt_get_stats", "rsrt_cast_rays", "rsrt_describe", "rsrt_get_debug_counters", "rsrt_get_region_counters", "rsrt_get_walk_counters", "rsrt_display_srgb8",
            "rsrt_selftest_numerics", "rsrt_selftest_sincos", "rsrt_build_id", "rsrt_wide_tree_build", "rsrt_scene_image_build", "rsrt_build_bvh_device",
            "rsrt_partition_owner", "rsrt_partition_mask", "rsrt_partition_tiles", "rsrt_comm_available", "rsrt_comm_unique_id", "rsrt_comm_init", "rsrt_comm_reduce", "rsrt_comm_set_mode", "rsrt_comm_destroy",
            "rsrt_multi_create", "rsrt_multi_destroy", "rsrt_multi_last_error", "rsrt_multi_size", "rsrt_multi_context",
            "rsrt_multi_upload_scene", "rsrt_multi_upload_environment", "rsrt_multi_resize", "rsrt_multi_clear", "rsrt_multi_render",
            "rsrt_multi_synchronize", "rsrt_multi_download", "rsrt_multi_display_srgb8", "rsrt_multi_get_stats", "rsrt_multi_uses_rccl",
            "rsrt_aov_render", "rsrt_aov_bind", "rsrt_aov_clear", "rsrt_aov_download", "rsrt_denoise", "rsrt_denoised_download",
            "rsrt_denoised_display_srgb8", "rsrt_temporal_accumulate", "rsrt_temporal_reset", "rsrt_temporal_download",
            "rsrt_temporal_accumulate_ex", "rsrt_temporal_moments_download",
            "rsrt_guide_render", "rsrt_guide_bind", "rsrt_guide_clear", "rsrt_guide_download", "rsrt_upsample", "rsrt_upsampled_download",
            "rsrt_upsampled_display_srgb8", "rsrt_noise_snapshot", "rsrt_noise_estimate", "rsrt_noise_download", "rsrt_noise_reset",
            "rsrt_exposure_meter", "rsrt_exposure_download", "rsrt_exposure_reset", "rsrt_display_exposed_srgb8",
            "rsrt_bloom", "rsrt_bloom_download", "rsrt_bloom_reset", "rsrt_display_bloomed_srgb8",
            "rsrt_local_exposure", "rsrt_local_exposure_download", "rsrt_local_exposure_reset", "rsrt_local_gain_download",
            "rsrt_display_local_srgb8",
            "rsrt_dof", "rsrt_dof_download", "rsrt_dof_coc_download", "rsrt_dof_depth_at", "rsrt_dof_reset",
            "rsrt_motion_blur", "rsrt_motion_download", "rsrt_motion_velocity_download", "rsrt_motion_tiles_download", "rsrt_motion_reset",
            "rsrt_fog_render", "rsrt_fog_bind", "rsrt_fog_clear", "rsrt_fog_download", "rsrt_fog_apply", "rsrt_fog_image_download", "rsrt_fog_reset",
            "rsrt_fog_apply_upsampled",
            "rsrt_environment_sky", "rsrt_environment_download",
            "rsrt_white_meter", "rsrt_white_download", "rsrt_white_reset", "rsrt_colour_lut_build", "rsrt_colour_lut_upload",
            "rsrt_colour_lut_download", "rsrt_colour_lut_reset", "rsrt_display_colour_srgb8", "rsrt_display_finished_srgb8",
            "rsrt_display_hdr", "rsrt_display_video",
            "rsrt_display_jpeg", "rsrt_display_jpeg_coefficients", "rsrt_jpeg_encode_coefficients"]


class RsrtError(RuntimeError):
    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status  # the rsrt_status of the failing call, where there is one


DENOISE_DEMODULATE = 1  # rsrt_denoise_params.flags: filter colour / albedo, then multiply the albedo back
# rsrt_denoise_params defaults (include/rsrt.h)
DENOISE_DEFAULTS = {"iterations": 5, "sigma_color": 2.0, "sigma_normal": 0.5, "sigma_depth": 0.3, "demodulate": True}
AOV_FLOATS = 8  # per pixel: albedo sum xyz, hits, normal sum xyz, distance sum


DENOISE_TEMPORAL = 2  # rsrt_denoise_params.flags: filter the temporal pass's colour instead of the accumulator's mean
# rsrt_temporal_params defaults (include/rsrt_temporal.h)
TEMPORAL_DEFAULTS = {"max_history": 32, "depth_tolerance": 0.05, "normal_tolerance": 0.9}
TEMPORAL_MOMENTS = 1  # rsrt_temporal_accumulate_ex flags: keep the luminance moments too
DENOISE_VARIANCE = 4  # rsrt_denoise_params.flags: variance-guided levels (include/rsrt_variance.h)
DENOISE_CLAMP = 8     # ... and the firefly clamp of the filter's input
VARIANCE_SIGMA_L = 4.0  # sigma_color's default under DENOISE_VARIANCE (RSRT_SV_SIGMA_L: SVGF's sigma_l)


# rsrt_upsample_params.flags and defaults (include/rsrt.h "guided upsampling")
UPSAMPLE_DEMODULATE = 1  # upsample colour / albedo, then multiply the guide's albedo back
UPSAMPLE_DENOISED = 2    # the low colour is the last denoise() output
UPSAMPLE_TEMPORAL = 4    # ... the last render_temporal frame's colour
UPSAMPLE_DEFAULTS = {"sigma_normal": 0.5, "sigma_depth": 0.3, "demodulate": True}


class UpsampleParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


# rsrt_noise_params defaults (include/rsrt.h "noise estimate")
NOISE_DEFAULTS = {"tile": (16, 16), "threshold": 0.0}


class NoiseParams(C.Structure):
    _fields_ = [("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("threshold", C.c_float), ("flags", C.c_uint32)]


class NoiseSummary(C.Structure):
    _fields_ = [("max_error", C.c_float), ("mean_error", C.c_float), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32),
                ("tiles_above", C.c_uint32), ("_pad", C.c_uint32)]


# rsrt_exposure_params defaults (include/rsrt.h "auto-exposure", include/rsrt_exposure.h) and the source names
EXPOSURE_DEFAULTS = {"low_permille": 100, "high_permille": 950, "key": 0.18, "min_exposure": 2.0 ** -16, "max_exposure": 2.0 ** 16,
                     "blend": 1.0, "previous_exposure": 0.0}
EXPOSURE_SOURCES = {"mean": 0, "denoised": 1, "temporal": 2, "upsampled": 3}
EXPOSURE_WORDS = 257
NOT_READY = 4  # RSRT_ERR_NOT_READY


class ExposureParams(C.Structure):
    _fields_ = [("low_permille", C.c_uint32), ("high_permille", C.c_uint32), ("key", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("blend", C.c_float), ("previous_exposure", C.c_float), ("flags", C.c_uint32)]


class ExposureResult(C.Structure):
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("average_luminance", C.c_float), ("metered", C.c_uint32),
                ("skipped", C.c_uint32), ("_pad", C.c_uint32)]


# rsrt_bloom_params.flags, its defaults and the default intensity (include/rsrt.h "bloom", include/rsrt_bloom.h)
BLOOM_KARIS = 1  # the first downsample weighs its groups by 1 / (1 + luminance)
BLOOM_MAX_LEVELS = 8
BLOOM_DEFAULTS = {"levels": 6, "flags": BLOOM_KARIS, "threshold": 1.0, "intensity": 0.1}


class BloomParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_float), ("_pad", C.c_float)]


# the local exposure pass's cells and defaults (include/rsrt.h "local exposure", include/rsrt_local.h)
LOCAL_CELLS = (8, 16, 32, 64)
LOCAL_GZ = 32
LOCAL_DEFAULTS = {"cell": 32, "shadows": 0.5, "highlights": 0.5, "key": 0.18, "max_stops": 4.0}


class LocalParams(C.Structure):
    _fields_ = [("shadows", C.c_float), ("highlights", C.c_float), ("key", C.c_float), ("max_stops", C.c_float), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


# the depth-of-field pass (include/rsrt.h "depth of field", include/rsrt_dof.h): the sources a pass can read — the four images and the
# lens image the pass leaves — its defaults and its parameters
IMAGE_SOURCES = dict(EXPOSURE_SOURCES, lens=4)
DOF_MAX_RADIUS = 16
DOF_DEFAULTS = {"focus_distance": 1.0, "aperture": 0.01, "max_radius": 8, "flags": 0}


class DofParams(C.Structure):
    _fields_ = [("focus_distance", C.c_float), ("aperture", C.c_float), ("max_radius", C.c_uint32), ("flags", C.c_uint32)]


# camera motion blur (include/rsrt.h "camera motion blur", include/rsrt_motion.h): the sources the passes after it can read — the five
# images and the motion image the pass leaves — its tile, its defaults and its parameters
DISPLAY_SOURCES = dict(IMAGE_SOURCES, motion=5)
MOTION_TILE = 16
MOTION_MAX_RADIUS = 16
MOTION_DEFAULTS = {"shutter": 0.5, "max_radius": 16, "taps": 16, "flags": 0}


class MotionParams(C.Structure):
    _fields_ = [("shutter", C.c_float), ("max_radius", C.c_uint32), ("taps", C.c_uint32), ("flags", C.c_uint32)]


def camera_earlier(camera, yaw=0.0, dolly=0.0):
    """The rsrt_camera record of the camera one frame before `camera` (a record like State.camera), for motion_blur(previous=...):
    turned back by `yaw` radians about the world's up axis (+y) and moved back by `dolly` scene units along camera's forward axis."""
    prev = np.array(camera).view(T.CAMERA).reshape(1).copy()
    axes = prev["rot_transform"][0][:, :3].astype(np.float64)  # row j: the camera's axis j (right, up, backward) in the world
    c, s = np.cos(-yaw), np.sin(-yaw)
    if yaw:
        prev["rot_transform"][0][:, :3] = (np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ axes.T).T
    prev["pos"][0] = prev["pos"][0].astype(np.float64) + dolly * axes[2]
    return prev


# white balance and colour grading (include/rsrt.h "white balance and colour grading", include/rsrt_colour.h): the meter's defaults,
# the identity CDL, the LUT sizes and the parameter blocks
WHITE_WORDS = 4097
WHITE_DEFAULTS = {"gate": 12, "iterations": 3, "min_permille": 50, "strength": 1.0, "max_stops": 2.0, "blend": 1.0, "previous": (0.0, 0.0, 0.0)}
CDL_DEFAULTS = {"slope": 1.0, "offset": 0.0, "power": 1.0, "saturation": 1.0}
COLOUR_LUT_SIZES = (2, 3, 17, 33, 65)


class WhiteParams(C.Structure):
    _fields_ = [("gate", C.c_uint32), ("iterations", C.c_uint32), ("min_permille", C.c_uint32), ("strength", C.c_float), ("max_stops", C.c_float),
                ("blend", C.c_float), ("previous", C.c_float * 3), ("flags", C.c_uint32)]


class WhiteResult(C.Structure):
    _fields_ = [("white", C.c_float * 3), ("target", C.c_float * 3), ("illuminant", C.c_float * 3), ("eu", C.c_float), ("ev", C.c_float),
                ("gated", C.c_uint32), ("counted", C.c_uint32), ("skipped", C.c_uint32), ("estimated", C.c_uint32), ("_pad", C.c_uint32)]


class CdlParams(C.Structure):
    _fields_ = [("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]

    @classmethod
    def of(cls, slope=None, offset=None, power=None, saturation=None, flags=0):
        """CDL_DEFAULTS where None; slope, offset and power are one number for all channels or three."""
        q = {"slope": slope, "offset": offset, "power": power}
        three = lambda k: (C.c_float * 3)(*np.broadcast_to(np.asarray(CDL_DEFAULTS[k] if q[k] is None else q[k], np.float32), (3,)))  # noqa: E731
        return cls(three("slope"), three("offset"), three("power"), CDL_DEFAULTS["saturation"] if saturation is None else saturation, flags, 0)


class ColourParams(C.Structure):
    _fields_ = [("white", C.c_float * 3), ("lut_strength", C.c_float), ("flags", C.c_uint32), ("_pad", C.c_uint32 * 3)]


# the finished display (include/rsrt.h "finished display", include/rsrt_finish.h): its flag, its defaults and its parameters
FINISH_NOISE_AWARE = 1  # rsrt_finish_params.flags: sharpen less where a pixel stands out of its cross
FINISH_DEFAULTS = {"sharpness": 0.5, "grain": 0.0, "dither": 1.0, "seed": 0, "flags": 0}


class FinishParams(C.Structure):
    _fields_ = [("sharpness", C.c_float), ("grain", C.c_float), ("dither", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32 * 3)]


# the HDR display (include/rsrt.h "HDR display", include/rsrt_hdr.h): its encodings, its defaults, its parameters and its light levels
HDR_PQ10, HDR_SCRGB16F = 0, 1
HDR_ENCODINGS = {"pq10": HDR_PQ10, "scrgb16f": HDR_SCRGB16F}
HDR_DEFAULTS = {"paper_white": 203.0, "peak": 1000.0, "knee": 0.5, "dither": 0.0, "seed": 0, "encoding": "pq10", "flags": 0}


class HdrParams(C.Structure):
    _fields_ = [("paper_white_nits", C.c_float), ("peak_nits", C.c_float), ("knee", C.c_float), ("dither", C.c_float), ("seed", C.c_uint32),
                ("encoding", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class HdrLevels(C.Structure):
    _fields_ = [("sum_q", C.c_uint64), ("max_q", C.c_uint32), ("max_cll", C.c_float), ("max_fall", C.c_float), ("_pad", C.c_uint32)]


def hdr_unpack_pq10(words):
    """The 10-bit codes of RSRT_HDR_PQ10 words (R | G << 10 | B << 20 | 3 << 30): [H, W] uint32 -> [H, W, 3] uint16."""
    w = np.asarray(words, np.uint32)
    return np.stack([(w >> np.uint32(10 * c)) & np.uint32(1023) for c in range(3)], axis=-1).astype(np.uint16)


# the video pass (include/rsrt.h "video output", include/rsrt_video.h): its enumerators, its defaults, its parameters and its frame
VIDEO_BT709, VIDEO_HDR10 = 0, 1
VIDEO_SEMIPLANAR, VIDEO_PLANAR = 0, 1
VIDEO_LIMITED, VIDEO_FULL = 0, 1
VIDEO_SITING_LEFT, VIDEO_SITING_CENTRE, VIDEO_SITING_TOPLEFT = 0, 1, 2  # H.273 chroma sample location types
VIDEO_STANDARDS = {"bt709": VIDEO_BT709, "hdr10": VIDEO_HDR10}
VIDEO_LAYOUTS = {"nv12": (VIDEO_SEMIPLANAR, 8), "i420": (VIDEO_PLANAR, 8), "p010": (VIDEO_SEMIPLANAR, 10), "i420p10": (VIDEO_PLANAR, 10)}  # (layout, depth)
VIDEO_RANGES = {"limited": VIDEO_LIMITED, "full": VIDEO_FULL}
VIDEO_SITINGS = {"left": VIDEO_SITING_LEFT, "centre": VIDEO_SITING_CENTRE, "topleft": VIDEO_SITING_TOPLEFT}
VIDEO_DEFAULTS = {"standard": "bt709", "depth": 8, "layout": "nv12", "range": "limited", "siting": "left", "dither": 0.0, "seed": 0, "flags": 0}


class VideoParams(C.Structure):
    _fields_ = [("standard", C.c_uint32), ("depth", C.c_uint32), ("layout", C.c_uint32), ("range", C.c_uint32), ("siting", C.c_uint32),
                ("dither", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32)]


def video_planes(width, height, depth=8, layout=VIDEO_SEMIPLANAR):
    """rsrt_video_planes: (the frame's byte count, [(offset, pitch, width, height) of each plane, in bytes and samples]).  layout: a
    VIDEO_* enumerator or a name of VIDEO_LAYOUTS, whose depth then counts.  The interleaved plane's width counts both of a pair."""
    if layout in VIDEO_LAYOUTS:
        layout, depth = VIDEO_LAYOUTS[layout]
    if width < 1 or height < 1 or depth not in (8, 10) or layout not in (VIDEO_SEMIPLANAR, VIDEO_PLANAR):
        raise ValueError("video_planes: want a size of at least 1 x 1, depth 8 or 10, a known layout")
    cw, ch, b = (width + 1) // 2, (height + 1) // 2, 2 if depth == 10 else 1
    sizes = [(width, height), (2 * cw, ch)] if layout == VIDEO_SEMIPLANAR else [(width, height), (cw, ch), (cw, ch)]
    planes, at = [], 0
    for w, h in sizes:
        planes.append((at, w * b, w, h))
        at += w * b * h
    return at, planes


# the JPEG pass (include/rsrt.h "JPEG output", include/rsrt_jpeg.h): its enumerators, its defaults, its parameters and its sizes
JPEG_420, JPEG_444 = 0, 1
JPEG_SUBSAMPLINGS = {"420": JPEG_420, "444": JPEG_444}
JPEG_DEFAULTS = {"quality": 90, "subsampling": "420", "flags": 0, "reserved": 0}
JPEG_HEADER_BYTES = 623  # SOI .. SOS
JPEG_BLOCK_BITS = 1664   # a block's slot in the worst case


class JpegParams(C.Structure):
    _fields_ = [("quality", C.c_uint32), ("subsampling", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def jpeg_params(quality=None, subsampling=None):
    """rsrt_jpeg_params of quality 1 .. 100 and subsampling "420", "444" or a JPEG_* enumerator; JPEG_DEFAULTS where None.  What is
    out of range is the library's to refuse."""
    d = JPEG_DEFAULTS
    sub = d["subsampling"] if subsampling is None else subsampling
    return JpegParams(d["quality"] if quality is None else quality, JPEG_SUBSAMPLINGS.get(sub, sub), d["flags"], d["reserved"])


def jpeg_blocks(width, height, subsampling="420"):
    """rsrt_jpeg_blocks: the 8 x 8 blocks of a width x height picture's scan, partial MCUs whole."""
    side, per = (8, 3) if JPEG_SUBSAMPLINGS.get(subsampling, subsampling) == JPEG_444 else (16, 6)
    return -(-width // side) * -(-height // side) * per


def jpeg_max_bytes(width, height, subsampling="420"):
    """rsrt_jpeg_max_bytes: the room that always suffices for a width x height file."""
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        return 0
    return JPEG_HEADER_BYTES + 2 * (JPEG_BLOCK_BITS // 8) * jpeg_blocks(width, height, subsampling) + 2


class VideoFrame:
    """A frame of State.display_video: `data` the bytes as laid out (uint8 [n]: what an encoder or rsrt_y4m_write takes), `y` [H, W], `cb`,
    `cr` [ceil(H / 2), ceil(W / 2)] numpy views of the codes (a copy with the shift removed for P010, whose words are code << 6), `width`,
    `height` and `params` (the VideoParams of the call)."""

    def __init__(self, data, width, height, params):
        self.data, self.width, self.height, self.params = data, width, height, params

    def _planes(self):
        p = self.params
        _, planes = video_planes(self.width, self.height, p.depth, p.layout)
        t = np.dtype("<u2") if p.depth == 10 else np.dtype(np.uint8)
        views = [self.data[at:at + pitch * h].view(t).reshape(h, w) for at, pitch, w, h in planes]
        if p.layout == VIDEO_SEMIPLANAR:
            c = views[1].reshape(views[1].shape[0], -1, 2)
            views = [views[0], c[..., 0], c[..., 1]]
            if p.depth == 10:
                views = [v >> 6 for v in views]
        return views

    y = property(lambda self: self._planes()[0])
    cb = property(lambda self: self._planes()[1])
    cr = property(lambda self: self._planes()[2])


# the procedural daylight sky (include/rsrt.h rsrt_environment_sky, include/rsrt_sky.h): its defaults (RSRT_SKY_*) and its parameters.
# Angles in radians; the elevation's range is 1 .. 90 degrees, the turbidity's 2 .. 10
SKY_DEFAULTS = {"sun_azimuth": 0.0, "sun_elevation": 0.78539816339744830962, "turbidity": 3.0, "ground_albedo": (0.2, 0.2, 0.2), "scale": 1.0 / 64,
                "sun_illuminance": 128.0, "sun_radius": 0.00465, "flags": 0}


class SkyParams(C.Structure):
    _fields_ = [("sun_azimuth", C.c_float), ("sun_elevation", C.c_float), ("turbidity", C.c_float), ("ground_albedo", C.c_float * 3),
                ("scale", C.c_float), ("sun_illuminance", C.c_float), ("sun_radius", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, **params):
        """SKY_DEFAULTS with `params` over them; an unknown name is a TypeError."""
        unknown = set(params) - set(SKY_DEFAULTS)
        if unknown:
            raise TypeError("unknown sky parameter(s): " + ", ".join(sorted(unknown)))
        p = dict(SKY_DEFAULTS, **params)
        return cls(p["sun_azimuth"], p["sun_elevation"], p["turbidity"], (C.c_float * 3)(*p["ground_albedo"]), p["scale"], p["sun_illuminance"],
                   p["sun_radius"], p["flags"])


# volumetric fog (include/rsrt.h "volumetric fog", include/rsrt_fog.h): the sources the passes after it can read — the six images and
# the fog image rsrt_fog_apply leaves — its defaults (RSRT_FOG_*; the light has none: fog_light_from_sky gives a sky's sun) and its
# parameters
ALL_SOURCES = dict(DISPLAY_SOURCES, fog=6)
FOG_JITTER = 1
FOG_MAX_STEPS = 64
FOG_FLOATS = 4  # per pixel: inscatter sum rgb, transmittance sum
FOG_DEFAULTS = {"density": 0.05, "albedo": (1.0, 1.0, 1.0), "anisotropy": 0.6, "light_dir": (0.0, 1.0, 0.0), "light_irradiance": (1.0, 1.0, 1.0),
                "ambient": (0.0, 0.0, 0.0), "max_distance": 50.0, "steps": 16, "flags": FOG_JITTER}


class FogParams(C.Structure):
    _fields_ = [("density", C.c_float), ("albedo", C.c_float * 3), ("anisotropy", C.c_float), ("light_dir", C.c_float * 3),
                ("light_irradiance", C.c_float * 3), ("ambient", C.c_float * 3), ("max_distance", C.c_float), ("steps", C.c_uint32),
                ("flags", C.c_uint32)]

    @classmethod
    def of(cls, **params):
        """FOG_DEFAULTS with `params` over them (albedo, light_irradiance, ambient: one number for all channels or three; jitter=bool sets
        flags); an unknown name is a TypeError."""
        if "jitter" in params:
            params = dict(params)
            params["flags"] = FOG_JITTER if params.pop("jitter") else 0
        unknown = set(params) - set(FOG_DEFAULTS)
        if unknown:
            raise TypeError("unknown fog parameter(s): " + ", ".join(sorted(unknown)))
        p = dict(FOG_DEFAULTS, **params)
        three = lambda k: (C.c_float * 3)(*np.broadcast_to(np.asarray(p[k], np.float32), (3,)))  # noqa: E731
        return cls(p["density"], three("albedo"), p["anisotropy"], three("light_dir"), three("light_irradiance"), three("ambient"), p["max_distance"],
                   p["steps"], p["flags"])


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("depth_tolerance", C.c_float), ("normal_tolerance", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float)]


class SceneImageInfo(C.Structure):
    """rsrt_scene_image_info (include/rsrt.h): where each section of the scene's device image lies, in float4s, and the scalars
    rsrt_upload_scene derives with it.  lib().rsrt_scene_image_build fills one on the CPU, without a context."""
    _fields_ = ([(n, C.c_uint64) for n in ("nodes", "escape", "prims", "tri_normals", "materials", "fb_spheres", "fb_planes", "flat_leaves",
                                            "flat_rank", "pnodes", "prim_rank", "wnodes", "n_float4", "traversal_head_f4")] +
                [(n, C.c_uint32) for n in ("n_nodes", "n_prims", "n_tris", "n_materials", "n_spheres", "n_planes", "n_leaves", "n_pnodes",
                                            "n_wnodes", "tri_mask_lo", "tri_mask_hi", "plane_mask_lo", "plane_mask_hi", "flat_ok", "flat_ostride",
                                            "typed_leaves", "wide_ok", "wide_deep", "coop_ok", "stack_entries", "lds_float4s")] +
                [("cull_min", C.c_float * 3 * 8), ("cull_max", C.c_float * 3 * 8), ("cull_mask", C.c_uint32 * 8)] +
                [(n, C.c_uint32) for n in ("cull_always", "n_cull", "top_elems", "wimg_nodes", "small_image_bytes", "hybrid_room_f4", "_pad")])


def build_id():
    """rsrt_build_id(): which kernel sources the loaded librsrt.so was compiled from."""
    return lib().rsrt_build_id().decode()


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("ext_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_paths", C.c_uint64), ("total_ext_rays", C.c_uint64), ("total_shadow_rays", C.c_uint64),
                ("total_kernel_ms", C.c_double), ("launches", C.c_uint32), ("_pad", C.c_uint32),
                ("trace_kernel_ms", C.c_double), ("resolve_kernel_ms", C.c_double), ("reduce_ms", C.c_double), ("traversal_steps", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


_lib = None


def lib():
    """Loads librsrt.so (building it in-tree when sources are newer). Raises if it cannot be loaded."""
    global _lib
    if _lib is None:
        try:
            import os
            path = os.environ.get("RSRT_LIB") or _build.build_hip(instrument=os.environ.get("RSRT_INSTRUMENT") == "1")  # RSRT_LIB: experiment builds (tools/flag_sweep.sh)
            L = C.CDLL(path)
        except Exception as e:  # noqa: BLE001
            raise RsrtError("librsrt.so (the HIP integrator) is not available: %s" % e) from e
        for s in _SYMBOLS:
            getattr(L, s)
        L.rsrt_last_error.restype = C.c_char_p
        L.rsrt_last_error.argtypes = [C.c_void_p]
        L.rsrt_describe.restype = C.c_char_p
        L.rsrt_describe.argtypes = [C.c_void_p]
        L.rsrt_build_id.restype = C.c_char_p
        L.rsrt_build_id.argtypes = []
        L.rsrt_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.rsrt_context_destroy.argtypes = [C.c_void_p]
        L.rsrt_upload_scene.argtypes = [C.c_void_p] + [C.c_void_p, C.c_uint32] * 8
        L.rsrt_upload_environment.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_set_partition.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rsrt_accumulator_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_accumulator_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_accumulator_clear.argtypes = [C.c_void_p]
        L.rsrt_accumulator_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_resolve_mean_f16.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_debug_view_f16.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_display_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_render.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p]
        L.rsrt_synchronize.argtypes = [C.c_void_p]
        L.rsrt_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_get_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_get_region_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_get_walk_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rsrt_selftest_numerics.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_selftest_sincos.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_cast_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_scene_image_build.argtypes = [C.c_void_p, C.c_uint32] * 8 + [C.c_uint32, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(SceneImageInfo)]
        L.rsrt_partition_owner.restype = C.c_uint32
        L.rsrt_partition_owner.argtypes = [C.c_uint32] * 7
        L.rsrt_partition_mask.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]
        L.rsrt_partition_tiles.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]
        L.rsrt_comm_available.restype = C.c_int
        L.rsrt_comm_available.argtypes = []
        L.rsrt_comm_unique_id.argtypes = [C.c_void_p]
        L.rsrt_comm_init.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_comm_reduce.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_comm_destroy.argtypes = [C.c_void_p]
        L.rsrt_comm_set_mode.argtypes = [C.c_void_p, C.c_uint32]
        L.rsrt_multi_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rsrt_multi_destroy.argtypes = [C.c_void_p]
        L.rsrt_multi_last_error.restype = C.c_char_p
        L.rsrt_multi_last_error.argtypes = [C.c_void_p]
        L.rsrt_multi_size.restype = C.c_uint32
        L.rsrt_multi_size.argtypes = [C.c_void_p]
        L.rsrt_multi_context.restype = C.c_void_p
        L.rsrt_multi_context.argtypes = [C.c_void_p, C.c_uint32]
        L.rsrt_multi_upload_scene.argtypes = [C.c_void_p] + [C.c_void_p, C.c_uint32] * 8
        L.rsrt_multi_upload_environment.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_multi_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_multi_clear.argtypes = [C.c_void_p]
        L.rsrt_multi_render.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7
        L.rsrt_multi_synchronize.argtypes = [C.c_void_p]
        L.rsrt_multi_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_multi_display_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_multi_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.rsrt_multi_uses_rccl.argtypes = [C.c_void_p]
        L.rsrt_aov_render.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p]
        L.rsrt_aov_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_aov_clear.argtypes = [C.c_void_p]
        L.rsrt_aov_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_denoise.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsrt_denoised_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_denoised_display_srgb8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_temporal_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_temporal_reset.argtypes = [C.c_void_p]
        L.rsrt_temporal_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_temporal_accumulate_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.rsrt_temporal_moments_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_guide_render.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p]
        L.rsrt_guide_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_guide_clear.argtypes = [C.c_void_p]
        L.rsrt_guide_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_upsample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsrt_upsampled_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_upsampled_display_srgb8.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_noise_snapshot.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.rsrt_noise_estimate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_noise_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_noise_reset.argtypes = [C.c_void_p]
        L.rsrt_exposure_meter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_exposure_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_exposure_reset.argtypes = [C.c_void_p]
        L.rsrt_display_exposed_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t]
        L.rsrt_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        L.rsrt_bloom_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rsrt_bloom_reset.argtypes = [C.c_void_p]
        L.rsrt_display_bloomed_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_size_t]
        L.rsrt_local_exposure.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_local_exposure_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_local_exposure_reset.argtypes = [C.c_void_p]
        L.rsrt_local_gain_download.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_display_local_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t]
        L.rsrt_dof.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsrt_dof_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rsrt_dof_coc_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_dof_depth_at.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_dof_reset.argtypes = [C.c_void_p]
        L.rsrt_motion_blur.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsrt_motion_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rsrt_motion_velocity_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_motion_tiles_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.rsrt_motion_reset.argtypes = [C.c_void_p]
        L.rsrt_fog_render.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        L.rsrt_fog_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rsrt_fog_clear.argtypes = [C.c_void_p]
        L.rsrt_fog_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_fog_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_fog_apply_upsampled.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rsrt_fog_image_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_fog_reset.argtypes = [C.c_void_p]
        L.rsrt_environment_sky.argtypes =[C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_environment_download.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_white_meter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rsrt_white_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_white_reset.argtypes = [C.c_void_p]
        L.rsrt_colour_lut_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rsrt_colour_lut_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        L.rsrt_colour_lut_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_colour_lut_reset.argtypes = [C.c_void_p]
        L.rsrt_display_colour_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_display_finished_srgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_display_hdr.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_display_jpeg.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_display_jpeg_coefficients.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.rsrt_jpeg_encode_coefficients.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rsrt_display_video.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class State:
    def __init__(self, device=0):
        self._L = lib()
        self._ctx = C.c_void_p()
        rc = self._L.rsrt_context_create(device, C.byref(self._ctx))
        if rc != 0:
            raise RsrtError("rsrt_context_create: %s" % self._L.rsrt_last_error(None).decode())
        self.width = self.height = 0
        self.sample_count = 0          # hdr.sample_count (state.rs:775-789)
        self.max_bounces = 10          # MAX_BOUNCES (shader.wgsl:232)
        self.environment_index = 0     # state.rs:638
        self.camera = None
        self._last_hash = None
        self.flags = 0
        self.aov_sample_count = 0      # samples in the AOV buffer (render_samples(aov=True) / render_aov)
        self._has_aov = False
        self.temporal_sample_count = 0  # first sample index of the next render_temporal frame (only grows until temporal_reset)
        self._temporal_key = None       # what the history was rendered under: environment, bounces, flags, size
        self.guide_sample_count = 0     # samples in the upsampler's guide (render_guide / render_upsampled)
        self.guide_width = self.guide_height = 0  # the guide's size: what upsample() returns
        self._guide_bound = False
        self.exposure = None            # the last auto_exposure() (None: none since exposure_reset)
        self.white = None               # the last auto_white_balance()'s white point (None: none since white_reset)
        self.focus_distance = None      # the last focus_at() that hit a surface (None: depth_of_field takes DOF_DEFAULTS')
        self.motion_camera = None       # the camera of the last motion_blur() (None: the next one takes its own camera as the previous)
        self._env_sizes = {}            # slot -> (width, height) of what upload_environment / environment_sky put there
        self.fog_sample_count = 0       # samples in the fog records (render_fog)
        self.fog_params = None          # the FogParams the records were rendered with (None: none since clear_fog / fog_reset)
        self.fog_width = self.fog_height = 0  # the records' size
        self._fog_shape = None          # (H, W) of the last fog() image
        self._fog_bound = False

    # -- construction ---------------------------------------------------------------------------
    @classmethod
    def new(cls, scene, environments, width, height, device=0, camera=None):
        st = cls(device)
        st.upload_scene(scene)
        for i, env in enumerate(environments if isinstance(environments, (list, tuple)) else [environments]):
            st.upload_environment(i, env)
        st.resize(width, height)
        st.camera = np.array(camera if camera is not None else scene.camera_uniform()).view(T.CAMERA).reshape(1).copy()
        return st

    def _check(self, rc, what):
        if rc != 0:
            raise RsrtError("%s failed (%d): %s" % (what, rc, self._L.rsrt_last_error(self._ctx).decode()), rc)

    def _total(self, sample_total):
        """The samples in the accumulator a pass is told of: sample_count unless given."""
        return self.sample_count if sample_total is None else sample_total

    def _source_total(self, source, sample_total):
        """(source id, sample total) as the image passes' entry points take them: `source` a name of ALL_SOURCES or an id."""
        return ALL_SOURCES.get(source, source), self._total(sample_total)

    def _displayed(self, name, source, sample_total, *args):
        """The display `name`(ctx, source, sample_total, *args, bytes, their number) into [H, W, 4] uint8 of the source's own shape."""
        out = np.empty(self._source_shape(source) + (4,), np.uint8)
        self._check(getattr(self._L, name)(self._ctx, *self._source_total(source, sample_total), *args, _p(out), out.size), name)
        return out

    def _colour_params(self, white, lut_strength):
        """rsrt_colour_params: `white` (None: the remembered white point, else (1, 1, 1)), lut_strength (None: 1 with a LUT, 0 without)."""
        if white is None:
            white = (1.0, 1.0, 1.0) if self.white is None else self.white
        if lut_strength is None:
            lut_strength = 1.0 if self._has_colour_lut() else 0.0
        return ColourParams((C.c_float * 3)(*white), lut_strength, 0, (C.c_uint32 * 3)())

    def close(self):
        if self._ctx:
            self._L.rsrt_context_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def describe(self):
        return self._L.rsrt_describe(self._ctx).decode()

    def upload_scene(self, scene):
        a = [scene.materials, scene.spheres, scene.planes, scene.vertices, scene.normals, scene.triangles, scene.primitives,
             scene.bvh_nodes]
        dts = [T.MATERIAL, T.SPHERE, T.PLANE, T.VEC3, T.VEC3, T.TRIANGLE, T.PRIMITIVE_INFO, T.BVH_NODE]
        args = []
        for arr, dt in zip(a, dts):
            arr = np.ascontiguousarray(arr)
            assert arr.dtype.itemsize == dt.itemsize, (arr.dtype, dt)
            args += [_p(arr), len(arr)]
        self._keep = a
        self._check(self._L.rsrt_upload_scene(self._ctx, *args), "rsrt_upload_scene")

    def upload_environment(self, slot, env):
        rgba = np.ascontiguousarray(env.rgba, dtype=np.float32)
        alias = np.ascontiguousarray(env.alias)
        assert rgba.shape == (env.height, env.width, 4) and alias.dtype.itemsize == 16 and len(alias) == env.width * env.height
        self._check(self._L.rsrt_upload_environment(self._ctx, slot, env.width, env.height, _p(rgba), _p(alias)),
                    "rsrt_upload_environment")
        self._env_sizes[slot] = (env.width, env.height)

    def environment_sky(self, slot, width=2048, height=1024, **params):
        """rsrt_environment_sky: fills `slot` with the procedural daylight sky of `params` (SKY_DEFAULTS otherwise: sun_azimuth,
        sun_elevation in radians, turbidity, ground_albedo, scale, sun_illuminance, sun_radius) and builds its alias table, all on the
        device.  Like upload_environment it replaces what the slot held, drops the temporal history and leaves the accumulator alone
        (clear() restarts a progressive picture); a refused call changes no slot.  host.Environment.sky gives the same texels on the
        CPU."""
        p = SkyParams.of(**params)
        self._check(self._L.rsrt_environment_sky(self._ctx, slot, width, height, C.byref(p)), "rsrt_environment_sky")
        self._env_sizes[slot] = (width, height)

    def environment_download(self, slot, width=None, height=None):
        """rsrt_environment_download: the texels of `slot`, [H, W, 4] float32 with alpha 0, whether a sky or an upload filled it.  The
        size is the one this State put there; give width and height for a slot filled behind its back."""
        w, h = (width, height) if width and height else self._env_sizes.get(slot, (0, 0))
        out = np.empty((h, w, 4), np.float32)
        self._check(self._L.rsrt_environment_download(self._ctx, slot, _p(out), out.size), "rsrt_environment_download")
        return out

    def set_partition(self, rank, world_size, tile_w=16, tile_h=16):
        self._check(self._L.rsrt_set_partition(self._ctx, rank, world_size, tile_w, tile_h), "rsrt_set_partition")

    # -- multi-GPU, one process per GPU: the RCCL reduce lives in the library (include/rsrt.h) -----
    @staticmethod
    def comm_unique_id():
        """Rank 0: the 128 bytes every rank passes to comm_init (hand them over by any channel)."""
        L = lib()
        buf = C.create_string_buffer(128)
        rc = L.rsrt_comm_unique_id(buf)
        if rc != 0:
            raise RsrtError("rsrt_comm_unique_id failed (%d): %s" % (rc, L.rsrt_last_error(None).decode()))
        return buf.raw

    @staticmethod
    def comm_available():
        """True when librccl can be loaded (a dlopen, no collective): every rank asks BEFORE the collective comm_init."""
        return bool(lib().rsrt_comm_available())

    def comm_init(self, rank, world_size, unique_id):
        assert len(unique_id) == 128
        self._check(self._L.rsrt_comm_init(self._ctx, rank, world_size, C.create_string_buffer(unique_id, 128)), "rsrt_comm_init")

    def comm_reduce(self, root=0, recv_ptr=None, stream=None):
        """The exchange step: every rank's tiles onto `root` over RCCL (in place unless recv_ptr names a device buffer)."""
        self._check(self._L.rsrt_comm_reduce(self._ctx, root, C.c_void_p(recv_ptr) if recv_ptr else None,
                                             C.c_void_p(stream) if stream else None), "rsrt_comm_reduce")

    def comm_set_mode(self, dense_reduce):
        """False: the exchange is the gather of compact tile buffers (default); True: the dense ncclReduce of the full accumulators."""
        self._check(self._L.rsrt_comm_set_mode(self._ctx, 1 if dense_reduce else 0), "rsrt_comm_set_mode")

    def comm_destroy(self):
        self._check(self._L.rsrt_comm_destroy(self._ctx), "rsrt_comm_destroy")

    # -- State::resize / update / render --------------------------------------------------------
    def resize(self, width, height):
        self._check(self._L.rsrt_accumulator_resize(self._ctx, width, height), "rsrt_accumulator_resize")
        self.width, self.height = width, height
        self._last_hash = None

    def bind_accumulator(self, device_ptr, width, height):
        """Use caller-owned device memory (W*H*4 f32), e.g. a torch tensor's data_ptr()."""
        self._check(self._L.rsrt_accumulator_bind(self._ctx, C.c_void_p(device_ptr), width, height), "rsrt_accumulator_bind")
        self.width, self.height = width, height
        self._last_hash = None

    def update(self, camera=None, environment_index=None):
        if camera is not None:
            self.camera = np.array(camera).view(T.CAMERA).reshape(1).copy()
        if environment_index is not None:
            self.environment_index = environment_index

    def _scene_hash(self):
        return hash((self.camera.tobytes(), self.environment_index))

    def clear(self):
        self._check(self._L.rsrt_accumulator_clear(self._ctx), "rsrt_accumulator_clear")
        self.sample_count = 0

    def render_samples(self, n, stream=None, aov=False):
        """Adds samples [sample_count, sample_count+n); resets first when camera/environment changed.  aov=True: the AOV pass
        (render_aov) over the same sample range too."""
        h = self._scene_hash()
        if h != self._last_hash:  # state.rs:778-786
            self._last_hash = h
            self.clear()
            if self._has_aov:
                self.clear_aov()
            if self.guide_width:
                self.clear_guide()
        self._check(self._L.rsrt_render(self._ctx, _p(self.camera), self.width, self.height, self.sample_count, n,
                                        self.max_bounces, self.environment_index, self.flags,
                                        C.c_void_p(stream) if stream else None), "rsrt_render")
        if aov:
            self.render_aov(self.sample_count, n, stream=stream)
        self.sample_count += n

    def render(self):
        """One reference frame: exactly one more sample per pixel."""
        self.render_samples(1)

    def render_range(self, sample_begin, sample_count, stream=None):
        """Raw rsrt_render: no hash check, no counter update."""
        self._check(self._L.rsrt_render(self._ctx, _p(self.camera), self.width, self.height, sample_begin, sample_count,
                                        self.max_bounces, self.environment_index, self.flags,
                                        C.c_void_p(stream) if stream else None), "rsrt_render")

    def synchronize(self):
        self._check(self._L.rsrt_synchronize(self._ctx), "rsrt_synchronize")

    # -- denoiser (include/rsrt.h "denoiser") -------------------------------------------------------
    def render_aov(self, sample_begin, sample_count, stream=None):
        """rsrt_aov_render: adds the first hits of the camera rays of samples [sample_begin, sample_begin + sample_count) to the
        AOV buffer.  Raw, like render_range: no hash check; aov_sample_count grows by sample_count."""
        self._check(self._L.rsrt_aov_render(self._ctx, _p(self.camera), self.width, self.height, sample_begin, sample_count, 0,
                                            C.c_void_p(stream) if stream else None), "rsrt_aov_render")
        self._has_aov = True
        self.aov_sample_count += sample_count

    def bind_aov(self, device_ptr, width, height):
        """Use caller-owned device memory (W*H*8 f32) as the AOV buffer (None: back to the library's)."""
        self._check(self._L.rsrt_aov_bind(self._ctx, C.c_void_p(device_ptr) if device_ptr else None, width, height), "rsrt_aov_bind")
        self._has_aov = bool(device_ptr)

    def clear_aov(self):
        self._check(self._L.rsrt_aov_clear(self._ctx), "rsrt_aov_clear")
        self.aov_sample_count = 0

    def download_aov(self):
        """[H, W, 8] float32: albedo sum xyz, hits, normal sum xyz, distance sum."""
        out = np.empty((self.height, self.width, AOV_FLOATS), np.float32)
        self._check(self._L.rsrt_aov_download(self._ctx, _p(out), out.size), "rsrt_aov_download")
        return out

    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, sample_total=None,
                aov_sample_total=None, out_ptr=None, stream=None, download=True, temporal=False, variance=False, clamp=False):
        """rsrt_denoise of the accumulator's mean, guided by the AOV buffer: [H, W, 4] float32 (alpha 1), or None with download=False
        (the result stays on the device: denoised_display_srgb8, or out_ptr when given).  Unset arguments take DENOISE_DEFAULTS and
        the sample counters.  temporal=True: of the last render_temporal frame's colour instead (RSRT_DENOISE_TEMPORAL).
        variance=True: variance-guided levels (RSRT_DENOISE_VARIANCE; sigma_color is then sigma_l and defaults to VARIANCE_SIGMA_L; with
        temporal=True the last frame must have been rendered with moments=True); clamp=True: the firefly clamp (RSRT_DENOISE_CLAMP)."""
        d = DENOISE_DEFAULTS
        pick = lambda v, k: d[k] if v is None else v  # noqa: E731
        flags = (DENOISE_DEMODULATE if pick(demodulate, "demodulate") else 0) | (DENOISE_TEMPORAL if temporal else 0) \
            | (DENOISE_VARIANCE if variance else 0) | (DENOISE_CLAMP if clamp else 0)
        if sigma_color is None and variance:
            sigma_color = VARIANCE_SIGMA_L
        p = DenoiseParams(pick(iterations, "iterations"), flags, pick(sigma_color, "sigma_color"), pick(sigma_normal, "sigma_normal"),
                          pick(sigma_depth, "sigma_depth"))
        n = self._total(sample_total)
        na = self.aov_sample_count if aov_sample_total is None else aov_sample_total
        self._check(self._L.rsrt_denoise(self._ctx, n, na, C.byref(p), C.c_void_p(out_ptr) if out_ptr else None,
                                         C.c_void_p(stream) if stream else None), "rsrt_denoise")
        if not download:
            return None
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rsrt_denoised_download(self._ctx, _p(out), out.size), "rsrt_denoised_download")
        return out

    def denoised_display_srgb8(self):
        """The last denoise() output through the display pass (rsrt_display_pixel(denoised, 1)): [H, W, 4] uint8."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rsrt_denoised_display_srgb8(self._ctx, _p(out), out.size), "rsrt_denoised_display_srgb8")
        return out

    # -- guided upsampling (include/rsrt.h "guided upsampling") --------------------------------------
    # The state's own size (resize) is the LOW size the paths are traced at; the guide has the output's.  The caller picks a low size of
    # the output's aspect: ceil(W / 2) x ceil(H / 2) for half size.  The guide wants as many samples as the low frame.
    def render_guide(self, width, height, sample_begin, sample_count, stream=None):
        """rsrt_guide_render: adds the first hits of the camera rays of samples [sample_begin, sample_begin + sample_count), for a frame of
        width x height, to the guide.  Raw, like render_aov: no hash check; guide_sample_count grows by sample_count."""
        self._check(self._L.rsrt_guide_render(self._ctx, _p(self.camera), width, height, sample_begin, sample_count, 0,
                                              C.c_void_p(stream) if stream else None), "rsrt_guide_render")
        self.guide_width, self.guide_height = width, height
        self.guide_sample_count += sample_count

    def bind_guide(self, device_ptr, width, height):
        """Use caller-owned device memory (W*H*8 f32) as the guide (None: back to the library's, which the next render_guide allocates)."""
        self._check(self._L.rsrt_guide_bind(self._ctx, C.c_void_p(device_ptr) if device_ptr else None, width, height), "rsrt_guide_bind")
        if device_ptr:
            self.guide_width, self.guide_height, self._guide_bound = width, height, True
        elif self._guide_bound:  # (the library gave its own buffer up at the bind)
            self.guide_width, self.guide_height, self._guide_bound = 0, 0, False

    def clear_guide(self):
        self._check(self._L.rsrt_guide_clear(self._ctx), "rsrt_guide_clear")
        self.guide_sample_count = 0

    def download_guide(self):
        """[H, W, 8] float32 of the guide's size: albedo sum xyz, hits, normal sum xyz, distance sum."""
        out = np.empty((self.guide_height, self.guide_width, AOV_FLOATS), np.float32)
        self._check(self._L.rsrt_guide_download(self._ctx, _p(out), out.size), "rsrt_guide_download")
        return out

    def upsample(self, source="mean", sigma_normal=None, sigma_depth=None, demodulate=None, sample_total=None, aov_sample_total=None,
                 guide_sample_total=None, out_ptr=None, stream=None, download=True):
        """rsrt_upsample of the low frame to the guide's size: [H, W, 4] float32 (alpha 1), or None with download=False (the result stays
        on the device: upsampled_display_srgb8, or out_ptr when given).  source: "mean" (the accumulator's), "denoised" (the last
        denoise() output) or "temporal" (the last render_temporal frame's colour).  Unset arguments take UPSAMPLE_DEFAULTS and the
        sample counters."""
        d = UPSAMPLE_DEFAULTS
        pick = lambda v, k: d[k] if v is None else v  # noqa: E731
        src = {"mean": 0, "denoised": UPSAMPLE_DENOISED, "temporal": UPSAMPLE_TEMPORAL}
        if source not in src:
            raise ValueError("upsample: source is 'mean', 'denoised' or 'temporal', not %r" % (source,))
        p = UpsampleParams((UPSAMPLE_DEMODULATE if pick(demodulate, "demodulate") else 0) | src[source], pick(sigma_normal, "sigma_normal"),
                           pick(sigma_depth, "sigma_depth"))
        n = self._total(sample_total)
        na = self.aov_sample_count if aov_sample_total is None else aov_sample_total
        ng = self.guide_sample_count if guide_sample_total is None else guide_sample_total
        self._check(self._L.rsrt_upsample(self._ctx, n, na, ng, C.byref(p), C.c_void_p(out_ptr) if out_ptr else None,
                                          C.c_void_p(stream) if stream else None), "rsrt_upsample")
        if not download:
            return None
        out = np.empty((self.guide_height, self.guide_width, 4), np.float32)
        self._check(self._L.rsrt_upsampled_download(self._ctx, _p(out), out.size), "rsrt_upsampled_download")
        return out

    def upsampled_display_srgb8(self):
        """The last upsample() output through the display pass (rsrt_display_pixel(upsampled, 1)): [H, W, 4] uint8."""
        out = np.empty((self.guide_height, self.guide_width, 4), np.uint8)
        self._check(self._L.rsrt_upsampled_display_srgb8(self._ctx, _p(out), out.size), "rsrt_upsampled_display_srgb8")
        return out

    def render_upsampled(self, out_width, out_height, n=1, denoise=True):
        """One progressive step of a picture of out_width x out_height traced at the state's own (low) size: render_samples(n, aov=True),
        the guide over the same samples at the output size (cleared first when the camera / environment changed or its size differs),
        denoise() and upsample("denoised") — or upsample("mean") with denoise=False.  Returns the picture, [out_height, out_width, 4]."""
        begin = self.sample_count if self._scene_hash() == self._last_hash else 0
        self.render_samples(n, aov=True)  # (a changed camera / environment cleared the guide with the accumulator)
        if (self.guide_width, self.guide_height) != (out_width, out_height):
            self.guide_sample_count = 0  # a guide of another size is allocated zeroed
        self.render_guide(out_width, out_height, begin, n)
        if denoise:
            self.denoise(download=False)
        return self.upsample("denoised" if denoise else "mean")

    # -- noise estimate (include/rsrt.h "noise estimate") --------------------------------------------
    def noise_snapshot(self, sample_total=None, stream=None):
        """rsrt_noise_snapshot: keeps a copy of the accumulator, the sum of sample_total (default: sample_count) samples."""
        self._check(self._L.rsrt_noise_snapshot(self._ctx, self._total(sample_total), C.c_void_p(stream) if stream else None), "rsrt_noise_snapshot")

    def noise_estimate(self, tile=(16, 16), threshold=0.0, sample_total=None, stream=None, download=True):
        """rsrt_noise_estimate of the accumulator (sample_total samples, default sample_count) against the last noise_snapshot():
        (tile map [tiles_y, tiles_x] float32, summary dict with max_error, mean_error, tiles_x, tiles_y, tiles_above), or None with
        download=False (noise_download() fetches it later)."""
        p = NoiseParams(tile[0], tile[1], threshold, 0)
        self._check(self._L.rsrt_noise_estimate(self._ctx, self._total(sample_total), C.byref(p), C.c_void_p(stream) if stream else None), "rsrt_noise_estimate")
        return self.noise_download() if download else None

    def noise_download(self):
        """The last noise_estimate(): (tile map [tiles_y, tiles_x] float32, summary dict)."""
        s = NoiseSummary()
        self._check(self._L.rsrt_noise_download(self._ctx, None, 0, C.byref(s)), "rsrt_noise_download")
        tiles = np.empty((s.tiles_y, s.tiles_x), np.float32)
        self._check(self._L.rsrt_noise_download(self._ctx, _p(tiles), tiles.size, C.byref(s)), "rsrt_noise_download")
        return tiles, {"max_error": s.max_error, "mean_error": s.mean_error, "tiles_x": s.tiles_x, "tiles_y": s.tiles_y,
                       "tiles_above": s.tiles_above}

    def noise_reset(self):
        """Drops the snapshot and the last estimate (clear(), resize() and a bind of another size do so too)."""
        self._check(self._L.rsrt_noise_reset(self._ctx), "rsrt_noise_reset")

    def render_to_noise(self, threshold, min_samples=8, max_samples=1024, tile=(16, 16), on_round=None, exposure=None):
        """Renders until the largest tile error is at most `threshold` or max_samples are in: clears and renders min_samples, then per
        round snapshots at n samples, renders up to min(2 n, max_samples) and estimates.  Returns (total, rounds), rounds a list of
        (n1, n2, max_error, mean_error, tiles_above); on_round, when given, is called with each as it is known.  The accumulator is
        what render_samples(total) leaves from a clear, bit for bit: the estimate only reads it.  exposure: None compares the errors
        with `threshold` itself; a float E, or "auto" (metered once with blend 1 after the min_samples render, and remembered),
        compares them with threshold / sqrt(E) in f32 — the threshold is then in displayed units."""
        if not (min_samples >= 1 and max_samples > min_samples):
            raise ValueError("render_to_noise: 1 <= min_samples < max_samples")
        self._last_hash = None  # start from a clear, whatever was rendered before
        self.render_samples(min_samples)
        if exposure is not None:
            if exposure == "auto":
                self.exposure = None
                exposure = self.auto_exposure()["exposure"]
            with np.errstate(all="ignore"):
                threshold = float(np.float32(threshold) / np.sqrt(np.float32(exposure)))
        rounds = []
        while True:
            n1 = self.sample_count
            self.noise_snapshot()
            self.render_samples(min(2 * n1, max_samples) - n1)
            _, s = self.noise_estimate(tile, threshold)
            rounds.append((n1, self.sample_count, s["max_error"], s["mean_error"], s["tiles_above"]))
            if on_round:
                on_round(rounds[-1])
            if s["max_error"] <= threshold or self.sample_count >= max_samples:
                return self.sample_count, rounds

    # -- auto-exposure (include/rsrt.h "auto-exposure") -----------------------------------------------
    def exposure_meter(self, source="mean", sample_total=None, stream=None):
        """rsrt_exposure_meter: builds the luminance histogram of `source` ("mean": the accumulator over sample_total, default
        sample_count; "denoised", "temporal", "upsampled", "lens": the last depth_of_field(), "motion": the last motion_blur()) on the device.  Asynchronous."""
        self._check(self._L.rsrt_exposure_meter(self._ctx, *self._source_total(source, sample_total), C.c_void_p(stream) if stream else None),
                    "rsrt_exposure_meter")

    def exposure_download(self, **params):
        """rsrt_exposure_download of the last exposure_meter(): (histogram, 257 uint32: 256 bins and the skipped pixels; result dict
        with exposure, target, average_luminance, metered, skipped).  params: rsrt_exposure_params fields, EXPOSURE_DEFAULTS otherwise."""
        q = dict(EXPOSURE_DEFAULTS, **params)
        p = ExposureParams(q["low_permille"], q["high_permille"], q["key"], q["min_exposure"], q["max_exposure"], q["blend"],
                           q["previous_exposure"], 0)
        hist = np.zeros(EXPOSURE_WORDS, np.uint32)
        r = ExposureResult()
        self._check(self._L.rsrt_exposure_download(self._ctx, C.byref(p), _p(hist), hist.size, C.byref(r)), "rsrt_exposure_download")
        return hist, {"exposure": r.exposure, "target": r.target, "average_luminance": r.average_luminance, "metered": r.metered,
                      "skipped": r.skipped}

    def auto_exposure(self, source="mean", blend=1.0, **params):
        """Meters `source`, downloads with the remembered exposure as previous_exposure and remembers the new one (self.exposure):
        the first call takes the target, later ones move a fraction `blend` of the way to it.  Returns the result dict."""
        self.exposure_meter(source)
        _, r = self.exposure_download(blend=blend, previous_exposure=self.exposure or 0.0, **params)
        self.exposure = r["exposure"]
        return r

    def exposure_reset(self):
        """Forgets the remembered exposure and drops the histogram."""
        self.exposure = None
        self._check(self._L.rsrt_exposure_reset(self._ctx), "rsrt_exposure_reset")

    def display_exposed_srgb8(self, source="mean", exposure=None, sample_total=None):
        """rsrt_display_exposed_srgb8: `source` through the display pass at `exposure` (None: the remembered one; RsrtError with
        RSRT_ERR_NOT_READY if there is none): [H, W, 4] uint8, of the source's own size ("upsampled": the guide's; "lens", "motion": their source's)."""
        if exposure is None:
            if self.exposure is None:
                raise RsrtError("display_exposed_srgb8: no remembered exposure (auto_exposure first)", NOT_READY)
            exposure = self.exposure
        return self._displayed("rsrt_display_exposed_srgb8", source, sample_total, exposure)

    # -- bloom (include/rsrt.h "bloom") -----------------------------------------------------------------
    def _exposure_or_one(self, exposure):
        return (1.0 if self.exposure is None else self.exposure) if exposure is None else exposure

    def bloom(self, source="mean", exposure=None, levels=None, threshold=None, karis=True, sample_total=None, stream=None):
        """rsrt_bloom: builds the bloom image of `source` ("mean": the accumulator over sample_total, default sample_count;
        "denoised", "temporal", "upsampled", "lens": the last depth_of_field(), "motion": the last motion_blur()) at `exposure` (None: the remembered one, else 1) on the device.  levels, threshold:
        BLOOM_DEFAULTS otherwise; karis: the firefly weighting of the first downsample.  Asynchronous."""
        p = BloomParams(BLOOM_DEFAULTS["levels"] if levels is None else levels, BLOOM_KARIS if karis else 0,
                        BLOOM_DEFAULTS["threshold"] if threshold is None else threshold, 0.0)
        self._check(self._L.rsrt_bloom(self._ctx, *self._source_total(source, sample_total), self._exposure_or_one(exposure), C.byref(p),
                                       C.c_void_p(stream) if stream else None), "rsrt_bloom")

    def bloom_download(self):
        """rsrt_bloom_download: the bloom image of the last bloom(), [ceil(H / 2), ceil(W / 2), 4] float32, alpha 1."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check(self._L.rsrt_bloom_download(self._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_bloom_download")
        out = np.empty((h.value, w.value, 4), np.float32)
        self._check(self._L.rsrt_bloom_download(self._ctx, _p(out), out.size, None, None), "rsrt_bloom_download")
        return out

    def bloom_reset(self):
        """Drops the bloom image."""
        self._check(self._L.rsrt_bloom_reset(self._ctx), "rsrt_bloom_reset")

    def display_bloomed_srgb8(self, source="mean", exposure=None, intensity=None, sample_total=None):
        """rsrt_display_bloomed_srgb8: `source` through the display pass at `exposure` (None: the remembered one, else 1 — what
        bloom() took) with `intensity` (BLOOM_DEFAULTS otherwise) times the doubled bloom image added before the tone map:
        [H, W, 4] uint8, of the source's own size ("upsampled": the guide's; "lens", "motion": their source's)."""
        return self._displayed("rsrt_display_bloomed_srgb8", source, sample_total, self._exposure_or_one(exposure),
                               BLOOM_DEFAULTS["intensity"] if intensity is None else intensity)

    # -- local exposure (include/rsrt.h "local exposure") ---------------------------------------------------
    def local_exposure(self, source="mean", cell=None, sample_total=None, stream=None):
        """rsrt_local_exposure: builds the blurred bilateral grid of `source` ("mean": the accumulator over sample_total, default
        sample_count; "denoised", "temporal", "upsampled", "lens": the last depth_of_field(), "motion": the last motion_blur()) on the device, in cells of `cell` pixels (8, 16, 32 or 64; LOCAL_DEFAULTS
        otherwise).  The grid is of the unexposed image.  Asynchronous."""
        self._check(self._L.rsrt_local_exposure(self._ctx, *self._source_total(source, sample_total), LOCAL_DEFAULTS["cell"] if cell is None else cell,
                                                C.c_void_p(stream) if stream else None), "rsrt_local_exposure")

    def local_exposure_download(self):
        """rsrt_local_exposure_download: (the blurred grid of the last local_exposure(), [32, gy, gx, 2] uint32 — count, sum of q; its
        cell)."""
        dims = (C.c_uint32 * 4)()
        self._check(self._L.rsrt_local_exposure_download(self._ctx, None, 0, dims), "rsrt_local_exposure_download")
        out = np.empty((dims[2], dims[1], dims[0], 2), np.uint32)
        self._check(self._L.rsrt_local_exposure_download(self._ctx, _p(out), out.size, None), "rsrt_local_exposure_download")
        return out, int(dims[3])

    def local_exposure_reset(self):
        """Drops the grid."""
        self._check(self._L.rsrt_local_exposure_reset(self._ctx), "rsrt_local_exposure_reset")

    @staticmethod
    def _local_params(shadows, highlights, params):
        q = dict(LOCAL_DEFAULTS, **params)
        return LocalParams(q["shadows"] if shadows is None else shadows, q["highlights"] if highlights is None else highlights, q["key"],
                           q["max_stops"], q.get("flags", 0), 0)

    def _source_shape(self, source):
        """(H, W) of `source`: the guide's for "upsampled", what the library holds for "lens" and "motion", else the state's own."""
        source = ALL_SOURCES.get(source, source)
        if source == ALL_SOURCES["fog"] and self._fog_shape is not None:  # (the size of the source the last fog() composed)
            return self._fog_shape
        if source == DISPLAY_SOURCES["motion"]:
            w, h = C.c_uint32(), C.c_uint32()
            self._check(self._L.rsrt_motion_download(self._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_motion_download")
            return (h.value, w.value)
        if source == IMAGE_SOURCES["lens"]:
            w, h = C.c_uint32(), C.c_uint32()
            self._check(self._L.rsrt_dof_download(self._ctx, None, 0, C.byref(w), C.byref(h)), "rsrt_dof_download")
            return (h.value, w.value)
        return (self.guide_height, self.guide_width) if source == IMAGE_SOURCES["upsampled"] else (self.height, self.width)

    def local_gain(self, source="mean", exposure=None, shadows=None, highlights=None, sample_total=None, **params):
        """rsrt_local_gain_download: the gain display_local_srgb8 multiplies every pixel of `source` by at `exposure` (None: the
        remembered one, else 1), [H, W] float32.  params: key, max_stops; LOCAL_DEFAULTS otherwise."""
        p = self._local_params(shadows, highlights, params)
        out = np.empty(self._source_shape(source), np.float32)
        self._check(self._L.rsrt_local_gain_download(self._ctx, *self._source_total(source, sample_total), self._exposure_or_one(exposure), C.byref(p),
                                                     _p(out), out.size), "rsrt_local_gain_download")
        return out

    def display_local_srgb8(self, source="mean", exposure=None, shadows=None, highlights=None, bloom_intensity=0.0, sample_total=None, **params):
        """rsrt_display_local_srgb8: `source` through the display pass at `exposure` (None: the remembered one, else 1) with the local
        gain of the last local_exposure() and, with bloom_intensity > 0, the last bloom() added before it: [H, W, 4] uint8, of the
        source's own size.  shadows, highlights and params (key, max_stops): LOCAL_DEFAULTS otherwise."""
        p = self._local_params(shadows, highlights, params)
        return self._displayed("rsrt_display_local_srgb8", source, sample_total, self._exposure_or_one(exposure), C.byref(p), bloom_intensity)

    # -- white balance and colour grading (include/rsrt.h "white balance and colour grading") ---------------
    def white_meter(self, source="mean", sample_total=None, stream=None):
        """rsrt_white_meter: builds the chroma histogram of `source` ("mean": the accumulator over sample_total, default sample_count;
        "denoised", "temporal", "upsampled", "lens", "motion") on the device.  Asynchronous."""
        self._check(self._L.rsrt_white_meter(self._ctx, *self._source_total(source, sample_total), C.c_void_p(stream) if stream else None), "rsrt_white_meter")

    def white_download(self, **params):
        """rsrt_white_download of the last white_meter(): (histogram, 4097 uint32: 64 x 64 bins, v-major, and the skipped pixels; result
        dict with white, target, illuminant (3 floats each), eu, ev, gated, counted, skipped, estimated).  params: rsrt_white_params
        fields, WHITE_DEFAULTS otherwise."""
        q = dict(WHITE_DEFAULTS, **params)
        p = WhiteParams(q["gate"], q["iterations"], q["min_permille"], q["strength"], q["max_stops"], q["blend"], (C.c_float * 3)(*q["previous"]),
                        q.get("flags", 0))
        hist = np.zeros(WHITE_WORDS, np.uint32)
        r = WhiteResult()
        self._check(self._L.rsrt_white_download(self._ctx, C.byref(p), _p(hist), hist.size, C.byref(r)), "rsrt_white_download")
        return hist, {"white": tuple(r.white), "target": tuple(r.target), "illuminant": tuple(r.illuminant), "eu": r.eu, "ev": r.ev, "gated": r.gated,
                      "counted": r.counted, "skipped": r.skipped, "estimated": bool(r.estimated)}

    def auto_white_balance(self, source="mean", blend=1.0, **params):
        """Meters `source`, downloads with the remembered white point as `previous` and remembers the new one (self.white): the first
        call takes the target, later ones move a fraction `blend` of the way to it.  Returns the result dict."""
        self.white_meter(source)
        _, r = self.white_download(blend=blend, previous=self.white or (0.0, 0.0, 0.0), **params)
        self.white = r["white"]
        return r

    def white_reset(self):
        """Forgets the remembered white point and drops the histogram."""
        self.white = None
        self._check(self._L.rsrt_white_reset(self._ctx), "rsrt_white_reset")

    def colour_lut(self, slope=None, offset=None, power=None, saturation=None, size=33, stream=None):
        """rsrt_colour_lut_build: bakes the ASC CDL (slope, offset, power: one number or three; saturation; CDL_DEFAULTS otherwise) into
        a size^3 LUT on the device.  Asynchronous."""
        p = CdlParams.of(slope, offset, power, saturation)
        self._check(self._L.rsrt_colour_lut_build(self._ctx, size, C.byref(p), C.c_void_p(stream) if stream else None), "rsrt_colour_lut_build")

    def colour_lut_upload(self, nodes):
        """rsrt_colour_lut_upload: nodes [n, n, n, 3] float32 (blue, green, red index; encoded rgb in [0, 1])."""
        nodes = np.ascontiguousarray(nodes, np.float32)
        self._check(self._L.rsrt_colour_lut_upload(self._ctx, nodes.shape[0] if nodes.ndim else 0, _p(nodes), nodes.size), "rsrt_colour_lut_upload")

    def colour_lut_download(self):
        """rsrt_colour_lut_download: the LUT, [n, n, n, 3] float32 (blue, green, red index)."""
        n = C.c_uint32()
        self._check(self._L.rsrt_colour_lut_download(self._ctx, None, 0, C.byref(n)), "rsrt_colour_lut_download")
        out = np.empty((n.value, n.value, n.value, 3), np.float32)
        self._check(self._L.rsrt_colour_lut_download(self._ctx, _p(out), out.size, None), "rsrt_colour_lut_download")
        return out

    def colour_lut_reset(self):
        """Drops the LUT."""
        self._check(self._L.rsrt_colour_lut_reset(self._ctx), "rsrt_colour_lut_reset")

    def _has_colour_lut(self):
        return self._L.rsrt_colour_lut_download(self._ctx, None, 0, None) == 0

    def display_colour_srgb8(self, source="mean", exposure=None, white=None, lut_strength=None, shadows=None, highlights=None, bloom_intensity=0.0,
                             sample_total=None, **params):
        """rsrt_display_colour_srgb8: `source` through the display pass at `exposure` (None: the remembered one, else 1) with `white`
        (None: the remembered white point, else (1, 1, 1)) multiplied in before the tone map and the LUT behind it at `lut_strength`
        (None: 1 with a LUT, 0 without).  shadows, highlights: both None for no local grade, otherwise the last local_exposure()'s gain
        with them (LOCAL_DEFAULTS for the one left None; params: key, max_stops); bloom_intensity > 0 adds the last bloom().
        [H, W, 4] uint8, of the source's own size."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        c = self._colour_params(white, lut_strength)
        return self._displayed("rsrt_display_colour_srgb8", source, sample_total, self._exposure_or_one(exposure),
                               C.byref(local) if local is not None else None, bloom_intensity, C.byref(c))

    # -- finished display (include/rsrt.h "finished display") -----------------------------------------------
    def display_finished_srgb8(self, source="mean", exposure=None, white=None, lut_strength=None, shadows=None, highlights=None, bloom_intensity=0.0,
                               sharpness=None, grain=None, dither=None, seed=None, noise_aware=False, sample_total=None, **params):
        """rsrt_display_finished_srgb8: display_colour_srgb8 (whose arguments `source` .. `bloom_intensity`, sample_total and params are)
        with the sharpener at `sharpness`, film grain at `grain` and the dithered quantiser at `dither` behind the LUT (None:
        FINISH_DEFAULTS), the noise seeded with `seed` (pass a frame index for grain that moves; the same seed gives the same bytes; an integer
        of any size or sign, of which the low 32 bits are used);
        noise_aware: the sharpener's limiter (FINISH_NOISE_AWARE).  [H, W, 4] uint8, of the source's own size."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        c = self._colour_params(white, lut_strength)
        d = FINISH_DEFAULTS
        f = FinishParams(d["sharpness"] if sharpness is None else sharpness, d["grain"] if grain is None else grain, d["dither"] if dither is None else dither,
                         (d["seed"] if seed is None else int(seed)) & 0xFFFFFFFF, d["flags"] | (FINISH_NOISE_AWARE if noise_aware else 0), (C.c_uint32 * 3)())
        return self._displayed("rsrt_display_finished_srgb8", source, sample_total, self._exposure_or_one(exposure),
                               C.byref(local) if local is not None else None, bloom_intensity, C.byref(c), C.byref(f))

    # -- HDR display (include/rsrt.h "HDR display") ----------------------------------------------------------
    def display_hdr(self, source="mean", exposure=None, white=None, shadows=None, highlights=None, bloom_intensity=0.0, paper_white=None, peak=None,
                    knee=None, encoding="pq10", dither=None, seed=None, levels=False, sample_total=None, **params):
        """rsrt_display_hdr: display_colour_srgb8's chain up to its tone map (whose arguments `source` .. `bloom_intensity`, sample_total and
        params are; there is no LUT here) brought under `peak` cd/m^2 by a hue-preserving shoulder that begins at `knee` of it, with a
        linear 1.0 at `paper_white` cd/m^2 (None: HDR_DEFAULTS), and encoded for an HDR surface.  encoding "pq10": [H, W] uint32, Rec.2020
        PQ codes packed R | G << 10 | B << 20 | 3 << 30 (hdr_unpack_pq10 takes them apart), dithered at `dither` with the noise of `seed`
        (an integer of any size or sign, of which the low 32 bits are used); "scrgb16f": [H, W, 4] float16, linear Rec.709, 1.0 = 80
        cd/m^2, alpha 1.  Of the source's own size.  levels=True: (image, {"max_cll", "max_fall" in cd/m^2, "max_q", "sum_q"}), the
        frame's CTA-861.3 content light levels."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        c = self._colour_params(white, 0.0)
        d = HDR_DEFAULTS
        enc = HDR_ENCODINGS.get(encoding, encoding)
        p = HdrParams(d["paper_white"] if paper_white is None else paper_white, d["peak"] if peak is None else peak, d["knee"] if knee is None else knee,
                      d["dither"] if dither is None else dither, (d["seed"] if seed is None else int(seed)) & 0xFFFFFFFF, enc, d["flags"], 0)
        shape = self._source_shape(source)
        out = np.empty(shape + (4,), np.uint16) if enc == HDR_SCRGB16F else np.empty(shape, np.uint32)
        lv = HdrLevels()
        self._check(self._L.rsrt_display_hdr(self._ctx, *self._source_total(source, sample_total), self._exposure_or_one(exposure),
                                             C.byref(local) if local is not None else None, bloom_intensity, C.byref(c), C.byref(p), _p(out), out.nbytes,
                                             C.byref(lv) if levels else None), "rsrt_display_hdr")
        img = out.view(np.float16) if enc == HDR_SCRGB16F else out
        return (img, {"max_cll": lv.max_cll, "max_fall": lv.max_fall, "max_q": lv.max_q, "sum_q": lv.sum_q}) if levels else img

    # -- video output (include/rsrt.h "video output") --------------------------------------------------------
    def display_video(self, source="mean", exposure=None, white=None, lut_strength=None, shadows=None, highlights=None, bloom_intensity=0.0,
                      standard="bt709", depth=None, layout=None, range=None, siting=None, dither=None, seed=None, paper_white=None, peak=None, knee=None,
                      levels=False, sample_total=None, **params):
        """rsrt_display_video: `source` as a Y'CbCr 4:2:0 frame.  standard "bt709": display_colour_srgb8's chain (whose arguments `source`
        .. `bloom_intensity`, sample_total and params are) with the LUT, under the sRGB transfer and the BT.709 matrix; "hdr10":
        display_hdr's (paper_white, peak, knee: HDR_DEFAULTS where None; no LUT: lut_strength must be None or 0) as Rec.2020 PQ under the
        BT.2020 matrix, 10 bits only.  layout "nv12", "i420" (8 bits), "p010", "i420p10" (10 bits) or a VIDEO_* enumerator with `depth`
        (None: the layout's, else VIDEO_DEFAULTS'; hdr10's default layout is "p010"); range "limited" or "full"; siting "left", "centre"
        or "topleft"; the quantiser dithered at `dither` with the noise of `seed` (an integer of any size or sign, of which the low 32
        bits are used).  Returns a VideoFrame; levels=True (hdr10): (frame, display_hdr's levels dict)."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        d = VIDEO_DEFAULTS
        std = VIDEO_STANDARDS.get(standard, standard)
        if layout is None:
            layout = "p010" if std == VIDEO_HDR10 and depth in (None, 10) else VIDEO_LAYOUTS[d["layout"]][0]
        lay, lay_depth = VIDEO_LAYOUTS.get(layout, (layout, None))
        if depth is None:
            depth = d["depth"] if lay_depth is None else lay_depth
        elif lay_depth is not None and depth != lay_depth:
            raise ValueError("display_video: layout %r is %d bits a sample, not %d" % (layout, lay_depth, depth))
        v = VideoParams(std, depth, lay, VIDEO_RANGES.get(d["range"] if range is None else range, range), VIDEO_SITINGS.get(d["siting"] if siting is None else siting, siting),
                        d["dither"] if dither is None else dither, (d["seed"] if seed is None else int(seed)) & 0xFFFFFFFF, d["flags"])
        hdr10 = std == VIDEO_HDR10
        c = self._colour_params(white, 0.0 if hdr10 and lut_strength is None else lut_strength)
        h = HDR_DEFAULTS
        hp = HdrParams(h["paper_white"] if paper_white is None else paper_white, h["peak"] if peak is None else peak, h["knee"] if knee is None else knee,
                       0.0, 0, HDR_PQ10, 0, 0) if hdr10 else None
        if not hdr10 and not (paper_white is None and peak is None and knee is None):
            raise ValueError("display_video: paper_white, peak and knee belong to standard \"hdr10\"")
        height, width = self._source_shape(source)
        try:
            n = video_planes(width, height, depth, lay)[0]
        except ValueError:
            n = 1  # (the library names what is wrong)
        out = np.empty(n, np.uint8)
        lv = HdrLevels()
        self._check(self._L.rsrt_display_video(self._ctx, *self._source_total(source, sample_total), self._exposure_or_one(exposure),
                                               C.byref(local) if local is not None else None, bloom_intensity, C.byref(c), C.byref(hp) if hp is not None else None,
                                               C.byref(v), _p(out), out.nbytes, C.byref(lv) if levels else None), "rsrt_display_video")
        frame = VideoFrame(out, width, height, v)
        return (frame, {"max_cll": lv.max_cll, "max_fall": lv.max_fall, "max_q": lv.max_q, "sum_q": lv.sum_q}) if levels else frame

    # -- JPEG output (include/rsrt.h "JPEG output") ----------------------------------------------------------
    def _jpeg_file(self, what, call, guess, limit):
        """call(buffer, capacity, byref(n)) into a buffer of `guess` bytes, once more with the size the library asks for (at most
        `limit`, which always suffices); the file's bytes."""
        n = C.c_size_t(0)
        out = np.empty(max(1, min(guess, limit)), np.uint8)
        rc = call(_p(out), out.nbytes, C.byref(n))
        if rc != 0 and out.nbytes < n.value <= limit:  # (refused for the room alone: n is the size needed)
            out = np.empty(n.value, np.uint8)
            rc = call(_p(out), out.nbytes, C.byref(n))
        self._check(rc, what)
        return out[:n.value].tobytes()

    def display_jpeg(self, source="mean", exposure=None, white=None, lut_strength=None, shadows=None, highlights=None, bloom_intensity=0.0,
                     quality=None, subsampling=None, sample_total=None, **params):
        """rsrt_display_jpeg: `source` as a complete baseline JPEG / JFIF file, coded on the device: display_colour_srgb8's chain (whose
        arguments `source` .. `bloom_intensity`, sample_total and params are) with the LUT, then JFIF's Y'CbCr at `subsampling` ("420":
        4:2:0, centre-sited; "444") and `quality` 1 .. 100 on the IJG scale (JPEG_DEFAULTS where None).  The buffer is sized from a guess,
        an eighth of the worst case, and the call is made once more with the size the library asks for.  bytes."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        c = self._colour_params(white, lut_strength)
        j = jpeg_params(quality, subsampling)
        height, width = self._source_shape(source)
        limit = jpeg_max_bytes(width, height, j.subsampling) or 1
        st = self._source_total(source, sample_total)
        ex = self._exposure_or_one(exposure)
        return self._jpeg_file("rsrt_display_jpeg", lambda out, cap, n: self._L.rsrt_display_jpeg(
            self._ctx, *st, ex, C.byref(local) if local is not None else None, bloom_intensity, C.byref(c), C.byref(j), out, cap, n), JPEG_HEADER_BYTES + 2 + limit // 8, limit)

    def jpeg_coefficients(self, source="mean", exposure=None, white=None, lut_strength=None, shadows=None, highlights=None, bloom_intensity=0.0,
                          quality=None, subsampling=None, sample_total=None, **params):
        """rsrt_display_jpeg_coefficients: display_jpeg's first stage alone, the quantised DCT coefficients: int16 [blocks, 64], zigzag
        order, blocks in scan order (MCUs row by row; Y00 Y01 Y10 Y11 Cb Cr, or Y Cb Cr at "444"), the DC as it is."""
        local = None if shadows is None and highlights is None else self._local_params(shadows, highlights, params)
        c = self._colour_params(white, lut_strength)
        j = jpeg_params(quality, subsampling)
        height, width = self._source_shape(source)
        out = np.empty((max(1, jpeg_blocks(width, height, j.subsampling)), 64), np.int16)
        self._check(self._L.rsrt_display_jpeg_coefficients(self._ctx, *self._source_total(source, sample_total), self._exposure_or_one(exposure),
                                                           C.byref(local) if local is not None else None, bloom_intensity, C.byref(c), C.byref(j), _p(out), out.size),
                    "rsrt_display_jpeg_coefficients")
        return out

    def jpeg_encode(self, coefs, width, height, quality=None, subsampling=None):
        """rsrt_jpeg_encode_coefficients: the file that `quality`'s tables and the coefficients `coefs` (jpeg_coefficients' layout, any
        shape of 64 * blocks int16) of a width x height picture make: the scan and the packer on the device.  bytes."""
        j = jpeg_params(quality, subsampling)
        coefs = np.ascontiguousarray(coefs, np.int16)
        limit = jpeg_max_bytes(width, height, j.subsampling) or 1
        return self._jpeg_file("rsrt_jpeg_encode_coefficients", lambda out, cap, n: self._L.rsrt_jpeg_encode_coefficients(
            self._ctx, width, height, C.byref(j), _p(coefs), coefs.size, out, cap, n), JPEG_HEADER_BYTES + 2 + limit // 8, limit)

    # -- depth of field (include/rsrt.h "depth of field") ---------------------------------------------------
    def depth_of_field(self, source="mean", focus_distance=None, aperture=None, max_radius=None, sample_total=None, stream=None, out_ptr=None):
        """rsrt_dof: builds the lens image of `source` ("mean": the accumulator over sample_total, default sample_count; "denoised",
        "temporal": with the AOV buffer; "upsampled": with the guide) seen through the state's camera, on the device (in out_ptr when
        given).  focus_distance None: the one focus_at() remembered, else DOF_DEFAULTS'; aperture (the blur radius of a point at
        infinity as a fraction of the picture's height) and max_radius (1 .. 16 pixels): DOF_DEFAULTS otherwise.  The later passes take
        the result as their source "lens".  Asynchronous."""
        d = DOF_DEFAULTS
        if focus_distance is None:
            focus_distance = d["focus_distance"] if self.focus_distance is None else self.focus_distance
        p = DofParams(focus_distance, d["aperture"] if aperture is None else aperture, d["max_radius"] if max_radius is None else max_radius, 0)
        self._check(self._L.rsrt_dof(self._ctx, *self._source_total(source, sample_total), _p(self.camera), C.byref(p), C.c_void_p(out_ptr) if out_ptr else None,
                                     C.c_void_p(stream) if stream else None), "rsrt_dof")

    def dof_download(self):
        """rsrt_dof_download: the lens image of the last depth_of_field(), [H, W, 4] float32 of its source's size, alpha 1."""
        out = np.empty(self._source_shape("lens") + (4,), np.float32)
        self._check(self._L.rsrt_dof_download(self._ctx, _p(out), out.size, None, None), "rsrt_dof_download")
        return out

    def dof_coc(self):
        """rsrt_dof_coc_download: the signed blur radii of the last depth_of_field() in pixels, [H, W] float32 (negative: near field)."""
        out = np.empty(self._source_shape("lens"), np.float32)
        self._check(self._L.rsrt_dof_coc_download(self._ctx, _p(out), out.size), "rsrt_dof_coc_download")
        return out

    def focus_at(self, x, y, source="mean"):
        """Autofocus (rsrt_dof_depth_at): the depth along the optical axis at pixel (x, y) of `source`'s records, remembered as the focus
        distance of later depth_of_field() calls.  A sky pixel returns inf and leaves the focus as it was."""
        z = C.c_float()
        self._check(self._L.rsrt_dof_depth_at(self._ctx, ALL_SOURCES.get(source, source), _p(self.camera), x, y, C.byref(z)), "rsrt_dof_depth_at")
        if np.isfinite(z.value) and z.value > 0:
            self.focus_distance = z.value
        return z.value

    def dof_reset(self):
        """Drops the lens image (the remembered focus distance stays)."""
        self._check(self._L.rsrt_dof_reset(self._ctx), "rsrt_dof_reset")

    # -- camera motion blur (include/rsrt.h "camera motion blur") -------------------------------------------
    def motion_blur(self, source="mean", previous=None, shutter=None, max_radius=None, taps=None, sample_total=None, out_ptr=None, stream=None):
        """rsrt_motion_blur: builds the motion image of `source` ("mean": the accumulator over sample_total, default sample_count;
        "denoised", "temporal": with the AOV buffer; "upsampled": with the guide; "lens": with the records the lens image was built
        from) seen through the state's camera after `previous` (an rsrt_camera record: the camera one frame earlier), on the device (in
        out_ptr when given).  previous None: the camera of this state's last motion_blur(); on the first call, or after
        motion_reset(), the current camera, and the output is the source.  Every call remembers its camera afterwards.  shutter (the
        fraction of the frame interval the shutter is open), max_radius (1 .. 16 pixels) and taps (even, 2 .. 32): MOTION_DEFAULTS
        otherwise.  The later passes take the result as their source "motion".  Asynchronous."""
        d = MOTION_DEFAULTS
        p = MotionParams(d["shutter"] if shutter is None else shutter, d["max_radius"] if max_radius is None else max_radius,
                         d["taps"] if taps is None else taps, 0)
        if previous is None:
            previous = self.camera if self.motion_camera is None else self.motion_camera
        previous = np.ascontiguousarray(previous)
        self._check(self._L.rsrt_motion_blur(self._ctx, *self._source_total(source, sample_total), _p(self.camera), _p(previous), C.byref(p),
                                             C.c_void_p(out_ptr) if out_ptr else None, C.c_void_p(stream) if stream else None), "rsrt_motion_blur")
        self.motion_camera = self.camera.copy()

    def motion_download(self):
        """rsrt_motion_download: the motion image of the last motion_blur(), [H, W, 4] float32 of its source's size, alpha 1."""
        out = np.empty(self._source_shape("motion") + (4,), np.float32)
        self._check(self._L.rsrt_motion_download(self._ctx, _p(out), out.size, None, None), "rsrt_motion_download")
        return out

    def motion_velocity(self):
        """rsrt_motion_velocity_download: the velocities of the last motion_blur() in pixels, [H, W, 3] float32 (ux, uy, l)."""
        out = np.empty(self._source_shape("motion") + (3,), np.float32)
        self._check(self._L.rsrt_motion_velocity_download(self._ctx, _p(out), out.size), "rsrt_motion_velocity_download")
        return out

    def motion_tiles(self):
        """rsrt_motion_tiles_download: every 16 x 16 tile's own maximum of the last motion_blur(), [tiles_y, tiles_x, 3] float32."""
        tx, ty = C.c_uint32(), C.c_uint32()
        self._check(self._L.rsrt_motion_tiles_download(self._ctx, None, 0, C.byref(tx), C.byref(ty)), "rsrt_motion_tiles_download")
        out = np.empty((ty.value, tx.value, 3), np.float32)
        self._check(self._L.rsrt_motion_tiles_download(self._ctx, _p(out), out.size, None, None), "rsrt_motion_tiles_download")
        return out

    def motion_reset(self):
        """Drops the motion image and forgets the remembered camera."""
        self.motion_camera = None
        self._check(self._L.rsrt_motion_reset(self._ctx), "rsrt_motion_reset")

    # -- volumetric fog (include/rsrt.h "volumetric fog") -----------------------------------------------------
    def render_fog(self, n=None, sample_begin=None, stream=None, size=None, **params):
        """rsrt_fog_render: adds the fog of n samples (default 1) from sample_begin (default fog_sample_count: progressive, like
        render_aov) of the state's camera to the fog records, of the state's size or of size = (width, height) — the guide's, for the fog
        of the upsampled image.  params: rsrt_fog_params fields (density, albedo, anisotropy,
        light_dir, light_irradiance, ambient, max_distance, steps, flags or jitter=bool), FOG_DEFAULTS otherwise; fog_light_from_sky
        gives light_dir and light_irradiance of a sky's sun.  With no params at all a later call takes the ones the records were
        rendered with.  Raw, like render_aov: no hash check; clear_fog() before a new camera or other parameters.  Asynchronous."""
        p = self.fog_params if (not params and self.fog_params is not None) else FogParams.of(**params)
        n = 1 if n is None else n
        w, h = (self.width, self.height) if size is None else size
        have = self.fog_sample_count if (self.fog_width, self.fog_height) == (w, h) else 0  # (records of another size are allocated zeroed)
        begin = have if sample_begin is None else sample_begin
        self._check(self._L.rsrt_fog_render(self._ctx, _p(self.camera), w, h, begin, n, C.byref(p),
                                            C.c_void_p(stream) if stream else None), "rsrt_fog_render")
        self.fog_width, self.fog_height = w, h
        self.fog_params = p
        self.fog_sample_count = have + n

    def bind_fog(self, device_ptr, width, height):
        """Use caller-owned device memory (W*H*4 f32) as the fog records (None: back to the library's, which the next render_fog allocates)."""
        self._check(self._L.rsrt_fog_bind(self._ctx, C.c_void_p(device_ptr) if device_ptr else None, width, height), "rsrt_fog_bind")
        if device_ptr:
            self.fog_width, self.fog_height, self._fog_bound = width, height, True
        elif self._fog_bound:  # (the library gave its own buffer up at the bind)
            self.fog_width, self.fog_height, self._fog_bound = 0, 0, False

    def clear_fog(self):
        """rsrt_fog_clear: zeroes the records; the remembered parameters go with them."""
        self._check(self._L.rsrt_fog_clear(self._ctx), "rsrt_fog_clear")
        self.fog_sample_count = 0
        self.fog_params = None

    def download_fog(self):
        """rsrt_fog_download: the records, [H, W, 4] float32 (inscatter sum rgb, transmittance sum)."""
        out = np.empty((self.fog_height, self.fog_width, FOG_FLOATS), np.float32)
        self._check(self._L.rsrt_fog_download(self._ctx, _p(out), out.size), "rsrt_fog_download")
        return out

    def fog(self, source="mean", out_ptr=None, stream=None, sample_total=None, fog_sample_total=None, upsample=False, record_sample_total=None):
        """rsrt_fog_apply: builds the fog image of `source` ("mean": the accumulator over sample_total, default sample_count;
        "denoised", "temporal", "upsampled") and the fog records (of fog_sample_total samples, default fog_sample_count), on the device
        (in out_ptr when given).  The later passes — depth_of_field, motion_blur, the meters, bloom, local exposure and the displays —
        take the result as their source "fog".  Asynchronous.
        upsample=True: rsrt_fog_apply_upsampled — the records are smaller than the source (render_fog(size=...), half the size say) and
        the fog image is rebuilt from them and the source's first-hit records (the guide for "upsampled", the AOV buffer otherwise; of
        record_sample_total samples, default guide_sample_count / aov_sample_count) with the remembered fog_params."""
        src, n = self._source_total(source, sample_total)
        nf = self.fog_sample_count if fog_sample_total is None else fog_sample_total
        out, on = C.c_void_p(out_ptr) if out_ptr else None, C.c_void_p(stream) if stream else None
        if upsample:
            if self.fog_params is None:
                raise RsrtError("fog(upsample=True): no fog parameters remembered (render_fog first)")
            nr = record_sample_total
            if nr is None:
                nr = self.guide_sample_count if src == ALL_SOURCES["upsampled"] else self.aov_sample_count
            self._check(self._L.rsrt_fog_apply_upsampled(self._ctx, src, n, nf, nr, C.byref(self.fog_params), out, on), "rsrt_fog_apply_upsampled")
        else:
            self._check(self._L.rsrt_fog_apply(self._ctx, src, n, nf, out, on), "rsrt_fog_apply")
        self._fog_shape = self._source_shape(src)

    def fog_download(self):
        """rsrt_fog_image_download: the fog image of the last fog(), [H, W, 4] float32 of its source's size, alpha 1."""
        out = np.empty((self._fog_shape or (self.height, self.width)) + (4,), np.float32)
        self._check(self._L.rsrt_fog_image_download(self._ctx, _p(out), out.size), "rsrt_fog_image_download")
        return out

    def fog_reset(self):
        """rsrt_fog_reset: drops the records and the fog image, and forgets the parameters."""
        self._check(self._L.rsrt_fog_reset(self._ctx), "rsrt_fog_reset")
        self.fog_sample_count = 0
        self.fog_params = None
        self.fog_width = self.fog_height = 0
        self._fog_bound = False
        self._fog_shape = None

    def fog_light_from_sky(self, slot=None, height=None, **sky_params):
        """rsrt_fog_light_from_sky on the host: {"light_dir": (x, y, z), "light_irradiance": (r, g, b)} of the sun of the procedural sky
        of `sky_params` (SKY_DEFAULTS otherwise) on a map of `height` rows (default: the height environment_sky gave `slot`, else the
        environment_index's, else 1024) — what render_fog(**...) takes."""
        from . import host
        if height is None:
            height = self._env_sizes.get(self.environment_index if slot is None else slot, (2048, 1024))[1]
        return host.fog_light_from_sky(height, **sky_params)

    # -- temporal pass (include/rsrt.h "temporal pass") ----------------------------------------------
    def render_temporal(self, n=1, max_history=None, depth_tolerance=None, normal_tolerance=None, stream=None, moments=False):
        """One displayed frame of an interactive view: clears the accumulator and the AOV buffer, renders samples [k, k + n) of the
        current camera with the AOV pass (k = temporal_sample_count: fresh random numbers every frame) and blends them with the
        reprojected history (rsrt_temporal_accumulate).  Afterwards sample_count = aov_sample_count = n, and a later render_samples
        starts clean.  The history is reset first when environment_index, max_bounces, flags or the size changed since the last frame.
        The result stays on the device: download_temporal, denoise(temporal=True).  moments=True keeps the luminance moments too
        (RSRT_TEMPORAL_MOMENTS: download_temporal_moments, denoise(temporal=True, variance=True)); toggling it resets the history."""
        key = (self.environment_index, self.max_bounces, self.flags, self.width, self.height, bool(moments))
        if key != self._temporal_key:
            self.temporal_reset()
            self._temporal_key = key
        self.clear()
        if self._has_aov:
            self.clear_aov()
        k = self.temporal_sample_count
        self.render_range(k, n, stream=stream)
        self.render_aov(k, n, stream=stream)
        d = TEMPORAL_DEFAULTS
        p = TemporalParams(d["max_history"] if max_history is None else max_history,
                           d["depth_tolerance"] if depth_tolerance is None else depth_tolerance,
                           d["normal_tolerance"] if normal_tolerance is None else normal_tolerance)
        self._check(self._L.rsrt_temporal_accumulate_ex(self._ctx, _p(self.camera), n, n, C.byref(p), TEMPORAL_MOMENTS if moments else 0,
                                                        C.c_void_p(stream) if stream else None), "rsrt_temporal_accumulate_ex")
        self.temporal_sample_count = k + n
        self.sample_count = n
        self._last_hash = None

    def temporal_reset(self):
        """Drops the history: the next render_temporal frame is a first frame, from sample 0."""
        self._check(self._L.rsrt_temporal_reset(self._ctx), "rsrt_temporal_reset")
        self.temporal_sample_count = 0

    def download_temporal(self):
        """The last temporal frame: [H, W, 4] float32 (colour, sample weight)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rsrt_temporal_download(self._ctx, _p(out), out.size), "rsrt_temporal_download")
        return out

    def download_temporal_moments(self):
        """The last temporal frame's luminance moments (render_temporal(moments=True)): [H, W, 4] float32 (mu1, mu2, frames, scale)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rsrt_temporal_moments_download(self._ctx, _p(out), out.size), "rsrt_temporal_moments_download")
        return out

    # -- results ---------------------------------------------------------------------------------
    def download(self):
        """cumulative_light_texture: [H, W, 4] float32 sums, alpha 1 where rendered."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rsrt_accumulator_download(self._ctx, _p(out), out.size), "rsrt_accumulator_download")
        return out

    def download_mean_f16(self, sample_total=None):
        """out_texture: [H, W, 4] float16 mean radiance."""
        out = np.empty((self.height, self.width, 4), np.float16)
        self._check(self._L.rsrt_resolve_mean_f16(self._ctx, self._total(sample_total), _p(out), out.size), "rsrt_resolve_mean_f16")
        return out

    def debug_view(self, dev_index, out_texture=None, sample_count=None, environment_index=None):
        """The reference's developer views (shader.wgsl:1314-1338) as out_texture, [H, W, 4] float16: dev_index 3 = the HDRI, 2 = draws
        of the alias table added onto `out_texture` (the previous frame's; zeros when None).  See rsrt_debug_view_f16."""
        out = np.zeros((self.height, self.width, 4), np.float16) if out_texture is None else np.ascontiguousarray(out_texture, np.float16).copy()
        assert out.shape == (self.height, self.width, 4)
        n = self.sample_count if sample_count is None else sample_count
        e = self.environment_index if environment_index is None else environment_index
        self._check(self._L.rsrt_debug_view_f16(self._ctx, dev_index, e, n, _p(out), out.size), "rsrt_debug_view_f16")
        return out

    def display_srgb8(self, sample_total=None):
        """What the reference shows on screen: [H, W, 4] uint8 (ACES tonemap of the f16 mean, sRGB encoded)."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rsrt_display_srgb8(self._ctx, self._total(sample_total), _p(out), out.size), "rsrt_display_srgb8")
        return out

    def stats(self):
        s = Stats()
        self._check(self._L.rsrt_get_stats(self._ctx, C.byref(s)), "rsrt_get_stats")
        return s.as_dict()

    def debug_counters(self):
        out = np.zeros(32, np.uint64)
        self._check(self._L.rsrt_get_debug_counters(self._ctx, _p(out)), "rsrt_get_debug_counters")
        return out

    def region_counters(self):
        """Lanes that passed each region mark since the last call (instrumented build; zeros in the product build)."""
        out = np.zeros(32, np.uint64)
        self._check(self._L.rsrt_get_region_counters(self._ctx, _p(out)), "rsrt_get_region_counters")
        return out

    def walk_counters(self):
        """The cooperative walk's counters since the context was created (rsrt_get_walk_counters): a dict of WALK_COUNTERS; 'peak' is a
        maximum, the others are sums.  The probe (cast_rays, traversal 6) counts all of them, a render only 'overflows'."""
        out = np.zeros(len(WALK_COUNTERS), np.uint64)
        self._check(self._L.rsrt_get_walk_counters(self._ctx, _p(out), len(out)), "rsrt_get_walk_counters")
        return {k: int(v) for k, v in zip(WALK_COUNTERS, out)}

    def selftest_numerics(self):
        """Exhaustive device check of the short reciprocal (all 2^32 inputs): dict of the four words of rsrt_selftest_numerics."""
        out = np.zeros(4, np.uint64)
        self._check(self._L.rsrt_selftest_numerics(self._ctx, _p(out)), "rsrt_selftest_numerics")
        return {"mismatches": int(out[0]), "short_path_inputs": int(out[1]), "bare_rcp_wrong": int(out[2]), "first_bad": int(out[3])}

    def selftest_sincos(self):
        """Exhaustive device check of rsrt_sincosf against rsrt_sinf / rsrt_cosf (all 2^32 inputs): dict of the words of rsrt_selftest_sincos."""
        out = np.zeros(4, np.uint64)
        self._check(self._L.rsrt_selftest_sincos(self._ctx, _p(out)), "rsrt_selftest_sincos")
        return {"mismatches": int(out[0]), "checked": int(out[1]), "first_bad": int(out[3])}

    def build_bvh_device(self, spheres, plane_descs, vertices, triangles):
        """build_bvh on the device (rsrt_build_bvh_device): (primitives, nodes, depth, device milliseconds) — the host
        builder's arrays, bit for bit."""
        sph, pls = np.ascontiguousarray(spheres).view(T.SPHERE).reshape(-1), np.ascontiguousarray(plane_descs).view(T.PLANE_DESC).reshape(-1)
        ver, tri = np.ascontiguousarray(vertices).view(T.VEC3).reshape(-1), np.ascontiguousarray(triangles).view(T.TRIANGLE).reshape(-1)
        n = len(sph) + len(pls) + len(tri)
        prims, nodes = np.zeros(max(n, 1), T.PRIMITIVE_INFO), np.zeros(max(2 * n, 1), T.BVH_NODE)
        n_nodes, depth, ms = C.c_uint32(0), C.c_uint32(0), C.c_double(0.0)
        self._check(self._L.rsrt_build_bvh_device(self._ctx, _p(sph), len(sph), _p(pls), len(pls), _p(ver), len(ver), _p(tri), len(tri), _p(prims), _p(nodes),
                                                  C.byref(n_nodes), C.byref(depth), C.byref(ms)), "rsrt_build_bvh_device")
        return prims[:n], nodes[:n_nodes.value].copy(), depth.value, ms.value

    def cast_rays(self, origins, directions, mode=0, flags=0):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        assert o.shape == d.shape
        out = np.zeros(len(o), T.HIT)
        self._check(self._L.rsrt_cast_rays(self._ctx, len(o), _p(o), _p(d), mode, flags, _p(out)), "rsrt_cast_rays")
        return out


class MultiState:
    """`State` over a LIST of devices of one node, driven by one thread (rsrt_multi_*, include/rsrt.h): device i renders
    the tiles of rank i (partition.py), the frame is gathered onto devices[0] by RCCL inside the library when it is asked for."""

    def __init__(self, scene, environments, width, height, devices=(0,), camera=None):
        self._L = lib()
        self._m = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = self._L.rsrt_multi_create(devs, len(devices), C.byref(self._m))
        if rc != 0:
            raise RsrtError("rsrt_multi_create failed (%d): %s" % (rc, self._L.rsrt_multi_last_error(None).decode()))
        a = [scene.materials, scene.spheres, scene.planes, scene.vertices, scene.normals, scene.triangles, scene.primitives, scene.bvh_nodes]
        args = []
        for arr in a:
            arr = np.ascontiguousarray(arr)
            args += [_p(arr), len(arr)]
        self._check(self._L.rsrt_multi_upload_scene(self._m, *args), "rsrt_multi_upload_scene")
        for i, env in enumerate(environments if isinstance(environments, (list, tuple)) else [environments]):
            rgba, alias = np.ascontiguousarray(env.rgba, dtype=np.float32), np.ascontiguousarray(env.alias)
            self._check(self._L.rsrt_multi_upload_environment(self._m, i, env.width, env.height, _p(rgba), _p(alias)), "rsrt_multi_upload_environment")
        self._check(self._L.rsrt_multi_resize(self._m, width, height), "rsrt_multi_resize")
        self.width, self.height = width, height
        self.camera = np.array(camera if camera is not None else scene.camera_uniform()).view(T.CAMERA).reshape(1).copy()
        self.max_bounces, self.environment_index, self.flags, self.sample_count = 10, 0, 0, 0

    def _check(self, rc, what):
        if rc != 0:
            raise RsrtError("%s failed (%d): %s" % (what, rc, self._L.rsrt_multi_last_error(self._m).decode()))

    def close(self):
        if self._m:
            self._L.rsrt_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def size(self):
        return self._L.rsrt_multi_size(self._m)

    def uses_rccl(self):
        return bool(self._L.rsrt_multi_uses_rccl(self._m))

    def clear(self):
        self._check(self._L.rsrt_multi_clear(self._m), "rsrt_multi_clear")
        self.sample_count = 0

    def render_samples(self, n):
        self._check(self._L.rsrt_multi_render(self._m, _p(self.camera), self.width, self.height, self.sample_count, n, self.max_bounces,
                                              self.environment_index, self.flags), "rsrt_multi_render")
        self.sample_count += n

    def download(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.rsrt_multi_download(self._m, _p(out), out.size), "rsrt_multi_download")
        return out

    def display_srgb8(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(self._L.rsrt_multi_display_srgb8(self._m, self.sample_count, _p(out), out.size), "rsrt_multi_display_srgb8")
        return out

    def stats(self):
        s = Stats()
        self._check(self._L.rsrt_multi_get_stats(self._m, C.byref(s)), "rsrt_multi_get_stats")
        return s.as_dict()
