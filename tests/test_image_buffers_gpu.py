"""The image-space passes' buffers on one context: who owns them, which size they follow, what drops them (the table in the
section on the context).  The per-pass suites hold each pass's image against its reference; this one holds what the passes share —
the refusals of an empty context word for word, the derived images across a resize to the same size, to the same pixel count in
another shape and to no accumulator at all, and the AOV buffer and the guide through owned -> bound -> unbound.

Accumulator 16x8, guide 32x16, noise tile 16x4 (64 pixels: the smallest legal tile), one sample a pass."""
import torch  # (before librsrt is loaded: the library then shares torch's HIP runtime)

import collections
import ctypes as C
import re

import numpy as np
import pytest

import lifecycle_cases as L
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import state as S

pytestmark = pytest.mark.gpu

OK = 0
W, H = 16, 8
GW, GH = 32, 16
TILE = (16, 4)
ENV = "tiny"

NO_ACC = "no accumulator"
NO_SCENE = "no scene uploaded"
NO_AOV = "no AOV buffer"
NO_GUIDE = "no guide buffer"
NO_DENOISED = "no denoised image (rsrt_denoise first)"
NO_TEMPORAL = "no temporal frame since the last reset (rsrt_temporal_accumulate first)"
NO_MOMENTS = "the last temporal frame carried no moments (rsrt_temporal_accumulate_ex with RSRT_TEMPORAL_MOMENTS first)"
NO_UPSAMPLED = "no upsampled image (rsrt_upsample first)"
NO_ESTIMATE = "no noise estimate (rsrt_noise_estimate first)"
NO_SNAPSHOT = "noise_estimate: no snapshot of this accumulator (rsrt_noise_snapshot first)"
NO_HISTOGRAM = "no exposure histogram (rsrt_exposure_meter first)"


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def outcome(call):
    """(status, the library's error text) of a State call; (0, None) when it went through."""
    try:
        call()
    except R.RsrtError as e:
        return e.status, str(e).split("): ", 1)[1]
    return OK, None


def refused(call, status, text):
    assert outcome(call) == (status, text)


def new_state(w=W, h=H):
    st = R.State.new(L.scene("default"), L.env(ENV), w, h)
    st.max_bounces = L.MB
    return st


# the downloads the State wrapper only offers fused with their pass, or sized by the state's own idea of the size
def floats(st, fn, shape):
    out = np.empty(shape, np.float32)
    st._check(getattr(st._L, fn)(st._ctx, S._p(out), out.size), fn)
    return out


def denoised(st, w, h):
    return floats(st, "rsrt_denoised_download", (h, w, 4))


def upsampled(st):
    return floats(st, "rsrt_upsampled_download", (GH, GW, 4))


def temporal_ex(st, moments):
    p = S.TemporalParams(32, 0.05, 0.9)
    fn = "rsrt_temporal_accumulate_ex" if moments is not None else "rsrt_temporal_accumulate"
    args = (st._ctx, S._p(st.camera), 1, 1, C.byref(p)) + ((moments,) if moments is not None else ()) + (None,)
    st._check(getattr(st._L, fn)(*args), fn)


# ---------------------------------------------------------------------------------------------------- a: an empty context
# (status, text) of every image-space entry point on a context that has a camera and nothing else: no scene, no environment, no
# accumulator.  The texts are those of the library's source.
EMPTY = [
    # aov
    ("render_aov", lambda st: st.render_aov(0, 1), L.NOT_READY, NO_SCENE),
    ("bind_aov(None)", lambda st: st.bind_aov(None, 0, 0), OK, None),
    ("clear_aov", lambda st: st.clear_aov(), L.NOT_READY, NO_AOV),
    ("download_aov", lambda st: st.download_aov(), L.NOT_READY, NO_AOV),
    # guide
    ("render_guide", lambda st: st.render_guide(GW, GH, 0, 1), L.NOT_READY, NO_SCENE),
    ("bind_guide(None)", lambda st: st.bind_guide(None, 0, 0), OK, None),
    ("clear_guide", lambda st: st.clear_guide(), L.NOT_READY, NO_GUIDE),
    ("download_guide", lambda st: st.download_guide(), L.NOT_READY, NO_GUIDE),
    # denoise
    ("denoise", lambda st: st.denoise(sample_total=1, aov_sample_total=1), L.NOT_READY, NO_ACC),
    ("denoised_download", lambda st: denoised(st, 0, 0), L.NOT_READY, NO_DENOISED),
    ("denoised_display_srgb8", lambda st: st.denoised_display_srgb8(), L.NOT_READY, NO_DENOISED),
    # temporal
    ("temporal_accumulate", lambda st: temporal_ex(st, None), L.NOT_READY, NO_ACC),
    ("temporal_accumulate_ex", lambda st: temporal_ex(st, S.TEMPORAL_MOMENTS), L.NOT_READY, NO_ACC),
    ("temporal_accumulate_ex(flags 2)", lambda st: temporal_ex(st, 2), L.INVALID, "temporal: unknown flags 0x2"),
    ("temporal_reset", lambda st: st.temporal_reset(), OK, None),
    ("download_temporal", lambda st: st.download_temporal(), L.NOT_READY, NO_TEMPORAL),
    ("download_temporal_moments", lambda st: st.download_temporal_moments(), L.NOT_READY, NO_MOMENTS),
    # upsample
    ("upsample", lambda st: st.upsample(sample_total=1, aov_sample_total=1, guide_sample_total=1), L.NOT_READY, NO_ACC),
    ("upsampled_download", lambda st: upsampled(st), L.NOT_READY, NO_UPSAMPLED),
    ("upsampled_display_srgb8", lambda st: st.upsampled_display_srgb8(), L.NOT_READY, NO_UPSAMPLED),
    # noise
    ("noise_snapshot(0)", lambda st: st.noise_snapshot(0), L.INVALID, "noise_snapshot: sample_total must be > 0"),
    ("noise_snapshot", lambda st: st.noise_snapshot(1), L.NOT_READY, NO_ACC),
    ("noise_estimate", lambda st: st.noise_estimate(TILE, sample_total=2), L.NOT_READY, NO_ACC),
    ("noise_estimate(10x10)", lambda st: st.noise_estimate((10, 10), sample_total=2), L.INVALID,
     "noise_estimate: tile 10x10: pixel count must be a multiple of 64 and at most 4096"),
    ("noise_download", lambda st: st.noise_download(), L.NOT_READY, NO_ESTIMATE),
    ("noise_reset", lambda st: st.noise_reset(), OK, None),
    # exposure
    ("exposure_meter(mean, 0)", lambda st: st.exposure_meter("mean", 0), L.INVALID, "exposure_meter: sample_total must be > 0"),
    ("exposure_meter(mean)", lambda st: st.exposure_meter("mean", 1), L.NOT_READY, NO_ACC),
    ("exposure_meter(denoised)", lambda st: st.exposure_meter("denoised", 1), L.NOT_READY, NO_DENOISED),
    ("exposure_meter(temporal)", lambda st: st.exposure_meter("temporal", 1), L.NOT_READY, NO_TEMPORAL),
    ("exposure_meter(upsampled)", lambda st: st.exposure_meter("upsampled", 1), L.NOT_READY, NO_UPSAMPLED),
    ("exposure_meter(9)", lambda st: st.exposure_meter(9, 1), L.INVALID, "exposure_meter: unknown source 9"),
    ("exposure_download", lambda st: st.exposure_download(), L.NOT_READY, NO_HISTOGRAM),
    ("exposure_reset", lambda st: st.exposure_reset(), OK, None),
    ("display_exposed(mean, 0)", lambda st: st.display_exposed_srgb8("mean", 1.0, 0), L.INVALID, "display_exposed_srgb8: sample_total must be > 0"),
    ("display_exposed(mean)", lambda st: st.display_exposed_srgb8("mean", 1.0, 1), L.NOT_READY, NO_ACC),
    ("display_exposed(denoised)", lambda st: st.display_exposed_srgb8("denoised", 1.0, 1), L.NOT_READY, NO_DENOISED),
    ("display_exposed(temporal)", lambda st: st.display_exposed_srgb8("temporal", 1.0, 1), L.NOT_READY, NO_TEMPORAL),
    ("display_exposed(upsampled)", lambda st: st.display_exposed_srgb8("upsampled", 1.0, 1), L.NOT_READY, NO_UPSAMPLED),
    ("display_exposed(9)", lambda st: st.display_exposed_srgb8(9, 1.0, 1), L.INVALID, "display_exposed_srgb8: unknown source 9"),
    # display / download of the accumulator
    ("bind_accumulator(None)", lambda st: st.bind_accumulator(None, 0, 0), OK, None),
    ("clear", lambda st: st.clear(), L.NOT_READY, NO_ACC),
    ("download", lambda st: st.download(), L.NOT_READY, NO_ACC),
    ("download_mean_f16", lambda st: st.download_mean_f16(1), L.NOT_READY, NO_ACC),
    ("debug_view", lambda st: st.debug_view(3), L.NOT_READY, NO_ACC),
    ("display_srgb8", lambda st: st.display_srgb8(1), L.NOT_READY, NO_ACC),
]


def test_empty_context():
    st = R.State(0)
    st.camera = L.camera(L.scene("default"))
    try:
        got = {name: outcome(lambda: call(st)) for name, call, _, _ in EMPTY}
    finally:
        st.close()
    assert got == {name: (status, text) for name, _, status, text in EMPTY}


# ---------------------------------------------------------------------------------------------------- b: every derived image
def derive(st, w, h, guide):
    """Every image derived from a w x h accumulator, from a state that may hold anything: a first temporal frame with moments (sample 0
    and its AOV records), its denoise, with `guide` the upsampled picture, a noise snapshot at 1 sample with the estimate at 2, and the
    histogram of the 2-sample mean."""
    st.temporal_reset()
    st._temporal_key = None
    st.render_temporal(1, moments=True)
    out = {"temporal": st.download_temporal(), "moments": st.download_temporal_moments()}
    out["denoised"] = st.denoise(sample_total=1, aov_sample_total=1)
    if guide:
        if st.guide_width:
            st.clear_guide()
        st.render_guide(GW, GH, 0, 1)
        out["upsampled"] = st.upsample("mean", sample_total=1, aov_sample_total=1, guide_sample_total=1)
    st.noise_snapshot(1)
    st.render_range(1, 1)  # (raw: no clear, which would drop the snapshot)
    out["noise"], out["noise_summary"] = st.noise_estimate(TILE, sample_total=2)
    st.exposure_meter("mean", 2)
    out["histogram"] = st.exposure_download()[0]
    assert (out["denoised"].shape, out["noise"].shape) == ((h, w, 4), (-(-h // TILE[1]), -(-w // TILE[0])))
    return out


def downloads(st, w, h):
    """... each fetched again, by the download calls alone."""
    tiles, summary = st.noise_download()
    return {"temporal": st.download_temporal(), "moments": st.download_temporal_moments(), "denoised": denoised(st, w, h), "upsampled": upsampled(st),
            "noise": tiles, "noise_summary": summary, "histogram": st.exposure_download()[0]}


def differing(a, b):
    """The names of the images that are not the same bit for bit."""
    assert a.keys() == b.keys()
    return [k for k in a if not (a[k] == b[k] if isinstance(a[k], dict) else same(a[k], b[k]))]


@pytest.fixture(scope="module")
def made():
    """(the context of parts b to d, what derive() returned on it while it was fresh)."""
    st = new_state()
    try:
        yield st, derive(st, W, H, guide=True)
    finally:
        st.close()


def test_derived_images_follow_the_accumulators_size(made):
    st, first = made
    assert first["temporal"][..., 3].any() and first["histogram"].sum() == W * H
    assert differing(downloads(st, W, H), first) == []  # b: each one is there
    st.resize(W, H)  # c: the size it has
    assert differing(downloads(st, W, H), first) == []
    st.resize(H, W)  # d: 8x16 — as many pixels, another shape
    refused(lambda: denoised(st, H, W), L.NOT_READY, NO_DENOISED)
    refused(st.download_temporal, L.NOT_READY, NO_TEMPORAL)
    refused(st.download_temporal_moments, L.NOT_READY, NO_MOMENTS)
    refused(st.noise_download, L.NOT_READY, NO_ESTIMATE)
    refused(lambda: st.noise_estimate(TILE, sample_total=2), L.NOT_READY, NO_SNAPSHOT)
    assert same(upsampled(st), first["upsampled"])  # (of the guide's size, in a buffer of its own)
    assert same(st.exposure_download()[0], first["histogram"])
    again = derive(st, H, W, guide=False)
    fresh = new_state(H, W)
    try:
        assert differing(again, derive(fresh, H, W, guide=False)) == []
    finally:
        fresh.close()
    assert not same(again["denoised"].reshape(-1), first["denoised"].reshape(-1))  # (8x16 is another picture, not 16x8 re-read)


# ---------------------------------------------------------------------------------------------------- e: AOV and guide ownership
Records = collections.namedtuple("Records", "size other render bind clear download none pointer misfit")


def _raw(st, fn, *args):
    st._check(getattr(st._L, fn)(st._ctx, *args), fn)


def _render(fn):
    return lambda st, w, h: _raw(st, fn, S._p(st.camera), w, h, 0, 1, 0, None)


def _bind(fn):
    return lambda st, ptr, w, h: _raw(st, fn, C.c_void_p(ptr) if ptr else None, w, h)


def _download(fn):
    return lambda st, w, h: floats(st, fn, (h, w, 8))


# `size`: what the library's own buffer has here (the AOV buffer follows the accumulator); `other`: the bound tensor's.  misfit: the
# refusal of a render that wants `size` while `other` is bound (its second half was worded in two ways until the buffers were unified)
RECORDS = {
    "aov": Records((W, H), (GW, GH), _render("rsrt_aov_render"), _bind("rsrt_aov_bind"), lambda st: _raw(st, "rsrt_aov_clear"), _download("rsrt_aov_download"),
                   NO_AOV, "AOV pointer must be 16-byte aligned", r"bound AOV buffer is 32x16 but (the accumulator is 16x8|16x8 was requested)"),
    "guide": Records((GW, GH), (24, 12), _render("rsrt_guide_render"), _bind("rsrt_guide_bind"), lambda st: _raw(st, "rsrt_guide_clear"),
                     _download("rsrt_guide_download"), NO_GUIDE, "guide pointer must be 16-byte aligned", r"bound guide buffer is 24x12 but 32x16 was requested"),
}


@pytest.mark.parametrize("which", sorted(RECORDS))
def test_record_buffer_ownership(which):
    """owned -> bound to a zeroed torch tensor of another size -> unbound, for the AOV buffer and the guide alike."""
    r = RECORDS[which]
    (w, h), (ow, oh) = r.size, r.other
    want = L.aov_reference("default", w, h, 0, 1)
    st = new_state()
    try:
        r.render(st, w, h)  # owned
        assert same(r.download(st, w, h), want)
        t = torch.zeros((oh, ow, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        refused(lambda: r.bind(st, t.data_ptr() + 4, ow, oh), L.INVALID, r.pointer)
        refused(lambda: r.bind(st, t.data_ptr(), 0, oh), L.INVALID, "bad resolution 0x%d" % oh)
        assert same(r.download(st, w, h), want)  # (a refused bind leaves the library's buffer in place)
        r.bind(st, t.data_ptr(), ow, oh)  # bound
        status, text = outcome(lambda: r.render(st, w, h))
        assert status == L.INVALID and re.fullmatch(r.misfit, text), text
        assert not r.download(st, ow, oh).any()
        t.fill_(1.0)
        torch.cuda.synchronize()
        assert (r.download(st, ow, oh) == 1.0).all()
        r.clear(st)
        st.synchronize()
        assert not t.cpu().numpy().any()
        r.bind(st, None, 0, 0)  # unbound: the library gave its own buffer up at the bind
        refused(lambda: r.clear(st), L.NOT_READY, r.none)
        refused(lambda: r.download(st, w, h), L.NOT_READY, r.none)
        r.render(st, w, h)  # ... and the next render allocates one, zeroed (the records are sums)
        assert same(r.download(st, w, h), want)
        assert not t.cpu().numpy().any()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- f: no accumulator
def test_unbinding_the_only_accumulator_drops_the_derived_images(made):
    """rsrt_accumulator_bind(NULL) on a context whose own accumulator was given up at the earlier bind leaves no accumulator: a change of
    its size like any other, which drops what was derived from it."""
    _, first = made
    st = new_state()
    try:
        t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st.bind_accumulator(t.data_ptr(), W, H)
        st.render_temporal(1)
        assert same(st.denoise(sample_total=1, aov_sample_total=1), first["denoised"])
        st.bind_accumulator(None, 0, 0)
        refused(st.denoised_display_srgb8, L.NOT_READY, NO_DENOISED)
        refused(lambda: st.exposure_meter("denoised"), L.NOT_READY, NO_DENOISED)
        refused(st.download_temporal, L.NOT_READY, NO_TEMPORAL)
        refused(lambda: st.display_srgb8(1), L.NOT_READY, NO_ACC)
        st.resize(W, H)
        st.render_range(0, 1)  # (the AOV buffer is the library's own and still holds sample 0's records)
        assert same(st.denoise(sample_total=1, aov_sample_total=1), first["denoised"])
    finally:
        st.close()
