"""What the display chain's entry points refuse, as one table of (call, status, exact text): rsrt_display_bloomed_srgb8,
rsrt_display_local_srgb8, rsrt_local_gain_download, rsrt_display_colour_srgb8, rsrt_display_finished_srgb8 and the two meters' downloads.
Every row is one call on one small context; the text is the library's own (rsrt_last_error), so the table pins the words, the status and —
in the rows with two faults at once — the order in which the checks are made.

The context has two sizes: an accumulator of 12 x 8 and a guide of 24 x 16 (rsrt_upsample wants the guide at least as large as the
accumulator), so that "upsampled" is a source of another size than "mean"."""
import ctypes as C

import numpy as np
import pytest

import rsoderh_raytracing_amd as R
from test_denoise_gpu import state
from test_finish import colour_params, finish_params

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = 1, 4
S = R.state
W, H, GW, GH = 12, 8, 24, 16
N = W * H
NAN, INF = float("nan"), float("inf")
MEAN, UPSAMPLED = 0, 3

LOCAL_TEXT = "%s: want shadows and highlights in [0, 1], key finite and > 0, max_stops in [0, 16], flags 0"
COLOUR_TEXT = "%s: want white finite and > 0, lut_strength in [0, 1], flags 0"
FINISH_TEXT = "%s: want sharpness, grain and dither in [0, 1], flags RSRT_FINISH_NOISE_AWARE or 0"
NO_GRID = "no local exposure grid (rsrt_local_exposure first)"
NO_BLOOM = "no bloom image (rsrt_bloom first)"
NO_LUT = "no colour LUT (rsrt_colour_lut_build or rsrt_colour_lut_upload first)"
GRID_SIZE = "%s: the grid was built for 24x16, the source is 12x8"
BLOOM_SIZE = "%s: the bloom image was built for 24x16, the source is 12x8"


def lp(shadows=0.5, highlights=0.5, key=0.18, max_stops=4.0, flags=0):
    return S.LocalParams(shadows, highlights, key, max_stops, flags, 0)


cp, fp = colour_params, finish_params
BYTES = np.zeros((H, W, 4), np.uint8)
GAINS = np.zeros((H, W), np.float32)
ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731


# one function an entry point; the defaults are a call that is accepted when the grid, the bloom image and the LUT are there
def bloomed(st, source=MEAN, n=2, e=1.5, i=0.5, nb=N * 4):
    return st._L.rsrt_display_bloomed_srgb8(st._ctx, source, n, e, i, S._p(BYTES), nb)


def local(st, source=MEAN, n=2, e=1.5, p=lp(), i=0.0, nb=N * 4):
    return st._L.rsrt_display_local_srgb8(st._ctx, source, n, e, ref(p), i, S._p(BYTES), nb)


def gain(st, source=MEAN, n=2, e=1.5, p=lp(), out=GAINS, nf=N):
    return st._L.rsrt_local_gain_download(st._ctx, source, n, e, ref(p), S._p(out), nf)


def colour(st, source=MEAN, n=2, e=1.5, p=None, i=0.0, c=cp(), nb=N * 4):
    return st._L.rsrt_display_colour_srgb8(st._ctx, source, n, e, ref(p), i, ref(c), S._p(BYTES), nb)


def finished(st, source=MEAN, n=2, e=1.5, p=None, i=0.0, c=cp(), f=fp(), nb=N * 4):
    return st._L.rsrt_display_finished_srgb8(st._ctx, source, n, e, ref(p), i, ref(c), ref(f), S._p(BYTES), nb)


def exposure_download(st, p=S.ExposureParams(100, 950, 0.18, 2.0 ** -16, 2.0 ** 16, 1.0, 0.0, 0), words=S.EXPOSURE_WORDS):
    hist = np.zeros(S.EXPOSURE_WORDS + 1, np.uint32)
    return st._L.rsrt_exposure_download(st._ctx, ref(p), S._p(hist), words, None)


def white_download(st, p=S.WhiteParams(12, 3, 50, 1.0, 2.0, 1.0, (C.c_float * 3)(), 0), words=S.WHITE_WORDS):
    hist = np.zeros(S.WHITE_WORDS + 1, np.uint32)
    return st._L.rsrt_white_download(st._ctx, ref(p), S._p(hist), words, None)


NAMES = {bloomed: "display_bloomed_srgb8", local: "display_local_srgb8", gain: "local_gain_download", colour: "display_colour_srgb8",
         finished: "display_finished_srgb8"}
ALL = (bloomed, local, gain, colour, finished)
TILED = (local, gain, colour, finished)
GRADED = (colour, finished)  # (their local params are optional)
BAD_LOCAL = [lp(shadows=-0.1), lp(highlights=1.5), lp(key=0.0), lp(key=INF), lp(max_stops=16.5), lp(max_stops=NAN), lp(flags=1)]
BAD_COLOUR = [cp(white=(0.0, 1.0, 1.0)), cp(white=(1.0, INF, 1.0)), cp(white=(1.0, 1.0, NAN)), cp(strength=-0.1), cp(strength=1.5), cp(flags=1)]
BAD_FINISH = [fp(sharpness=-0.001), fp(sharpness=NAN), fp(grain=1.001), fp(dither=INF), fp(flags=2)]


def rows_ready():
    """The grid, the bloom image (both of "mean") and a LUT are there: only the arguments are at fault."""
    rows = []
    for f in ALL:
        w = NAMES[f]
        size = ("%s: expected %d floats" % (w, N)) if f is gain else ("%s: expected %d bytes" % (w, N * 4))
        word = "intensity" if f is bloomed else "bloom_intensity"
        rows += [(f, dict(source=9), INVALID, "%s: unknown source 9" % w),
                 (f, dict(n=0), INVALID, "%s: sample_total must be > 0" % w)]
        rows += [(f, dict(e=e), INVALID, "%s: exposure must be finite and > 0" % w) for e in (0.0, -1.0, INF, NAN)]
        rows += [(f, dict(nf=N - 1) if f is gain else dict(nb=N * 4 - 4), INVALID, size)]
        if f is not gain:
            rows += [(f, dict(i=i), INVALID, "%s: %s must be finite and >= 0" % (w, word)) for i in (-0.5, INF, NAN)]
            rows += [(f, dict(i=-0.5, nb=0), INVALID, "%s: %s must be finite and >= 0" % (w, word))]  # the intensity before the size
        # (the exposure, then sample_total — which counts on the mean alone — then the source)
        rows += [(f, dict(e=0.0, n=0), INVALID, "%s: exposure must be finite and > 0" % w),
                 (f, dict(e=0.0, source=9), INVALID, "%s: exposure must be finite and > 0" % w),
                 (f, dict(n=0, source=9), INVALID, "%s: unknown source 9" % w)]
    rows += [(gain, dict(out=None), INVALID, "local_gain_download: host_gain is NULL"),
             (gain, dict(out=None, e=0.0), INVALID, "local_gain_download: host_gain is NULL")]
    for f in TILED:
        w = NAMES[f]
        rows += [(f, dict(p=p), INVALID, LOCAL_TEXT % w) for p in BAD_LOCAL]
    for f in (local, gain):
        rows += [(f, dict(p=None), INVALID, "%s: params is NULL" % NAMES[f])]
    rows += [(local, dict(p=None, i=-1.0), INVALID, "display_local_srgb8: params is NULL"),
             (local, dict(p=BAD_LOCAL[0], i=-1.0), INVALID, LOCAL_TEXT % "display_local_srgb8")]
    for f in GRADED:
        w = NAMES[f]
        rows += [(f, dict(c=None), INVALID, "%s: colour is NULL" % w)]
        rows += [(f, dict(c=c), INVALID, COLOUR_TEXT % w) for c in BAD_COLOUR]
        rows += [(f, dict(p=BAD_LOCAL[0], c=None), INVALID, LOCAL_TEXT % w),  # bad local params with a NULL colour
                 (f, dict(c=BAD_COLOUR[0], i=-0.5), INVALID, COLOUR_TEXT % w)]
    w = NAMES[finished]
    rows += [(finished, dict(f=None), INVALID, "%s: finish is NULL" % w)]
    rows += [(finished, dict(f=f), INVALID, FINISH_TEXT % w) for f in BAD_FINISH]
    rows += [(finished, dict(c=BAD_COLOUR[3], f=BAD_FINISH[0]), INVALID, COLOUR_TEXT % w),  # bad colour with bad finish
             (finished, dict(c=None, f=None), INVALID, "%s: colour is NULL" % w),
             (finished, dict(f=None, i=-0.5), INVALID, "%s: finish is NULL" % w),
             (finished, dict(f=BAD_FINISH[0], i=-0.5), INVALID, FINISH_TEXT % w)]
    rows += [(exposure_download, dict(words=S.EXPOSURE_WORDS + 1), INVALID, "exposure_download: expected 257 words"),
             (exposure_download, dict(p=None), INVALID, "exposure_download: params is NULL"),
             (exposure_download, dict(p=S.ExposureParams(100, 950, 0.18, 2.0 ** -16, 2.0 ** 16, 1.0, 0.0, 1)), INVALID, "exposure_download: flags must be 0"),
             (white_download, dict(words=S.WHITE_WORDS - 1), INVALID, "white_download: expected 4097 words"),
             (white_download, dict(p=None), INVALID, "white_download: params is NULL")]
    return rows


def rows_nothing():
    """After the resets: no grid, no bloom image, no LUT, no histograms.  Each is missed only where it is asked for."""
    rows = [(bloomed, dict(), NOT_READY, NO_BLOOM),
            (bloomed, dict(i=0.0), NOT_READY, NO_BLOOM),  # the bloomed display wants its image at intensity 0 too
            (bloomed, dict(nb=0), INVALID, "display_bloomed_srgb8: expected %d bytes" % (N * 4)),
            (local, dict(), NOT_READY, NO_GRID),
            (local, dict(i=0.5), NOT_READY, NO_GRID),  # no grid with no bloom image
            (local, dict(nb=0), INVALID, "display_local_srgb8: expected %d bytes" % (N * 4)),  # a wrong size with no grid
            (gain, dict(), NOT_READY, NO_GRID),
            (gain, dict(nf=0), INVALID, "local_gain_download: expected %d floats" % N),
            (exposure_download, dict(), NOT_READY, "no exposure histogram (rsrt_exposure_meter first)"),
            (exposure_download, dict(words=3), INVALID, "exposure_download: expected 257 words"),
            (white_download, dict(), NOT_READY, "no chroma histogram (rsrt_white_meter first)"),
            (white_download, dict(words=3), INVALID, "white_download: expected 4097 words")]
    for f in GRADED:
        w = NAMES[f]
        rows += [(f, dict(p=lp()), NOT_READY, NO_GRID),
                 (f, dict(i=0.5), NOT_READY, NO_BLOOM),
                 (f, dict(c=cp(strength=0.5)), NOT_READY, NO_LUT),
                 (f, dict(p=lp(), nb=0), INVALID, "%s: expected %d bytes" % (w, N * 4)),  # a wrong size with no grid
                 (f, dict(p=lp(), i=0.5), NOT_READY, NO_GRID),  # no grid with no bloom image
                 (f, dict(i=0.5, c=cp(strength=0.5)), NOT_READY, NO_BLOOM)]  # no bloom image with no LUT
    return rows


def rows_other_size():
    """The grid and the bloom image were built for "upsampled" (24 x 16); the source is "mean" (12 x 8).  No LUT."""
    rows = [(bloomed, dict(), INVALID, BLOOM_SIZE % NAMES[bloomed]),
            (bloomed, dict(i=0.0), INVALID, BLOOM_SIZE % NAMES[bloomed]),
            (local, dict(), INVALID, GRID_SIZE % NAMES[local]),
            (local, dict(i=0.5), INVALID, GRID_SIZE % NAMES[local]),
            (gain, dict(), INVALID, GRID_SIZE % NAMES[gain])]
    for f in GRADED:
        w = NAMES[f]
        rows += [(f, dict(p=lp()), INVALID, GRID_SIZE % w),
                 (f, dict(i=0.5), INVALID, BLOOM_SIZE % w),
                 (f, dict(p=lp(), i=0.5), INVALID, GRID_SIZE % w),
                 (f, dict(i=0.5, c=cp(strength=0.5)), INVALID, BLOOM_SIZE % w)]
    return rows


def check(st, rows):
    wrong = []
    for f, kw, status, text in rows:
        rc = f(st, **kw)
        got = st._L.rsrt_last_error(st._ctx).decode()
        if (rc, got) != (status, text):
            wrong.append((f.__name__, {k: str(v) for k, v in kw.items()}, (rc, got), (status, text)))
    assert not wrong, wrong


def accepted(st):
    """Everything on at once is taken by every entry point."""
    for f, kw in ((bloomed, {}), (local, dict(i=0.5)), (gain, {}), (colour, dict(p=lp(), i=0.5, c=cp(strength=0.5))),
                  (finished, dict(p=lp(), i=0.5, c=cp(strength=0.5)))):
        assert f(st, **kw) == 0, (f.__name__, st._L.rsrt_last_error(st._ctx).decode())


def test_every_refusal_has_its_status_and_its_text():
    sc, st = state("default", W, H)
    try:
        st.render_upsampled(GW, GH, n=2, denoise=False)
        check(st, rows_nothing())  # a fresh context holds nothing
        st.bloom("mean", 1.5, 2)
        st.local_exposure("mean", 8)
        st.colour_lut(size=2)
        st.exposure_meter("mean")
        st.white_meter("mean")
        accepted(st)
        assert exposure_download(st) == 0 and white_download(st) == 0
        check(st, rows_ready())
        accepted(st)  # a refusal leaves what was there
        st.bloom_reset()
        st.local_exposure_reset()
        st.colour_lut_reset()
        st.exposure_reset()
        st.white_reset()
        check(st, rows_nothing())
        assert colour(st) == 0 and finished(st) == 0  # nothing asked for, nothing missed
        st.bloom("upsampled", 1.5, 2)
        st.local_exposure("upsampled", 8)
        check(st, rows_other_size())
        assert gain(st, source=UPSAMPLED, out=np.zeros((GH, GW), np.float32), nf=GW * GH) == 0  # the source they were built for is taken
    finally:
        st.close()
