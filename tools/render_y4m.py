"""python tools/render_y4m.py <scene> <w> <h> <spp> <bounces> <out.y4m> frames=N [pan=DYAW_DEG[,DPITCH_DEG]] [dolly=UNITS] [fps=30 | fps=NUM/DEN] [depth=8|10] [hdr=on[,PAPER_WHITE[,PEAK]]] [siting=left|centre|topleft] [range=limited|full] [dither=AMPLITUDE] [--denoise] [exposure=auto | exposure=X] [bloom=on | bloom=INTENSITY] [local=on | local=SHADOWS,HIGHLIGHTS] [wb=auto | wb=R,G,B] [cdl=SLOPE,OFFSET,POWER,SAT]
— render a sequence through the product path and write it as a YUV4MPEG2 file, the uncompressed video every encoder and player reads
(x264, x265, SVT-AV1, ffmpeg, mpv).  Frame k is the scene's camera turned by k * DYAW_DEG degrees about the world's up axis and k * DPITCH_DEG
about its own right axis and moved k * UNITS scene units forward; each frame is rendered afresh with <spp> samples, goes through the
passes render_png.py knows by the same names (--denoise, exposure=, bloom=, local=, wb=, cdl=: see there), becomes a planar Y'CbCr 4:2:0
frame on the device (State.display_video: I420, or yuv420p10le with depth=10; hdr=on: HDR10, Rec.2020 PQ at 10 bits, which takes no cdl=) and is
appended to the file (host.write_y4m).  exposure=auto and wb=auto meter the first frame fully and follow later frames a quarter of the way, so
that the picture does not pump.  The dither's seed is the frame's index.  The frames' content light levels are printed with hdr=on; a stream's
MaxCLL and MaxFALL are the largest of them:
    house 480 270 16 8 out.y4m frames=30 pan=2,0 exposure=auto"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host
from rsoderh_raytracing_amd import types as T

KEYS = ("frames=", "pan=", "dolly=", "fps=", "depth=", "hdr=", "siting=", "range=", "dither=", "exposure=", "bloom=", "local=", "wb=", "cdl=")
opt = lambda key: next((a[len(key):] for a in sys.argv[1:] if a.startswith(key)), None)  # noqa: E731
denoise = "--denoise" in sys.argv
args = [a for a in sys.argv[1:] if a != "--denoise" and not a.startswith(KEYS)]
if len(args) != 6 or opt("frames=") is None:
    sys.exit(__doc__)
name, w, h, spp, mb, out = args[0], int(args[1]), int(args[2]), int(args[3]), int(args[4]), args[5]
frames = int(opt("frames="))
pan = tuple(math.radians(float(v)) for v in (opt("pan=") or "0").split(","))
dyaw, dpitch = pan[0], pan[1] if len(pan) > 1 else 0.0
dolly = float(opt("dolly=") or 0.0)
fps = tuple(int(v) for v in (opt("fps=") or "30").split("/"))
fps = fps if len(fps) == 2 else (fps[0], 1)
hdr = opt("hdr=")
hdr = None if hdr in (None, "off") else hdr.split(",")
depth = int(opt("depth=") or (10 if hdr else 8))
exposure = opt("exposure=")
if exposure is not None and exposure != "auto":
    exposure = float(exposure)
bloom = opt("bloom=")
if bloom is not None:
    bloom = None if bloom == "off" else (R.state.BLOOM_DEFAULTS["intensity"] if bloom == "on" else float(bloom))
local = opt("local=")
if local is not None:
    local = None if local == "off" else ((None, None) if local == "on" else tuple(float(v) for v in local.split(",")))
wb = opt("wb=")
if wb is not None and wb != "auto":
    wb = tuple(float(v) for v in wb.split(","))
cdl = opt("cdl=")
cdl = None if cdl is None else tuple(float(v) for v in cdl.split(","))
if hdr and (cdl is not None or depth != 10):
    sys.exit("render_y4m.py: hdr=on is 10 bits and takes no cdl=")
video = dict(standard="hdr10" if hdr else "bt709", layout="i420p10" if depth == 10 else "i420", range=opt("range=") or "limited", siting=opt("siting=") or "left",
             dither=float(opt("dither=") or 0.0))
if hdr:
    video.update(paper_white=float(hdr[1]) if len(hdr) > 1 else None, peak=float(hdr[2]) if len(hdr) > 2 else None)


def camera_at(first, k):
    """The camera record of frame k: `first` turned by k * dyaw about +y, by k * dpitch about its own right axis, moved k * dolly forward."""
    cam = first.copy()
    axes = cam["rot_transform"][0][:, :3].astype(np.float64)  # row j: the camera's axis j (right, up, backward) in the world
    c, s = math.cos(k * dyaw), math.sin(k * dyaw)
    axes = (np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ axes.T).T
    c, s = math.cos(k * dpitch), math.sin(k * dpitch)
    right, up, back = axes
    axes = np.stack([right, c * up + s * back, c * back - s * up])
    cam["rot_transform"][0][:, :3] = axes
    cam["pos"][0] = first["pos"][0].astype(np.float64) - k * dolly * first["rot_transform"][0][2, :3].astype(np.float64)
    return cam


sc = R.Scene.load_toml(os.path.join(ROOT, 'tests', 'golden', 'assets', 'scenes', name + '.toml'))
st = R.State.new(sc, R.Environment.synthetic(2048, 1024), w, h); st.max_bounces = mb
first = np.array(st.camera).view(T.CAMERA).reshape(1).copy()
if cdl is not None:
    st.colour_lut(*cdl)
white = (1.0, 1.0, 1.0) if wb is None else wb
for k in range(frames):
    st.camera = camera_at(first, k)
    st.render_samples(spp, aov=denoise)
    if denoise:
        st.denoise(download=False)
    source = "denoised" if denoise else "mean"
    e = 1.0 if exposure is None else exposure
    if exposure == "auto":
        e = st.auto_exposure(source, blend=1.0 if k == 0 else 0.25)["exposure"]
    if wb == "auto":
        white = st.auto_white_balance(source, blend=1.0 if k == 0 else 0.25)["white"]
    if bloom is not None:
        st.bloom(source, e)
    strengths = {}
    if local is not None:
        st.local_exposure(source)
        strengths = {"shadows": R.state.LOCAL_DEFAULTS["shadows"] if local[0] is None else local[0], "highlights": local[1]}
    got = st.display_video(source, e, white, None if hdr else (1.0 if cdl is not None else 0.0), bloom_intensity=bloom or 0.0, seed=k, levels=bool(hdr), **video, **strengths)
    frame, levels = got if hdr else (got, None)
    host.write_y4m(out, frame, fps, append=k > 0)
    print("frame %d: exposure %.6g%s" % (k, e, "" if levels is None else ", MaxCLL %.6g cd/m^2, MaxFALL %.6g cd/m^2" % (levels["max_cll"], levels["max_fall"])), flush=True)
g = st.stats()
print("%s: %d frames of %dx%d, %d bytes each, to %s; kernel ms %s" % (name, frames, w, h, frame.data.nbytes, out, g['kernel_ms']))
