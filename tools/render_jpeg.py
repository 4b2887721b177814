"""python tools/render_jpeg.py <scene> <w> <h> <spp> <bounces> <out.jpg | out.avi> [quality=90] [subsampling=420|444] [frames=N pan=DYAW_DEG[,DPITCH_DEG] dolly=UNITS fps=30 | fps=NUM/DEN] [--denoise] [exposure=auto | exposure=X] [bloom=on | bloom=INTENSITY] [local=on | local=SHADOWS,HIGHLIGHTS] [wb=auto | wb=R,G,B] [cdl=SLOPE,OFFSET,POWER,SAT]
— render through the product path and write a baseline JPEG file that the device coded (State.display_jpeg: DCT, quantiser and Huffman
coder are HIP kernels; the host adds the headers), or, with frames=N and a name that ends in .avi, N such files as one Motion-JPEG AVI
(host.write_avi_mjpeg), which every player opens.  Frame k is the scene's camera turned by k * DYAW_DEG degrees about the world's up axis and
k * DPITCH_DEG about its own right axis and moved k * UNITS scene units forward, rendered afresh with <spp> samples; the passes are those
render_png.py knows by the same names (--denoise, exposure=, bloom=, local=, wb=, cdl=: see there).  exposure=auto and wb=auto meter the first
frame fully and follow later frames a quarter of the way, so that the picture does not pump:
    house 480 270 16 8 out.jpg quality=90 exposure=auto
    house 480 270 16 8 out.avi frames=30 pan=2,0 exposure=auto"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host
from rsoderh_raytracing_amd import types as T

KEYS = ("quality=", "subsampling=", "frames=", "pan=", "dolly=", "fps=", "exposure=", "bloom=", "local=", "wb=", "cdl=")
opt = lambda key: next((a[len(key):] for a in sys.argv[1:] if a.startswith(key)), None)  # noqa: E731
denoise = "--denoise" in sys.argv
args = [a for a in sys.argv[1:] if a != "--denoise" and not a.startswith(KEYS)]
if len(args) != 6:
    sys.exit(__doc__)
name, w, h, spp, mb, out = args[0], int(args[1]), int(args[2]), int(args[3]), int(args[4]), args[5]
clip = out.lower().endswith(".avi")
frames = int(opt("frames=") or 1)
if (frames != 1 or opt("frames=") is not None) != clip or frames < 1:
    sys.exit("render_jpeg.py: frames=N goes with a name that ends in .avi, a still with any other")
quality = int(opt("quality=") or R.state.JPEG_DEFAULTS["quality"])
subsampling = opt("subsampling=") or R.state.JPEG_DEFAULTS["subsampling"]
pan = tuple(math.radians(float(v)) for v in (opt("pan=") or "0").split(","))
dyaw, dpitch = pan[0], pan[1] if len(pan) > 1 else 0.0
dolly = float(opt("dolly=") or 0.0)
fps = tuple(int(v) for v in (opt("fps=") or "30").split("/"))
fps = fps if len(fps) == 2 else (fps[0], 1)
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
files = []
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
    files.append(st.display_jpeg(source, e, white, 1.0 if cdl is not None else 0.0, bloom_intensity=bloom or 0.0, quality=quality, subsampling=subsampling, **strengths))
    print("frame %d: exposure %.6g, %d bytes" % (k, e, len(files[-1])), flush=True)
if clip:
    host.write_avi_mjpeg(out, files, w, h, fps)
else:
    with open(out, "wb") as f:
        f.write(files[0])
g = st.stats()
print("%s: %d frame%s of %dx%d, quality %d, %d bytes in all, to %s; kernel ms %s" % (name, frames, "" if frames == 1 else "s", w, h, quality, sum(len(f) for f in files), out, g['kernel_ms']))
