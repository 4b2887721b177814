"""python tools/render_png.py <scene> <w> <h> <spp | noise=X[,MAX]> <bounces> <out.png> [--denoise] [sky=ELEV_DEG,AZIMUTH_DEG[,TURBIDITY]] [exposure=auto | exposure=X] [bloom=on | bloom=INTENSITY] [local=on | local=SHADOWS,HIGHLIGHTS] [dof=FOCUS,APERTURE[,RADIUS] | dof=auto,APERTURE[,RADIUS]] [motion=YAW_DEG,DOLLY[,SHUTTER[,RADIUS]]] [fog=DENSITY[,G[,STEPS]]] [foghalf=on] [wb=auto | wb=R,G,B] [cdl=SLOPE,OFFSET,POWER,SAT] [finish=SHARPNESS[,GRAIN[,DITHER]]] [hdr=pq[,PAPER_WHITE[,PEAK]]] — render
through the product path and write the display image; noise=X in place of a sample count: render until the largest 16x16 tile's noise
estimate is at most X (State.render_to_noise, at most MAX samples, default 1024) and print the rounds; --denoise: the AOV pass over the
same samples and the default filter, the denoised display image instead; exposure=auto: meter the picture that is written
(State.auto_exposure), print the metered exposure and average luminance and write the exposed display image; exposure=X: that exposure.
With noise=X the exposure also puts the threshold in displayed units (auto: metered after the first 8 samples).  bloom=on or
bloom=INTENSITY: State.bloom of the picture that is written, at its exposure (1 without exposure=), and the bloomed display image at the
default or the given intensity.  local=on or local=SHADOWS,HIGHLIGHTS: State.local_exposure of the picture that is written and the graded
display image at its exposure, with the default or the given strengths and, with bloom=, the bloom added before the gain.
dof=FOCUS,APERTURE[,RADIUS]: State.depth_of_field of the picture (the AOV pass over the same samples gives the depths) focused at FOCUS
scene units along the axis (auto: at the depth of the picture's centre, State.focus_at), with APERTURE the blur radius of a point at
infinity as a fraction of the picture's height and at most RADIUS pixels (default 8); it runs before exposure=, bloom= and local=, which
then meter, bloom and grade the lens image.
motion=YAW_DEG,DOLLY[,SHUTTER[,RADIUS]]: State.motion_blur of the picture (the AOV pass over the same samples gives the depths) for a camera
that one frame earlier was turned back by YAW_DEG degrees about the world's up axis and stood DOLLY scene units back along its forward
axis, with the shutter open for SHUTTER of the frame interval (default 0.5) and a blur of at most RADIUS pixels each way (default 16);
it runs after dof= and before exposure=, bloom=, local=, wb= and cdl=, which then take the motion image.
fog=DENSITY[,G[,STEPS]]: State.render_fog over the picture's samples — a homogeneous medium of extinction DENSITY per scene unit, Henyey-Greenstein
anisotropy G (default 0.6), STEPS march points a camera ray (default 16) — and State.fog of the picture; the light is the sun of sky= when
given (State.fog_light_from_sky), else the synthetic map's sun, from normalize(0.4, 0.6, -0.7) with the irradiance of its lobe, 20 pi (1, 0.95,
0.85).  It runs after --denoise and before dof=, motion= and the rest, which then take the fog image.
foghalf=on (with fog=): the march runs at ceil(W / 2) x ceil(H / 2) and the fog image is rebuilt at full size from those records and the
picture's first-hit records (State.fog(upsample=True)); the AOV pass runs over the picture's samples for it.
sky=ELEV_DEG,AZIMUTH_DEG[,TURBIDITY]: environment 0 is the procedural daylight sky (State.environment_sky, 2048 x 1024, built on the
device: no map is prepared on the host) with the sun at that elevation and azimuth in degrees, instead of the synthetic map; it
composes with everything above.  The sky's default scale leaves daylight far above a display's range: use exposure=auto with it.
wb=auto: meter the chroma of the picture that is written (State.auto_white_balance), print the white point and multiply it in before the
tone map; wb=R,G,B: those gains.  cdl=SLOPE,OFFSET,POWER,SAT: bake that ASC CDL into a 33^3 LUT on the device (State.colour_lut) and read
the tone-mapped picture through it.  Either one sends the picture through the colour display (State.display_colour_srgb8), which
composes with exposure= (1 without), bloom=, local=, dof= and sky=:  house 960 540 64 8 out.png sky=8,120 exposure=auto wb=auto
finish=SHARPNESS[,GRAIN[,DITHER]]: the final display goes through the finished display (State.display_finished_srgb8) with whatever
exposure=, wb=, cdl=, local= and bloom= were given: the sharpener at SHARPNESS (0 .. 1), film grain at GRAIN (default 0) and the dithered
quantiser at DITHER (default 1), seed 0.
hdr=pq[,PAPER_WHITE[,PEAK]]: the final display is the HDR display (State.display_hdr, PQ10, a linear 1.0 at PAPER_WHITE cd/m^2 under a peak of
PEAK, defaults 203 and 1000) with whatever exposure=, wb=, local= and bloom= were given (cdl= and finish= are display-referred SDR and do not
compose with it), written as a 16-bit RGB PNG of the 10-bit codes (code << 6 | code >> 4) with a cICP chunk (BT.2020 primaries 9, PQ
transfer 16, RGB matrix 0, full range 1) and a cLLi chunk holding the frame's MaxCLL and MaxFALL:  house 960 540 64 8 out.png exposure=auto hdr=pq"""
import os, struct, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host
denoise = "--denoise" in sys.argv
exposure = next((a[len("exposure="):] for a in sys.argv[1:] if a.startswith("exposure=")), None)
if exposure is not None and exposure != "auto":
    exposure = float(exposure)
bloom = next((a[len("bloom="):] for a in sys.argv[1:] if a.startswith("bloom=")), None)
if bloom is not None:
    bloom = None if bloom == "off" else (R.state.BLOOM_DEFAULTS["intensity"] if bloom == "on" else float(bloom))
local = next((a[len("local="):] for a in sys.argv[1:] if a.startswith("local=")), None)
if local is not None:
    local = None if local == "off" else ((None, None) if local == "on" else tuple(float(v) for v in local.split(",")))
dof = next((a[len("dof="):].split(",") for a in sys.argv[1:] if a.startswith("dof=")), None)
motion = next((a[len("motion="):].split(",") for a in sys.argv[1:] if a.startswith("motion=")), None)
fog = next((a[len("fog="):].split(",") for a in sys.argv[1:] if a.startswith("fog=")), None)
foghalf = bool(fog) and "foghalf=on" in sys.argv[1:]
sky = next((a[len("sky="):].split(",") for a in sys.argv[1:] if a.startswith("sky=")), None)
wb = next((a[len("wb="):] for a in sys.argv[1:] if a.startswith("wb=")), None)
if wb is not None and wb != "auto":
    wb = tuple(float(v) for v in wb.split(","))
cdl = next((tuple(float(v) for v in a[len("cdl="):].split(",")) for a in sys.argv[1:] if a.startswith("cdl=")), None)
finish = next((tuple(float(v) for v in a[len("finish="):].split(",")) for a in sys.argv[1:] if a.startswith("finish=")), None)
hdr = next((a[len("hdr="):].split(",") for a in sys.argv[1:] if a.startswith("hdr=")), None)
if hdr is not None and (hdr[0] != "pq" or cdl is not None or finish is not None):
    sys.exit("render_png.py: hdr= is hdr=pq[,PAPER_WHITE[,PEAK]] and takes neither cdl= nor finish=")
args = [a for a in sys.argv[1:] if a != "--denoise" and not a.startswith(("exposure=", "bloom=", "local=", "dof=", "motion=", "fog=", "foghalf=", "sky=", "wb=", "cdl=", "finish=", "hdr="))]


def write_hdr_png(path, codes, levels):
    """codes [H, W, 3] 10-bit Rec.2020 PQ codes -> a 16-bit RGB PNG tagged with cICP (9, 16, 0, 1) and cLLi (MaxCLL, MaxFALL in 0.0001 cd/m^2)."""
    import numpy as np
    c = codes.astype(np.uint16)
    rows = ((c << 6) | (c >> 4)).astype(">u2").reshape(c.shape[0], -1)
    raw = b"".join(b"\0" + r.tobytes() for r in rows)  # filter 0 on every row
    chunk = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)  # noqa: E731
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", c.shape[1], c.shape[0], 16, 2, 0, 0, 0)) + chunk(b"cICP", bytes([9, 16, 0, 1])) +
                chunk(b"cLLi", struct.pack(">II", round(levels["max_cll"] * 10000), round(levels["max_fall"] * 10000))) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                chunk(b"IEND", b""))


name, w, h, mb, out = args[0], int(args[1]), int(args[2]), int(args[4]), args[5]
sc = R.Scene.load_toml(os.path.join(ROOT, 'tests', 'golden', 'assets', 'scenes', name + '.toml'))
if sky:
    import math
    st = R.State.new(sc, [], w, h); st.max_bounces = mb
    turbidity = float(sky[2]) if len(sky) > 2 else R.state.SKY_DEFAULTS["turbidity"]
    sky_params = {"sun_elevation": math.radians(float(sky[0])), "sun_azimuth": math.radians(float(sky[1])), "turbidity": turbidity}
    st.environment_sky(0, 2048, 1024, **sky_params)
    print("sky: sun at elevation %g degrees, azimuth %g degrees, turbidity %g (2048x1024, built on the device)" % (float(sky[0]), float(sky[1]), turbidity))
else:
    st = R.State.new(sc, R.Environment.synthetic(2048, 1024), w, h); st.max_bounces = mb
if args[3].startswith("noise="):
    target = args[3][len("noise="):].split(",")
    spp, _ = st.render_to_noise(float(target[0]), max_samples=int(target[1]) if len(target) > 1 else 1024, exposure=exposure,
                                on_round=lambda r: print("samples %4d -> %4d: max tile error %.4f, mean %.4f, %d tiles above" % r, flush=True))
    print("stopped at", spp, "samples")
    if denoise or dof or motion or foghalf:
        st.render_aov(0, spp)
else:
    st.render_samples(int(args[3]), aov=denoise or bool(dof) or bool(motion) or foghalf)
if denoise:
    st.denoise(download=False)
source = "denoised" if denoise else "mean"
if fog:
    import math
    if sky:
        light = st.fog_light_from_sky(**sky_params)
    else:  # the synthetic map's sun (rsrt_synth_environment): 5e4 exp(-(1 - cos) / 2e-4) (1, .95, .85) integrates to 5e4 * 2 pi * 2e-4 of each
        n = math.sqrt(0.4 * 0.4 + 0.6 * 0.6 + 0.7 * 0.7)
        light = {"light_dir": (0.4 / n, 0.6 / n, -0.7 / n), "light_irradiance": tuple(20.0 * math.pi * c for c in (1.0, 0.95, 0.85))}
    st.render_fog(st.sample_count, 0, density=float(fog[0]), anisotropy=float(fog[1]) if len(fog) > 1 else R.state.FOG_DEFAULTS["anisotropy"],
                  steps=int(fog[2]) if len(fog) > 2 else R.state.FOG_DEFAULTS["steps"], size=((w + 1) // 2, (h + 1) // 2) if foghalf else None, **light)
    st.fog(source, upsample=foghalf)
    rec = st.download_fog() / st.fog_sample_count
    print("fog: mean transmittance %.3g, mean inscatter %.3g %.3g %.3g (light from %.3f %.3f %.3f)" % ((rec[..., 3].mean(),) + tuple(rec[..., :3].mean(axis=(0, 1))) + tuple(light["light_dir"])))
    source = "fog"
if dof:
    focus = st.focus_at(w // 2, h // 2) if dof[0] == "auto" else float(dof[0])
    print("focus distance %.6g%s" % (focus, " (the centre is sky: the default focus)" if focus == float("inf") else ""))
    st.depth_of_field(source, None if dof[0] == "auto" else focus, float(dof[1]), int(dof[2]) if len(dof) > 2 else None)
    r = abs(st.dof_coc())
    print("blur radius: mean %.3g px, %.1f %% of the pixels above half a pixel" % (r.mean(), 100.0 * (r > 0.5).mean()))
    source = "lens"
if motion:
    import math
    previous = R.state.camera_earlier(st.camera, math.radians(float(motion[0])), float(motion[1]))
    st.motion_blur(source, previous, float(motion[2]) if len(motion) > 2 else None, int(motion[3]) if len(motion) > 3 else None)
    l = st.motion_velocity()[..., 2]
    print("blur half-length: mean %.3g px, largest %.3g px, %.1f %% of the pixels above half a pixel" % (l.mean(), l.max(), 100.0 * (l > 0.5).mean()))
    source = "motion"
if exposure == "auto":
    st.exposure_reset()  # meter the picture that is written, whatever render_to_noise metered on the way
    r = st.auto_exposure(source)
    print("metered exposure %.6g, average luminance %.6g (%d pixels metered, %d skipped)" % (r["exposure"], r["average_luminance"], r["metered"], r["skipped"]))
    exposure = r["exposure"]
if wb is not None or cdl is not None or finish is not None or hdr is not None:
    if wb == "auto":
        r = st.auto_white_balance(source)
        print("white point %.4f %.4f %.4f (illuminant %.4f 1 %.4f; %d of %d pixels in the window%s)" % (r["white"] + (r["illuminant"][0], r["illuminant"][2], r["gated"],
              r["counted"] + r["skipped"], "" if r["estimated"] else ": too few, no estimate")))
        wb = r["white"]
    if cdl is not None:
        st.colour_lut(*cdl)
    if bloom is not None:
        st.bloom(source, exposure)
    if local is not None:
        st.local_exposure(source)
        strengths = {"shadows": R.state.LOCAL_DEFAULTS["shadows"] if local[0] is None else local[0], "highlights": local[1]}
    if hdr is not None:
        words, levels = st.display_hdr(source, 1.0 if exposure is None else exposure, wb or (1.0, 1.0, 1.0), bloom_intensity=bloom or 0.0,
                                       paper_white=float(hdr[1]) if len(hdr) > 1 else None, peak=float(hdr[2]) if len(hdr) > 2 else None, levels=True,
                                       **(strengths if local is not None else {}))
        print("hdr: PQ10, MaxCLL %.6g cd/m^2, MaxFALL %.6g cd/m^2" % (levels["max_cll"], levels["max_fall"]))
        write_hdr_png(out, R.state.hdr_unpack_pq10(words), levels)
        g = st.stats(); print(name, 'kernel ms', g['kernel_ms'], 'rays', g['ext_rays'] + g['shadow_rays'])
        sys.exit(0)
    show = st.display_colour_srgb8
    if finish is not None:
        knobs = dict(zip(("sharpness", "grain", "dither"), finish))
        print("finish: sharpness %g, grain %g, dither %g" % tuple(knobs.get(k, R.state.FINISH_DEFAULTS[k]) for k in ("sharpness", "grain", "dither")))
        show = lambda *a, **kw: st.display_finished_srgb8(*a, **kw, **knobs)
    host.write_png(out, show(source, 1.0 if exposure is None else exposure, wb or (1.0, 1.0, 1.0), 1.0 if cdl is not None else 0.0,
                        bloom_intensity=bloom or 0.0, **(strengths if local is not None else {})))
elif local is not None:
    if bloom is not None:
        st.bloom(source, exposure)
    st.local_exposure(source)
    host.write_png(out, st.display_local_srgb8(source, exposure, local[0], local[1], bloom_intensity=bloom or 0.0))
elif bloom is not None:
    st.bloom(source, exposure)
    host.write_png(out, st.display_bloomed_srgb8(source, exposure, bloom))
elif exposure is not None:
    host.write_png(out, st.display_exposed_srgb8(source, exposure))
elif dof or motion or fog:
    host.write_png(out, st.display_exposed_srgb8(source, 1.0))  # (exposure 1: the bytes of the plain display pass)
else:
    host.write_png(out, st.denoised_display_srgb8() if denoise else st.display_srgb8())
g = st.stats(); print(name, 'kernel ms', g['kernel_ms'], 'rays', g['ext_rays'] + g['shadow_rays'])
