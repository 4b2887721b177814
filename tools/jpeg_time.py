"""Times the JPEG pass at 1920x1080 on house against the colour display and the video pass in the same process, on the host clock after 3
warm-up rounds (median and minimum of --reps), the way tools/video_time.py times the video pass — every one of these calls runs its
kernels on the context's stream, copies its result to the host and waits (8.3 MB for the colour display, 3.1 MB for NV12, the coded scan
alone for JPEG, behind an 8-byte copy of its size) — alternated: a round makes every call once, so that a drift of the machine falls on
all of them alike.  The calls: rsrt_display_colour_srgb8, rsrt_display_video as full-range NV12 at the centre siting (JPEG's own
sampling), and rsrt_display_jpeg at qualities 50, 90 and 100 at both subsamplings, into a buffer of the worst case's size so that no
call is made twice.  The files' sizes are recorded.  Prints one JSON line and writes it to profiles/jpeg_house_1080p.json (--out); the
line carries the library's build id.  The kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python tools/jpeg_time.py --reps 5 --out ''
and are folded in with --kernel-stats CSV.
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# as kernel_stats.csv names them (demangled), and the key each goes by in the JSON
KERNELS = {r"rt_display_colour_kernel": "rt_display_colour_kernel", r"rt_display_video_kernel<0u?, ?8u?, ?1u?, ?false>": "rt_display_video_kernel<bt709, 8, centre>",
           r"rt_jpeg_blocks_kernel<0u?>": "rt_jpeg_blocks_kernel<420>", r"rt_jpeg_blocks_kernel<1u?>": "rt_jpeg_blocks_kernel<444>",
           r"rt_jpeg_scan_kernel": "rt_jpeg_scan_kernel", r"rt_jpeg_pack_kernel": "rt_jpeg_pack_kernel"}
JPEG = {"jpeg_q%d_%s" % (q, s): dict(quality=q, subsampling=s) for q in (50, 90, 100) for s in ("420", "444")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="fold the kernels' rows of a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_house_1080p.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.loads(f.readline())
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(ln for ln in f if not ln.startswith("#"))]
        k = out["kernels_rocprofv3"] = {}
        for r in rows:
            for pattern, name in KERNELS.items():
                if re.search(pattern, r["Name"]):
                    k[name] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
        missing = [name for name in KERNELS.values() if name not in k]
        if missing:
            sys.exit("jpeg_time.py: %s has no row for %s" % (a.kernel_stats, ", ".join(missing)))
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    import rsoderh_raytracing_amd as R
    S = R.state
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps}
    st.render_samples(a.samples)
    e = out["exposure"] = st.auto_exposure()["exposure"]
    colour = st._colour_params((1.0, 1.0, 1.0), 0.0)
    room = np.empty(S.jpeg_max_bytes(a.width, a.height, "444"), np.uint8)
    n = C.c_size_t(0)

    def jpeg(kw):  # one call, no second try: the buffer holds the worst case
        j = S.jpeg_params(**kw)
        st._check(st._L.rsrt_display_jpeg(st._ctx, 0, st.sample_count, e, None, 0.0, C.byref(colour), C.byref(j), S._p(room), room.nbytes, C.byref(n)), "rsrt_display_jpeg")
        return n.value
    calls = {"display_colour": lambda: st.display_colour_srgb8(lut_strength=0.0, white=(1.0, 1.0, 1.0)),
             "nv12_full_centre": lambda: st.display_video(lut_strength=0.0, white=(1.0, 1.0, 1.0), layout="nv12", range="full", siting="centre")}
    for key, kw in JPEG.items():
        calls[key] = lambda kw=kw: jpeg(kw)
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):  # alternated: every call once a round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep >= 3:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out["calls"] = {k: {"host_ms_median": float(np.median(ts)), "host_ms_min": float(np.min(ts))} for k, ts in times.items()}
    yard = out["calls"]["nv12_full_centre"]
    for key, o in out["calls"].items():
        o["over_nv12"] = o["host_ms_median"] / yard["host_ms_median"]
        o["slower_than_nv12_by_more_than_its_spread"] = bool(o["host_ms_median"] - yard["host_ms_median"] > yard["host_ms_median"] - yard["host_ms_min"])
    out["bytes"] = {"display_colour": a.width * a.height * 4, "nv12_full_centre": int(S.video_planes(a.width, a.height, 8, S.VIDEO_SEMIPLANAR)[0])}
    out["bytes"].update({key: int(jpeg(kw)) for key, kw in JPEG.items()})
    st.close()
    out["build_id"] = S.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
