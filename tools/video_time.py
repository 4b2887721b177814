"""Times the video pass at 1920x1080 on house against the colour display and the HDR display in the same process, on the host clock
after 3 warm-up rounds (median and minimum of --reps), the way tools/hdr_time.py times the HDR display — every one of these calls runs
its kernel on the context's stream, copies its result to the host and waits (8.3 MB for the two yardsticks, 3.1 MB for NV12 and I420,
6.2 MB for the 10-bit frames) — alternated: a round makes every call once, so that a drift of the machine falls on all of them alike.
The calls: rsrt_display_colour_srgb8 and rsrt_display_hdr PQ10 (the yardsticks), and rsrt_display_video as NV12, I420, P010 and HDR10
P010, each at the three sitings, and NV12 with dither and HDR10 P010 with the light levels at the left siting — with local exposure and
bloom off, and with both on (no LUT).  Every video call is also set against its yardstick's own min-to-median spread in the run.
Prints one JSON line and writes it to profiles/video_house_1080p.json (--out); the line carries the library's build id.  The kernels'
own times come from
    rocprofv3 --kernel-trace --stats -- python tools/video_time.py --reps 5 --out ''
and are folded in with --kernel-stats CSV.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SITINGS = ("left", "centre", "topleft")
# as kernel_stats.csv names them (demangled: <standard, depth, siting, levels>), and the key each goes by in the JSON
KERNELS = {r"rt_display_colour_kernel": "rt_display_colour_kernel", r"rt_display_hdr_kernel<0u?, ?false>": "rt_display_hdr_kernel<pq10>"}
for std, depth, name in ((0, 8, "bt709, 8"), (0, 10, "bt709, 10"), (1, 10, "hdr10, 10")):
    for g, siting in ((0, "left"), (1, "centre"), (2, "topleft")):
        KERNELS[r"rt_display_video_kernel<%du?, ?%du?, ?%du?, ?false>" % (std, depth, g)] = "rt_display_video_kernel<%s, %s>" % (name, siting)
KERNELS[r"rt_display_video_kernel<1u?, ?10u?, ?0u?, ?true>"] = "rt_display_video_kernel<hdr10, 10, left, levels>"
VIDEO = {}
for siting in SITINGS:
    VIDEO["nv12_" + siting] = dict(layout="nv12", siting=siting)
    VIDEO["i420_" + siting] = dict(layout="i420", siting=siting)
    VIDEO["p010_" + siting] = dict(layout="p010", siting=siting)
    VIDEO["hdr10_p010_" + siting] = dict(standard="hdr10", layout="p010", siting=siting)
VIDEO["nv12_left_dither"] = dict(layout="nv12", siting="left", dither=1.0)
VIDEO["hdr10_p010_left_levels"] = dict(standard="hdr10", layout="p010", siting="left", levels=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="fold the display kernels' rows of a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_house_1080p.json"))
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
            sys.exit("video_time.py: %s has no row for %s" % (a.kernel_stats, ", ".join(missing)))
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps}
    st.render_samples(a.samples)
    out["exposure"] = st.auto_exposure()["exposure"]
    st.bloom()
    st.local_exposure()
    chains = {"plain": dict(white=(1.0, 1.0, 1.0)), "local_bloom": dict(white=(1.0, 1.0, 1.0), shadows=0.5, highlights=0.5, bloom_intensity=0.1)}
    calls = {}
    for cname, chain in chains.items():
        calls[cname, "display_colour"] = lambda chain=chain: st.display_colour_srgb8(lut_strength=0.0, **chain)
        calls[cname, "hdr_pq10"] = lambda chain=chain: st.display_hdr(**chain)
        for key, kw in VIDEO.items():
            calls[cname, key] = lambda chain=chain, kw=kw: st.display_video(lut_strength=0.0, **chain, **kw)
    times = {k: [] for k in calls}
    for rep in range(3 + a.reps):  # alternated: every call once a round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep >= 3:
                times[k].append((time.perf_counter() - t0) * 1e3)
    for (cname, key), ts in times.items():
        out.setdefault(cname, {})[key] = {"host_ms_median": float(np.median(ts)), "host_ms_min": float(np.min(ts))}
    for cname in chains:
        for key, o in out[cname].items():
            yard = out[cname]["hdr_pq10" if key.startswith("hdr") else "display_colour"]
            o["over_yardstick"] = o["host_ms_median"] / yard["host_ms_median"]
            o["slower_than_yardstick_by_more_than_its_spread"] = bool(o["host_ms_median"] - yard["host_ms_median"] > yard["host_ms_median"] - yard["host_ms_min"])
    out["frame_bytes"] = {key: int(st.display_video(lut_strength=0.0, **{k: v for k, v in kw.items() if k != "levels"}).data.nbytes) for key, kw in VIDEO.items()}
    st.close()
    out["build_id"] = R.state.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
