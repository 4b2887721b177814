"""Times the HDR display at 1920x1080 on house against the colour display in the same process, on the host clock after 3 warm-up rounds
(median and minimum of --reps), the way tools/finish_time.py times the finished display — every one of these calls runs its kernel on
the context's stream, copies its picture (8 MB; 16 MB for scRGB) to the host and waits — but alternated: a round makes every call once,
so that a drift of the machine falls on all of them alike.  The calls: rsrt_display_colour_srgb8, rsrt_display_finished_srgb8 with
everything 0 (the yardstick: one more tail behind the same head), and rsrt_display_hdr as PQ10, PQ10 with dither, PQ10 with the light
levels, PQ10 with both, scRGB and scRGB with the levels — each with local exposure and bloom off, and with both on (no LUT: the HDR
display takes none).  Prints one JSON line and writes it to profiles/hdr_house_1080p.json (--out); the line carries the library's
build id.  The kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python tools/hdr_time.py --reps 5 --skip-dither --out ''
(without the dithered calls a kernel's rows are one setting's, in both chains) and are folded in with --kernel-stats CSV.
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

# as kernel_stats.csv names them (demangled), and the key each goes by in the JSON
KERNELS = {r"rt_display_colour_kernel": "rt_display_colour_kernel", r"rt_display_finish_kernel<false>": "rt_display_finish_kernel<false>",
           r"rt_display_hdr_kernel<0u?, ?false>": "rt_display_hdr_kernel<pq10>", r"rt_display_hdr_kernel<0u?, ?true>": "rt_display_hdr_kernel<pq10, levels>",
           r"rt_display_hdr_kernel<1u?, ?false>": "rt_display_hdr_kernel<scrgb16f>", r"rt_display_hdr_kernel<1u?, ?true>": "rt_display_hdr_kernel<scrgb16f, levels>",
           r"rt_hdr_levels_kernel": "rt_hdr_levels_kernel"}
HDR = {"hdr_pq10": dict(encoding="pq10"), "hdr_pq10_dither": dict(encoding="pq10", dither=1.0), "hdr_pq10_levels": dict(encoding="pq10", levels=True),
       "hdr_pq10_dither_levels": dict(encoding="pq10", dither=1.0, levels=True), "hdr_scrgb16f": dict(encoding="scrgb16f"),
       "hdr_scrgb16f_levels": dict(encoding="scrgb16f", levels=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-dither", action="store_true", help="leave the dithered calls out (for the kernel trace: they share their kernels with the undithered ones)")
    ap.add_argument("--kernel-stats", default=None, help="fold the display kernels' rows of a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr_house_1080p.json"))
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
            sys.exit("hdr_time.py: %s has no row for %s" % (a.kernel_stats, ", ".join(missing)))
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
        calls[cname, "finished_all_zero"] = lambda chain=chain: st.display_finished_srgb8(lut_strength=0.0, sharpness=0.0, grain=0.0, dither=0.0, **chain)
        for key, kw in HDR.items():
            if not (a.skip_dither and "dither" in kw):
                calls[cname, key] = lambda chain=chain, kw=kw: st.display_hdr(**chain, **kw)
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
            o["over_display_colour"] = o["host_ms_median"] / out[cname]["display_colour"]["host_ms_median"]
        out[cname]["levels"] = st.display_hdr(levels=True, **chains[cname])[1]
    st.close()
    out["build_id"] = R.state.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
