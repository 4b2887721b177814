"""Times the finished display at 1920x1080 on house against the colour display in the same run, on the host clock after 3 warm-up calls
(median and minimum of --reps), the way tools/colour_time.py times the displays: every one of these calls runs its kernel on the
context's stream, copies 8 MB to the host and waits.  Four calls — rsrt_display_colour_srgb8, rsrt_display_finished_srgb8 with everything
0, with the dither only, with sharpness 0.5 and the dither — each with local exposure, bloom and the LUT off, and with all three on.
Prints one JSON line and writes it to profiles/finish_house_1080p.json (--out); the line carries the library's build id.  The kernels'
own times come from  rocprofv3 --kernel-trace --stats -- python tools/finish_time.py --reps 5 --out ''  and are folded in with
--kernel-stats CSV (the calls of a kernel are then the four or two settings that share it, in equal numbers).
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KERNELS = ("rt_display_colour_kernel", "rt_display_finish_kernel<false>", "rt_display_finish_kernel<true>")  # as kernel_stats.csv names them: demangled
SETTINGS = {"finished_all_zero": dict(sharpness=0.0, grain=0.0, dither=0.0), "finished_dither": dict(sharpness=0.0, grain=0.0, dither=1.0),
            "finished_sharpen_dither": dict(sharpness=0.5, grain=0.0, dither=1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="fold the display kernels' rows of a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finish_house_1080p.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.loads(f.readline())
        with open(a.kernel_stats) as f:
            rows = [r for r in csv.DictReader(ln for ln in f if not ln.startswith("#"))]
        k = out["kernels_rocprofv3"] = {}
        for r in rows:
            for name in KERNELS:
                if name in r["Name"]:
                    k[name] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
        missing = [name for name in KERNELS if name not in k]
        if missing:
            sys.exit("finish_time.py: %s has no row for %s" % (a.kernel_stats, ", ".join(missing)))
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces

    def host_timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"host_ms_median": float(np.median(ts)), "host_ms_min": float(np.min(ts))}

    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps}
    st.render_samples(a.samples)
    out["exposure"] = st.auto_exposure()["exposure"]
    st.bloom()
    st.local_exposure()
    st.colour_lut(1.1, 0.01, 1.2, 1.25, size=33)
    chains = {"plain": dict(white=(1.0, 1.0, 1.0), lut_strength=0.0), "local_bloom_lut": dict(white=(1.0, 1.0, 1.0), lut_strength=1.0, shadows=0.5, highlights=0.5, bloom_intensity=0.1)}
    for name, chain in chains.items():
        o = out[name] = {"display_colour": host_timed(lambda: st.display_colour_srgb8(**chain))}
        for key, kw in SETTINGS.items():
            o[key] = host_timed(lambda: st.display_finished_srgb8(**chain, **kw))
            o[key]["over_display_colour"] = o[key]["host_ms_median"] / o["display_colour"]["host_ms_median"]
        assert np.array_equal(st.display_finished_srgb8(**chain, **SETTINGS["finished_all_zero"]), st.display_colour_srgb8(**chain))
    st.close()
    out["build_id"] = R.state.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
