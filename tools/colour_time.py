"""Times white balance and colour grading at 1920x1080 on house with HIP events on one stream after 3 warm-up calls (median and minimum
of --reps): rsrt_white_meter and a 33^3 rsrt_colour_lut_build and, in the same run, rsrt_exposure_meter — the meter with the same trips
over a 257-word histogram — and a device-to-device copy of the same W x H float4 image on that stream.  The colour display — white
point alone, with the LUT, with the LUT and the local grade — against the exposed and the local display is timed on the host clock: every
one of these calls runs its kernel on the context's stream, copies 8 MB to the host and waits.  Then the picture: the white point metered
on the frame and on the frame under the tint (1.7, 1, 0.55), uploaded again as the accumulator.  Prints one JSON line and writes it to
profiles/colour_house_1080p.json (--out); the line carries the library's build id.  The per-kernel split comes from
rocprofv3 --kernel-trace --stats -- python tools/colour_time.py --reps 5 --out '' and is folded in with --kernel-stats CSV.
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KERNELS = ("rt_white_hist_kernel", "rt_colour_lut_kernel", "rt_display_colour_kernel", "rt_exposure_hist_kernel", "rt_display_exposed_kernel", "rt_display_local_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="fold the new and the neighbouring kernels' rows of a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_house_1080p.json"))
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
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces
    # HIP events on a stream of our own, from the HIP runtime librsrt.so is linked against
    maps = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln}, key=lambda q: "torch" in q)
    hip = C.CDLL(maps[0])  # (torch's copy only when torch was loaded first: the loader then gave librsrt that one)
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    sp = stream.value

    def timed(fn):
        for _ in range(3):  # warm-up
            fn()
        st.synchronize()
        ts = []
        for _ in range(a.reps):
            st.synchronize()
            hip.hipEventRecord(ev0, stream)
            fn()
            hip.hipEventRecord(ev1, stream)
            assert hip.hipEventSynchronize(ev1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ts.append(t.value)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_all": [round(t, 5) for t in ts]}

    def host_timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"host_ms_median": float(np.median(ts)), "host_ms_min": float(np.min(ts))}

    n = a.width * a.height
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps}
    st.render_samples(a.samples)
    out["exposure"] = st.auto_exposure()["exposure"]
    nbytes = n * 16
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
    acc = st.download()
    assert hip.hipMemcpy(src, acc.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out["device_copy"] = timed(lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, sp))
    out["exposure_meter"] = timed(lambda: st.exposure_meter(stream=sp))
    out["white_meter"] = timed(lambda: st.white_meter(stream=sp))
    out["white_meter"]["over_exposure_meter"] = out["white_meter"]["ms_median"] / out["exposure_meter"]["ms_median"]
    hist, r = st.white_download()
    out["white_meter"]["words_counted_into"] = int(np.count_nonzero(hist))
    out["colour_lut_33"] = timed(lambda: st.colour_lut(1.1, 0.01, 1.2, 1.25, size=33, stream=sp))
    out["colour_lut_33"]["bytes"] = 33 ** 3 * 16
    white = r["white"]
    out["white"] = {k: r[k] for k in ("white", "illuminant", "eu", "ev", "gated", "counted", "skipped", "estimated")}
    st.local_exposure()
    out["display_exposed"] = host_timed(lambda: st.display_exposed_srgb8())
    out["display_local"] = host_timed(lambda: st.display_local_srgb8())
    out["display_colour_white"] = host_timed(lambda: st.display_colour_srgb8(white=white, lut_strength=0.0))
    out["display_colour_lut"] = host_timed(lambda: st.display_colour_srgb8(white=white, lut_strength=1.0))
    out["display_colour_lut_local"] = host_timed(lambda: st.display_colour_srgb8(white=white, lut_strength=1.0, shadows=0.5, highlights=0.5))
    # the picture: the same frame under a tint, as the accumulator of a second context
    tint = (1.7, 1.0, 0.55)
    tinted = acc.copy()
    tinted[..., :3] *= np.float32(tint)
    assert hip.hipMemcpy(dst, tinted.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0
    other = R.State()
    other.bind_accumulator(dst.value, a.width, a.height)
    other.white_meter(sample_total=a.samples)
    t = other.white_download()[1]
    other.close()
    out["tinted"] = {"tint": tint, "white": t["white"], "eu": t["eu"], "ev": t["ev"], "gated": t["gated"],
                     "eu_error_octaves": t["eu"] - r["eu"] + float(np.log2(tint[0])), "ev_error_octaves": t["ev"] - r["ev"] + float(np.log2(tint[2]))}
    st.close()
    hip.hipFree(src), hip.hipFree(dst)
    out["build_id"] = R.state.build_id()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
