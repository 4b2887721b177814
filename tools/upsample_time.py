"""Times guided upsampling on house, output 1920x1080 from a 960x540 low frame: the guide pass per sample, rsrt_upsample (the low
prepare pass + rt_up_kernel), the whole interactive frame (clears, 4 spp low + AOV pass + guide + denoise + upsample) and, in the same
run, what the same number of paths costs without it (clears, 1 spp at 1080p + AOV pass + denoise) — HIP events on one stream after
warm-up, and a host clock around the same work ending in a synchronise.  Prints one JSON line; --out FILE also writes it.  The
per-kernel split (rt_up_kernel, the low prepare pass, an a-trous level at either size) comes from a separate run under the profiler,
whose per-dispatch trace a second, unprofiled run folds into its JSON:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/upsample_time.py --reps 5
    python tools/upsample_time.py --kernel-trace OUT/.../*_kernel_trace.csv --out profiles/upsample_house_1080p.json
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def kernel_split(path, low, full):
    """Median / minimum duration (us) per kernel and frame size from a rocprofv3 kernel trace: {label: {"us_median", "us_min", "calls"}}."""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            gx, gy = int(row["Grid_Size_X"]), int(row["Grid_Size_Y"])
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            for size, label in ((low, "low"), (full, "full")):
                n = size[0] * size[1]
                bx, by = (size[0] + 63) // 64, (size[1] + 3) // 4  # 64 x 4 workgroups over the frame; 256-thread blocks over its pixels
                rows_2d = (gx, gy) in ((bx * 64, by * 4), (bx, by))  # (a grid in work-items, or in workgroups)
                flat = gy == 1 and gx in ((n + 255) // 256 * 256, (n + 255) // 256)
                key = None
                if "rt_up_kernel" in name and rows_2d and label == "full":
                    key = "rt_up_kernel"
                elif "rt_dn_level_kernel" in name and rows_2d:
                    key = "rt_dn_level_kernel_" + label
                elif "rt_dn_prepare_kernel" in name and flat:
                    key = "rt_dn_prepare_kernel_" + label
                if key:
                    groups.setdefault(key, []).append(us)
    return {k: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "calls": len(v)} for k, v in sorted(groups.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920, help="output size")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4, help="samples of the low frame and of the guide")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel trace (csv) of an earlier run of this tool")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rsoderh_raytracing_amd as R
    W, H = a.width, a.height
    w, h = (W + 1) // 2, (H + 1) // 2
    scene = R.Scene.load_toml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    env = R.Environment.synthetic(256, 128)
    st = R.State.new(scene, env, w, h)      # traces at the low size
    full = R.State.new(scene, env, W, H)    # what there was before: every path at the output size
    st.max_bounces = full.max_bounces = a.bounces
    # HIP events on a stream of our own, from the HIP runtime librsrt.so is linked against
    maps = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln}, key=lambda q: "torch" in q)
    hip = C.CDLL(maps[0])  # (torch's copy only when torch was loaded first: the loader then gave librsrt that one)
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    sp = stream.value

    def timed(fn, sync):
        for _ in range(3):  # warm-up
            fn()
        sync()
        ev, wall = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            hip.hipEventRecord(ev0, stream)
            fn()
            hip.hipEventRecord(ev1, stream)
            assert hip.hipEventSynchronize(ev1) == 0
            sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ev.append(t.value)
        return {"ms_median": float(np.median(ev)), "ms_min": float(np.min(ev)), "host_ms_median": float(np.median(wall))}

    def frame_upsampled():
        st.clear()
        st.clear_aov()
        st.clear_guide()
        st.render_range(0, a.spp, stream=sp)
        st.render_aov(0, a.spp, stream=sp)
        st.render_guide(W, H, 0, a.spp, stream=sp)
        st.denoise(sample_total=a.spp, aov_sample_total=a.spp, stream=sp, download=False)
        st.upsample("denoised", aov_sample_total=a.spp, guide_sample_total=a.spp, stream=sp, download=False)

    def frame_full():
        full.clear()
        full.clear_aov()
        full.render_range(0, 1, stream=sp)
        full.render_aov(0, 1, stream=sp)
        full.denoise(sample_total=1, aov_sample_total=1, stream=sp, download=False)

    st.render_aov(0, 1)
    st.render_guide(W, H, 0, 1)
    full.render_aov(0, 1)
    frame_upsampled()
    frame_full()
    out = {"scene": a.scene, "width": W, "height": H, "low_width": w, "low_height": h, "spp": a.spp, "bounces": a.bounces, "reps": a.reps,
           "guide_1spp": timed(lambda: st.render_guide(W, H, 0, 1, stream=sp), st.synchronize),
           "aov_low_1spp": timed(lambda: st.render_aov(0, 1, stream=sp), st.synchronize)}
    frame_upsampled()  # (the two passes above left other sample counts behind)
    out["upsample_call"] = timed(lambda: st.upsample("denoised", aov_sample_total=a.spp, guide_sample_total=a.spp, stream=sp, download=False), st.synchronize)
    out["denoise_low"] = timed(lambda: st.denoise(sample_total=a.spp, aov_sample_total=a.spp, stream=sp, download=False), st.synchronize)
    out["denoise_full"] = timed(lambda: full.denoise(sample_total=1, aov_sample_total=1, stream=sp, download=False), full.synchronize)
    out["frame_upsampled_%dspp_low" % a.spp] = timed(frame_upsampled, st.synchronize)
    out["frame_full_1spp"] = timed(frame_full, full.synchronize)
    n_lo, n_hi = w * h, W * H
    # rt_up_kernel's unique bytes: the low colour + features once, the guide record and the output per output pixel; what its taps request
    out["up_unique_bytes"] = n_lo * (16 + 8) + n_hi * (32 + 16)
    out["up_tap_bytes"] = n_hi * 9 * (16 + 8)
    if a.kernel_trace:
        out["kernels"] = kernel_split(a.kernel_trace, (w, h), (W, H))
        up = out["kernels"].get("rt_up_kernel")
        if up:
            out["up_unique_GBps"] = out["up_unique_bytes"] / (up["us_median"] * 1e-6) / 1e9
    out["build_id"] = R.state.build_id()
    st.close()
    full.close()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
