"""Times auto-exposure at 1920x1080 on house with HIP events on one stream after 3 warm-up calls (median and minimum of --reps):
rsrt_exposure_meter (rt_exposure_hist_kernel with the zeroing of its histogram) on the rendered frame and on a frame of one constant
colour — every wave's 64 pixels in one bin, the contention case — and, in the same run, rsrt_noise_estimate at 16x16 tiles as the
yardstick and the snapshot copy, each one's unique bytes against its time.  The exposed display against the plain one is timed on
the host clock: both calls run their kernel on the context's stream, copy 8 MB to the host and wait.  Prints one JSON line and
writes it to profiles/exposure_house_1080p.json (--out).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_house_1080p.json"))
    a = ap.parse_args()
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
    half = a.samples // 2
    st.render_samples(half)
    out["snapshot"] = timed(lambda: st.noise_snapshot(stream=sp))
    out["snapshot"]["unique_bytes"] = n * 32  # read 16, write 16
    st.render_samples(a.samples - half)
    out["noise_estimate_16x16"] = timed(lambda: st.noise_estimate((16, 16), stream=sp, download=False))
    out["noise_estimate_16x16"]["unique_bytes"] = n * 32 + st.noise_download()[0].size * 4
    out["meter_rendered"] = timed(lambda: st.exposure_meter(stream=sp))
    out["meter_rendered"]["unique_bytes"] = n * 16 + 257 * 4
    hist, r = st.exposure_download()
    out["meter_rendered"]["result"] = r
    out["meter_rendered"]["bins_in_use"] = int(np.count_nonzero(hist[:256]))
    out["display_plain"] = host_timed(lambda: st.display_srgb8())
    out["display_exposed"] = host_timed(lambda: st.display_exposed_srgb8("mean", r["exposure"]))

    # one constant colour, in caller-owned memory (the bind frees the State's own accumulator: this comes last)
    const = np.ones((a.height, a.width, 4), np.float32)
    const[..., :3] = (0.8, 0.4, 0.1)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(const.nbytes)) == 0
    assert hip.hipMemcpy(ptr, const.ctypes.data_as(C.c_void_p), C.c_size_t(const.nbytes), 1) == 0
    st.bind_accumulator(ptr.value, a.width, a.height)
    out["meter_constant"] = timed(lambda: st.exposure_meter(sample_total=1, stream=sp))
    out["meter_constant"]["unique_bytes"] = n * 16 + 257 * 4
    hist, r = st.exposure_download()
    assert np.count_nonzero(hist) == 1 and int(hist.max()) == n
    out["meter_constant"]["result"] = r
    for k in ("snapshot", "noise_estimate_16x16", "meter_rendered", "meter_constant"):
        out[k]["unique_GBps"] = out[k]["unique_bytes"] / (out[k]["ms_median"] * 1e-3) / 1e9
    out["meter_over_noise_estimate"] = out["meter_rendered"]["ms_median"] / out["noise_estimate_16x16"]["ms_median"]
    out["constant_over_rendered"] = out["meter_constant"]["ms_median"] / out["meter_rendered"]["ms_median"]
    st.close()
    hip.hipFree(ptr)
    out["build_id"] = R.state.build_id()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
