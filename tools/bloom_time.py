"""Times bloom at 1920x1080 on house with HIP events on one stream after 3 warm-up calls (median and minimum of --reps): rsrt_bloom at
1, 3 and 6 levels at the metered exposure and, in the same run, a device-to-device copy of the same W x H float4 image on that stream
— the yardstick: the first level cannot beat one read of the source.  The bloomed display against the exposed one is timed on the
host clock: both calls run their kernel on the context's stream, copy 8 MB to the host and wait.  Prints one JSON line and writes it
to profiles/bloom_house_1080p.json (--out).  The per-kernel split comes from
rocprofv3 --kernel-trace --stats -- python tools/bloom_time.py --reps 5 --out ''.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_house_1080p.json"))
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
    st.render_samples(a.samples)
    r = st.auto_exposure()
    out["exposure"] = r["exposure"]
    # the yardstick: the accumulator's bytes copied device to device on the same stream
    nbytes = n * 16
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
    acc = st.download()
    assert hip.hipMemcpy(src, acc.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out["device_copy"] = timed(lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, sp))
    out["device_copy"]["unique_bytes"] = 2 * nbytes  # read 16, write 16
    half = ((a.width + 1) // 2) * ((a.height + 1) // 2)
    for levels in (1, 3, 6):
        k = "bloom_%d_levels" % levels
        out[k] = timed(lambda: st.bloom(levels=levels, stream=sp))
        out[k]["launches"] = 2 * levels
        out[k]["over_device_copy"] = out[k]["ms_median"] / out["device_copy"]["ms_median"]
    out["bloom_1_levels"]["unique_bytes"] = nbytes + 4 * half * 16  # the source read; D_1 written and read, B written (and nothing else)
    st.bloom()
    b = st.bloom_download()
    out["bloom_max"] = float(b[..., :3].max())
    out["bloom_texels_above_zero"] = int(np.count_nonzero(b[..., :3].max(axis=-1)))
    out["display_exposed"] = host_timed(lambda: st.display_exposed_srgb8())
    out["display_bloomed"] = host_timed(lambda: st.display_bloomed_srgb8())
    shown, plain = st.display_bloomed_srgb8(), st.display_exposed_srgb8()
    out["display_pixels_changed"] = int(np.count_nonzero((shown != plain).any(axis=-1)))
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
