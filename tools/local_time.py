"""Times local exposure at 1920x1080 on house with HIP events on one stream after 3 warm-up calls (median and minimum of --reps):
rsrt_local_exposure at cells 8, 16, 32 and 64 and, in the same run, a device-to-device copy of the same W x H float4 image on that
stream — the yardstick: the build reads the source once.  The graded display against the exposed one is timed on the host clock: both
calls run their kernel on the context's stream, copy 8 MB to the host and wait.  Then the picture: house at --picture-width x
--picture-height, --picture-samples samples, metered exposure — the share of pixels with a channel at byte 255 and the share with
every channel below byte 16, with and without the local exposure.  Prints one JSON line and writes it to
profiles/local_house_1080p.json (--out); the line carries the library's build id, which names an experiment build made through
RSRT_HIPCC_FLAGS.  The per-kernel split comes from
rocprofv3 --kernel-trace --stats -- python tools/local_time.py --reps 5 --out ''.
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
    ap.add_argument("--picture-width", type=int, default=960)
    ap.add_argument("--picture-height", type=int, default=540)
    ap.add_argument("--picture-samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_house_1080p.json"))
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
    for cell in R.state.LOCAL_CELLS:
        k = "local_exposure_cell_%d" % cell
        out[k] = timed(lambda: st.local_exposure(cell=cell, stream=sp))
        grid, _ = st.local_exposure_download()
        out[k]["launches"] = 2
        out[k]["grid_bytes"] = int(grid.nbytes)
        out[k]["unique_bytes"] = nbytes + 3 * int(grid.nbytes)  # the source read; the raw grid written and read, the blurred one written
        out[k]["over_device_copy"] = out[k]["ms_median"] / out["device_copy"]["ms_median"]
        out[k]["cells_counted_into"] = int(np.count_nonzero(grid[..., 0]))
    st.local_exposure()
    out["display_exposed"] = host_timed(lambda: st.display_exposed_srgb8())
    out["display_local"] = host_timed(lambda: st.display_local_srgb8())
    st.bloom()
    out["display_bloomed"] = host_timed(lambda: st.display_bloomed_srgb8())
    out["display_local_bloomed"] = host_timed(lambda: st.display_local_srgb8(bloom_intensity=R.state.BLOOM_DEFAULTS["intensity"]))
    gain = st.local_gain()
    out["gain_min"], out["gain_max"] = float(gain.min()), float(gain.max())
    st.close()
    hip.hipFree(src), hip.hipFree(dst)
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)

    # the picture
    pw, ph = a.picture_width, a.picture_height
    st = R.State.new(scene, R.Environment.synthetic(2048, 1024), pw, ph)
    st.max_bounces = a.bounces
    st.render_samples(a.picture_samples)
    r = st.auto_exposure()
    st.local_exposure()

    def shares(img):
        rgb = img[..., :3]
        return {"clipped_share": float((rgb == 255).any(axis=-1).mean()), "dark_share": float((rgb < 16).all(axis=-1).mean()),
                "mean_byte": float(rgb.mean())}
    gain = st.local_gain()
    out["picture"] = {"width": pw, "height": ph, "samples": a.picture_samples, "exposure": r["exposure"], "average_luminance": r["average_luminance"],
                      "exposed": shares(st.display_exposed_srgb8()), "local": shares(st.display_local_srgb8()),
                      "local_strength_1": shares(st.display_local_srgb8(shadows=1.0, highlights=1.0)),
                      "gain_min": float(gain.min()), "gain_max": float(gain.max()), "gain_above_one_share": float((gain > 1).mean()),
                      "gain_below_one_share": float((gain < 1).mean())}
    st.close()
    out["build_id"] = R.state.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
