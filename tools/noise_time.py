"""Times the noise estimate at 1920x1080 on house with HIP events on one stream after warm-up (median of --reps): the snapshot (a
device-to-device copy of the accumulator), rsrt_noise_estimate (rt_noise_tile_kernel, default 16x16 tiles, and 8x8 / 64x64 beside it)
and, in the same run, the temporal pass as the yardstick of a streaming image-space pass, plus each one's unique bytes against its
time.  Also one render_to_noise run at a reduced size with its rounds.  Prints one JSON line and writes it to
profiles/noise_house_1080p.json (--out).
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threshold", type=float, default=2.0, help="of the render_to_noise run (480x270, at most 256 spp)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_house_1080p.json"))
    a = ap.parse_args()
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    env = R.Environment.synthetic(256, 128)
    st = R.State.new(scene, env, a.width, a.height)
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
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts))}

    n = a.width * a.height
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "reps": a.reps}

    # the yardstick first (it clears the accumulator): the temporal pass over a 1-spp frame and its AOV records
    p = R.state.TemporalParams(**R.state.TEMPORAL_DEFAULTS)
    st.render_temporal(1)
    out["temporal"] = timed(lambda: st._check(st._L.rsrt_temporal_accumulate(st._ctx, R.state._p(st.camera), 1, 1, C.byref(p), C.c_void_p(sp)),
                                              "rsrt_temporal_accumulate"))
    out["temporal"]["unique_bytes"] = n * (16 + 32 + 16 + 16 + 16 + 16)  # tools/temporal_time.py

    st.clear()
    st.render_samples(4)
    out["snapshot"] = timed(lambda: st.noise_snapshot(stream=sp))
    out["snapshot"]["unique_bytes"] = n * 32  # read 16, write 16
    st.render_samples(4)
    for tile in ((16, 16), (8, 8), (64, 64)):
        key = "estimate_%dx%d" % tile
        out[key] = timed(lambda: st.noise_estimate(tile, stream=sp, download=False))
        tiles, s = st.noise_download()
        out[key]["unique_bytes"] = n * 32 + tiles.size * 4  # the accumulator's and the snapshot's float4 a pixel, one float a tile
        out[key]["summary"] = s
    for k in ("temporal", "snapshot", "estimate_16x16", "estimate_8x8", "estimate_64x64"):
        out[k]["unique_GBps"] = out[k]["unique_bytes"] / (out[k]["ms_median"] * 1e-3) / 1e9
    out["estimate_over_temporal"] = out["estimate_16x16"]["ms_median"] / out["temporal"]["ms_median"]
    st.close()

    small = R.State.new(scene, env, a.width // 4, a.height // 4)
    small.max_bounces = a.bounces
    t0 = time.perf_counter()
    total, rounds = small.render_to_noise(a.threshold, min_samples=8, max_samples=256)
    small.synchronize()
    out["render_to_noise"] = {"width": a.width // 4, "height": a.height // 4, "threshold": a.threshold, "total": total, "host_ms": (time.perf_counter() - t0) * 1e3,
                              "rounds": [list(r) for r in rounds]}
    small.close()
    out["build_id"] = R.state.build_id()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
