"""Times the temporal pass at 1920x1080 on house, with 1-spp frames along a moving camera and HIP events on one stream after warm-up:
the pass alone, and a whole interactive frame (render 1 spp + AOV + temporal pass + the default 5-level filter of its result), plus
the pass's unique bytes against its time.  Prints one JSON line and writes it to profiles/temporal_house_1080p.json (--out).  The
per-kernel split comes from a separate run under rocprofv3:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/temporal_time.py --reps 5 --out ''
"""
import argparse
import ctypes as C
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_house_1080p.json"))
    a = ap.parse_args()
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(ROOT, "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces
    desc = np.array(scene.camera_desc).view(R.types.CAMERA_DESC).reshape(1).copy()

    def step():  # the camera pans a little every frame, so every pass reprojects
        desc["yaw"] += np.float32(0.002)
        st.camera = np.array(R.camera_uniform(desc)).view(R.types.CAMERA).reshape(1).copy()

    # HIP events on a stream of our own, from the HIP runtime librsrt.so is linked against
    maps = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln}, key=lambda q: "torch" in q)
    hip = C.CDLL(maps[0])  # (torch's copy only when torch was loaded first: the loader then gave librsrt that one)
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    sp = stream.value

    def timed(fn, before=None):
        for _ in range(3):  # warm-up
            if before:
                before()
            fn()
        st.synchronize()
        ts = []
        for _ in range(a.reps):
            if before:
                before()
            st.synchronize()
            hip.hipEventRecord(ev0, stream)
            fn()
            hip.hipEventRecord(ev1, stream)
            assert hip.hipEventSynchronize(ev1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ts.append(t.value)
        return float(np.median(ts)), float(np.min(ts))

    p = R.state.TemporalParams(**R.state.TEMPORAL_DEFAULTS)

    def temporal_pass():
        st._check(st._L.rsrt_temporal_accumulate(st._ctx, R.state._p(st.camera), 1, 1, C.byref(p), C.c_void_p(sp)), "rsrt_temporal_accumulate")

    st.render_temporal(1)
    pass_ms = timed(temporal_pass, before=step)  # over the last frame's accumulator and AOV, the camera moved before each call

    def frame():
        st.render_temporal(1, stream=sp)
        st.denoise(temporal=True, stream=sp, download=False)

    frame_ms = timed(frame, before=step)
    n = a.width * a.height
    # unique bytes of the pass: the sum (16) and the AOV record (32), the previous history and features (16 + 16: each is read about once,
    # the 4 taps of neighbouring pixels overlap), the new history and features (16 + 16)
    unique = n * (16 + 32 + 16 + 16 + 16 + 16)
    out = {"scene": a.scene, "width": a.width, "height": a.height, "temporal_ms_median": pass_ms[0], "temporal_ms_min": pass_ms[1],
           "frame_ms_median": frame_ms[0], "frame_ms_min": frame_ms[1],
           "frame": "clear + render 1 spp + AOV 1 spp + temporal + %d-level filter" % R.state.DENOISE_DEFAULTS["iterations"],
           "temporal_unique_bytes": unique, "temporal_unique_GBps": unique / (pass_ms[0] * 1e-3) / 1e9, "build_id": R.state.build_id()}
    st.close()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
