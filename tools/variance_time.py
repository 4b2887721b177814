"""Times the variance guidance at 1920x1080 on house, with 1-spp frames along a moving camera and HIP events on one stream after
warm-up: the MOMENTS temporal pass against the plain one, the variance-guided filter (prepare, clamp / variance pass and 5 levels) with
and without the clamp against the fixed filter, and a whole interactive frame (render 1 spp + AOV + MOMENTS temporal pass + the
variance-guided, clamped filter of its result).  Prints one JSON line and writes it to profiles/variance_house_1080p.json (--out).
The per-kernel split comes from a separate run under rocprofv3:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/variance_time.py --reps 5 --out ''
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_house_1080p.json"))
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

    def temporal_pass(flags):
        def run():
            st._check(st._L.rsrt_temporal_accumulate_ex(st._ctx, R.state._p(st.camera), 1, 1, C.byref(p), flags, C.c_void_p(sp)),
                      "rsrt_temporal_accumulate_ex")
        return run

    st.render_temporal(1)
    plain_ms = timed(temporal_pass(0), before=step)  # over the last frame's accumulator and AOV, the camera moved before each call
    st.render_temporal(1, moments=True)
    moments_ms = timed(temporal_pass(R.state.TEMPORAL_MOMENTS), before=step)

    def filt(**kw):
        return lambda: st.denoise(temporal=True, stream=sp, download=False, **kw)

    fixed_ms = timed(filt())
    variance_ms = timed(filt(variance=True))
    clamp_ms = timed(filt(variance=True, clamp=True))

    def frame():
        st.render_temporal(1, stream=sp, moments=True)
        st.denoise(temporal=True, variance=True, clamp=True, stream=sp, download=False)

    frame_ms = timed(frame, before=step)
    out = {"scene": a.scene, "width": a.width, "height": a.height,
           "temporal_ms_median": plain_ms[0], "temporal_ms_min": plain_ms[1],
           "temporal_moments_ms_median": moments_ms[0], "temporal_moments_ms_min": moments_ms[1],
           "fixed_filter_ms_median": fixed_ms[0], "fixed_filter_ms_min": fixed_ms[1],
           "variance_filter_ms_median": variance_ms[0], "variance_filter_ms_min": variance_ms[1],
           "variance_clamp_filter_ms_median": clamp_ms[0], "variance_clamp_filter_ms_min": clamp_ms[1],
           "frame_ms_median": frame_ms[0], "frame_ms_min": frame_ms[1],
           "filter": "prepare + %d levels of the temporal colour" % R.state.DENOISE_DEFAULTS["iterations"],
           "frame": "clear + render 1 spp + AOV 1 spp + MOMENTS temporal + variance-guided clamped %d-level filter"
                    % R.state.DENOISE_DEFAULTS["iterations"],
           "build_id": R.state.build_id()}
    st.close()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
