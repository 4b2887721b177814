"""Times camera motion blur at 1920x1080 on house (4 spp with the AOV pass) with HIP events on one stream after 3 warm-up calls (median
and minimum of --reps): rsrt_motion_blur — the prepare and the gather kernel together — at max_radius 4, 8 and 16 with 16 taps for a
pan that saturates the radius (the camera one frame earlier turned back by --yaw radians); the same calls with the camera held still
(every tile copied: the prepare kernel and a copy); and, in the same run, a device-to-device copy of the W x H float4 image and rsrt_dof
at radius 8 on that stream.  No time is fixed in advance; the pass is expected to cost less than rsrt_dof at the same radius (16 taps
against up to 1089) and the still camera about the prepare kernel plus a copy, and `expectations` says whether the figures agree.
Prints one JSON line and writes it to profiles/motion_house_1080p.json (--out).
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
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radii", default="4,8,16")
    ap.add_argument("--taps", type=int, default=16)
    ap.add_argument("--yaw", type=float, default=0.2, help="the pan of one frame, in radians")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_house_1080p.json"))
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

    n = a.width * a.height
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps, "taps": a.taps,
           "yaw": a.yaw, "shutter": R.state.MOTION_DEFAULTS["shutter"]}
    st.render_samples(a.samples, aov=True)
    nbytes = n * 16
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out["device_copy"] = timed(lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, sp))
    st.focus_at(a.width // 2, a.height // 2)
    out["dof_radius_8"] = timed(lambda: st.depth_of_field(aperture=0.05, max_radius=8, stream=sp))
    pan = R.state.camera_earlier(st.camera, a.yaw, 0.0)
    for radius in [int(v) for v in a.radii.split(",")]:
        k = "motion_radius_%d" % radius
        out[k] = timed(lambda: st.motion_blur("mean", pan, max_radius=radius, taps=a.taps, stream=sp))
        l = st.motion_velocity()[..., 2]
        out[k]["pixels_at_max_radius"] = float((l >= radius).mean())
        out[k]["mean_length"] = float(l.mean())
        out[k]["tiles_gathered"] = float((st.motion_tiles()[..., 2] >= 0.5).mean())
        out[k + "_still"] = timed(lambda: st.motion_blur("mean", st.camera, max_radius=radius, taps=a.taps, stream=sp))
        assert not st.motion_velocity().any()
    copy, dof8, m8 = out["device_copy"]["ms_median"], out["dof_radius_8"]["ms_median"], out.get("motion_radius_8", {}).get("ms_median")
    still = max(v["ms_median"] for k, v in out.items() if k.endswith("_still"))
    out["expectations"] = {"motion_radius_8_below_dof_radius_8": None if m8 is None else bool(m8 < dof8),
                           "motion_radius_8_over_dof_radius_8": None if m8 is None else m8 / dof8,
                           "still_over_device_copy": still / copy}
    st.close()
    hip.hipFree(src), hip.hipFree(dst)
    out["build_id"] = R.state.build_id()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
