"""Times the denoiser at 1920x1080 on house: the AOV pass at 1 spp and the default 5-level filter, with HIP events on one stream
after warm-up, plus the filter's bytes moved against its kernel time.  Prints one JSON line; --png DIR also writes the noisy and the
denoised 4-spp frame as PNGs.  The per-kernel split comes from a separate run under rocprofv3:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/denoise_time.py --reps 5
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4, help="samples of the frame the filter denoises")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--png", default=None)
    a = ap.parse_args()
    import rsoderh_raytracing_amd as R
    scene = R.Scene.load_toml(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "assets", "scenes", a.scene + ".toml"))
    st = R.State.new(scene, R.Environment.synthetic(256, 128), a.width, a.height)
    st.max_bounces = a.bounces
    st.render_samples(a.spp, aov=True)
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
            hip.hipEventRecord(ev0, stream)
            fn()
            hip.hipEventRecord(ev1, stream)
            assert hip.hipEventSynchronize(ev1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
            ts.append(t.value)
        return float(np.median(ts)), float(np.min(ts))

    aov_ms = timed(lambda: st.render_aov(0, 1, stream=sp))
    st.clear_aov()
    st.render_aov(0, a.spp)
    filt_ms = timed(lambda: st.denoise(stream=sp, download=False))
    n = a.width * a.height
    it = R.state.DENOISE_DEFAULTS["iterations"]
    # unique bytes: prepare reads the sums + AOV records and writes colour + features; a level reads colour + features and writes
    # colour; the last also reads the AOV records again (remodulation)
    unique = n * (16 + 32 + 16 + 8) + it * n * (16 + 8 + 16) + n * 32
    taps = n * 25 * it * (16 + 8)  # what the levels' loads request (L1 / L2 / Infinity Cache hits included)
    out = {"scene": a.scene, "width": a.width, "height": a.height, "aov_1spp_ms_median": aov_ms[0], "aov_1spp_ms_min": aov_ms[1],
           "filter_ms_median": filt_ms[0], "filter_ms_min": filt_ms[1], "iterations": it, "filter_unique_bytes": unique,
           "filter_unique_GBps": unique / (filt_ms[0] * 1e-3) / 1e9, "filter_tap_bytes": taps,
           "filter_tap_GBps": taps / (filt_ms[0] * 1e-3) / 1e9, "build_id": R.state.build_id()}
    if a.png:
        os.makedirs(a.png, exist_ok=True)
        R.host.write_png(os.path.join(a.png, "%s_%dspp_noisy.png" % (a.scene, a.spp)), st.display_srgb8())
        st.denoise()
        R.host.write_png(os.path.join(a.png, "%s_%dspp_denoised.png" % (a.scene, a.spp)), st.denoised_display_srgb8())
    st.close()
    hip.hipEventDestroy(ev0), hip.hipEventDestroy(ev1), hip.hipStreamDestroy(stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
