"""Times depth of field at 1920x1080 on house (4 spp with the AOV pass) with HIP events on one stream after 3 warm-up calls (median and
minimum of --reps): rsrt_dof — the prepare and the gather kernel together — at max_radius 4, 8 and 16 with the focus on the picture's
centre and an aperture that defocuses most of the frame; the same call with aperture 0 (every tile in focus: the prepare kernel, the
staging and one tap a pixel); and, in the same run, the default denoiser and a device-to-device copy of the W x H float4 image on that
stream.  Beside the times it records the floor of the tap loop from the published figures of the machine, not from the code under test:
taps x 16 B over the LDS array's bytes a clock and CU, and taps x the VALU operations of one tap over the FP32 rate.  Prints one JSON
line and writes it to profiles/dof_house_1080p.json (--out).  The per-kernel split comes from
rocprofv3 --kernel-trace --stats -- python tools/dof_time.py --reps 20 --radii R --skip-in-focus --out '' and is folded in with
--kernel-stats R=CSV (the kernels' averages over the 3 warm-up and the 20 timed calls).
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# the machine, from its published figures (MI355X: 256 CUs at 2.4 GHz; a CU's LDS moves 256 B a clock; a CU's four SIMD-32 units retire
# 128 FP32 lane-operations a clock without packing or fusing — 78.64 T a second, bench.py's roof) and the tap of include/rsrt_dof.h counted by hand: max, two compares and two selects for the
# occlusion rule, add, subtract and the clamp's two, the compare with 0, the weight's multiply, three multiplies and four adds = 19
CUS, CLOCK_HZ, LDS_BYTES_PER_CLK_CU, FP32_LANE_OPS_PER_CLK_CU, VALU_OPS_PER_TAP = 256, 2.4e9, 256, 128, 19


def floor_ms(pixels, radius):
    taps = pixels * (2 * radius + 1) ** 2
    return {"taps": taps, "lds_ms": taps * 16 / (LDS_BYTES_PER_CLK_CU * CUS * CLOCK_HZ) * 1e3,
            "valu_ms": taps * VALU_OPS_PER_TAP / (FP32_LANE_OPS_PER_CLK_CU * CUS * CLOCK_HZ) * 1e3}


def set_floors(out):
    """The floors of every radius in `out`, the whole pass over the larger one and, where the per-kernel split is there, the gather
    kernel alone over it."""
    n = out["width"] * out["height"]
    for k in [k for k in out if k.startswith("dof_radius_") and "aperture" not in k]:
        radius = int(k.rsplit("_", 1)[1])
        f = out[k]["floor"] = floor_ms(n, radius)
        floor = max(f["lds_ms"], f["valu_ms"])
        out[k]["over_floor"] = out[k]["ms_median"] / floor
        g = out.get("kernels_rocprofv3", {}).get("radius_%d" % radius, {}).get("rt_dof_gather_kernel")
        if g:
            out[k]["gather_over_floor"] = g["average_ns"] * 1e-6 / floor


def fold_kernel_stats(out, specs):
    """R=CSV ...: the prepare and gather kernels' rows of a rocprofv3 kernel_stats.csv taken with --radii R."""
    for spec in specs:
        radius, path = spec.split("=", 1)
        with open(path) as f:
            rows = [r for r in csv.DictReader(ln for ln in f if not ln.startswith("#"))]
        k = out.setdefault("kernels_rocprofv3", {}).setdefault("radius_%s" % radius, {})
        for r in rows:
            for name in ("rt_dof_prepare_kernel", "rt_dof_gather_kernel", "rt_dn_level_kernel", "rt_dn_prepare_kernel"):
                if name in r["Name"]:
                    e = k.setdefault(name, {"calls": 0, "total_ns": 0.0, "min_ns": None})
                    e["calls"] += int(r["Calls"])
                    e["total_ns"] += float(r["TotalDurationNs"])
                    e["min_ns"] = float(r["MinNs"]) if e["min_ns"] is None else min(e["min_ns"], float(r["MinNs"]))
        for e in k.values():
            e["average_ns"] = e["total_ns"] / e["calls"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="house")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radii", default="4,8,16")
    ap.add_argument("--aperture", type=float, default=0.05)
    ap.add_argument("--skip-in-focus", action="store_true", help="leave the aperture-0 calls out (under rocprofv3: one kind of gather a kernel name)")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="R=CSV: fold a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dof_house_1080p.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.loads(f.readline())
        out.pop("kernels_rocprofv3", None)
        fold_kernel_stats(out, a.kernel_stats)
        set_floors(out)
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

    n = a.width * a.height
    out = {"scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "samples": a.samples, "reps": a.reps, "aperture": a.aperture}
    st.render_samples(a.samples, aov=True)
    out["focus_distance"] = st.focus_at(a.width // 2, a.height // 2)
    nbytes = n * 16
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out["device_copy"] = timed(lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, sp))
    out["denoise_default"] = timed(lambda: st.denoise(download=False, stream=sp))
    for radius in [int(v) for v in a.radii.split(",")]:
        k = "dof_radius_%d" % radius
        out[k] = timed(lambda: st.depth_of_field(aperture=a.aperture, max_radius=radius, stream=sp))
        r = np.abs(st.dof_coc())
        out[k]["pixels_defocused"] = float((r > 0.5).mean())
        out[k]["pixels_at_max_radius"] = float((r >= radius).mean())
        out[k]["mean_abs_radius"] = float(r.mean())
        out[k]["over_denoise"] = out[k]["ms_median"] / out["denoise_default"]["ms_median"]
        if not a.skip_in_focus:
            out["dof_radius_%d_aperture_0" % radius] = timed(lambda: st.depth_of_field(aperture=0.0, max_radius=radius, stream=sp))
    set_floors(out)
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
