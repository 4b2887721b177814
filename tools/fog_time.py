"""Times the volumetric fog pass at 1920x1080 on house with HIP events on one stream after 3 warm-up calls (median and minimum of
--reps): rsrt_fog_render of one sample at 8, 16 and 32 steps (jitter on, the light the synthetic map's sun), rsrt_fog_apply of the mean
and, for scale, in the same run, rsrt_aov_render of one sample — the same per-lane walk on the coherent camera rays.  The rates are
w h steps shadow queries (and w h camera rays for the AOV pass) over the median time.  No time is fixed in advance; `notes` says whether
the march's shadow-ray rate reaches the AOV pass's own rays per second.  Beside them, in the same run, fog at half size (DESIGN.md
§23): rsrt_fog_render at ceil(w / 2) x ceil(h / 2) at the same step counts and rsrt_fog_apply_upsampled of the mean at the full size,
with what they take of the full-size march and of rsrt_fog_apply.  Prints one JSON line and writes it to
profiles/fog_upsample_house_1080p.json (--out; profiles/fog_house_1080p.json holds the run before the half-size rows existed).
"""
import argparse
import ctypes as C
import json
import math
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", default="8,16,32")
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fog_upsample_house_1080p.json"))
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
    norm = math.sqrt(0.4 * 0.4 + 0.6 * 0.6 + 0.7 * 0.7)
    light = {"light_dir": (0.4 / norm, 0.6 / norm, -0.7 / norm), "light_irradiance": tuple(20.0 * math.pi * c for c in (1.0, 0.95, 0.85))}
    out = {"scene": a.scene, "width": a.width, "height": a.height, "reps": a.reps, "density": a.density, "samples": 1, "jitter": True}
    st.render_samples(1)
    out["aov_render"] = timed(lambda: st.render_aov(0, 1, stream=sp))
    out["aov_render"]["rays_per_s"] = n / (out["aov_render"]["ms_median"] * 1e-3)
    for steps in [int(v) for v in a.steps.split(",")]:
        k = "fog_render_%d_steps" % steps
        out[k] = timed(lambda: st.render_fog(1, 0, stream=sp, density=a.density, steps=steps, **light))
        st.clear_fog()
        st.render_fog(1, 0, density=a.density, steps=steps, **light)
        rec = st.download_fog()
        out[k]["shadow_rays_per_s"] = n * steps / (out[k]["ms_median"] * 1e-3)
        out[k]["rays_per_s"] = n * (steps + 1) / (out[k]["ms_median"] * 1e-3)  # the camera ray counted in
        out[k]["mean_transmittance"] = float(rec[..., 3].mean())
        out[k]["mean_inscatter"] = float(rec[..., :3].mean())
    out["fog_apply"] = timed(lambda: st.fog("mean", stream=sp))
    out["fog_apply"]["unique_bytes"] = n * 48  # the sum and the record read, the image written: a float4 each
    out["fog_apply"]["gb_per_s"] = n * 48 / (out["fog_apply"]["ms_median"] * 1e-3) / 1e9
    # fog at half size: the march over a quarter of the rays, and the rebuild at the full size in the place of rsrt_fog_apply
    hw, hh = (a.width + 1) // 2, (a.height + 1) // 2
    out["half_size"] = [hw, hh]
    for steps in [int(v) for v in a.steps.split(",")]:
        k = "fog_render_half_%d_steps" % steps
        out[k] = timed(lambda: st.render_fog(1, 0, stream=sp, size=(hw, hh), density=a.density, steps=steps, **light))
        out[k]["shadow_rays_per_s"] = hw * hh * steps / (out[k]["ms_median"] * 1e-3)
        out[k]["of_full_size"] = out[k]["ms_median"] / out["fog_render_%d_steps" % steps]["ms_median"]
    out["fog_apply_upsampled"] = timed(lambda: st.fog("mean", stream=sp, upsample=True))
    # the sum, the first-hit record and the image as before, the low records read and their source terms written and read
    out["fog_apply_upsampled"]["unique_bytes"] = n * 64 + hw * hh * 48
    out["fog_apply_upsampled"]["gb_per_s"] = out["fog_apply_upsampled"]["unique_bytes"] / (out["fog_apply_upsampled"]["ms_median"] * 1e-3) / 1e9
    out["fog_apply_upsampled"]["of_fog_apply"] = out["fog_apply_upsampled"]["ms_median"] / out["fog_apply"]["ms_median"]
    for steps in [int(v) for v in a.steps.split(",")]:
        full = out["fog_render_%d_steps" % steps]["ms_median"] + out["fog_apply"]["ms_median"]
        half = out["fog_render_half_%d_steps" % steps]["ms_median"] + out["fog_apply_upsampled"]["ms_median"]
        out["fog_render_half_%d_steps" % steps]["march_and_compose_gain"] = full / half
    rates = [v["shadow_rays_per_s"] for k, v in out.items() if k.startswith("fog_render_") and "half" not in k]
    out["notes"] = {"march_reaches_the_aov_ray_rate": bool(min(rates) >= out["aov_render"]["rays_per_s"]),
                    "march_over_aov_ray_rate": [r / out["aov_render"]["rays_per_s"] for r in rates]}
    st.close()
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
