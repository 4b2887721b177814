"""Times the procedural sky against the host path it replaces, at 2048x1024 and 4096x2048 (and 512x256), on one context.  Every timed call ends in a
device synchronise (the library's calls are synchronous), so the clock is the host's around the call; 3 warm-up rounds, then --reps
rounds in which the calls alternate, median and minimum of each:
  sky_call       rsrt_environment_sky: free and allocate the slot, the two fill kernels, the device alias builder, the packing
  alias_build    rsrt_environment_build_alias alone on the filled slot (it packs too)
  the host path  rsrt_synth_environment (CPU), the host alias builder rsrt_alias_table_build (CPU), rsrt_upload_environment with that
                 table (64 MiB over the bus at 2048x1024, and the packing), and their sum: what a change of the environment costs today
  upload_no_table  rsrt_upload_environment with alias NULL: texels over the bus, table on the device
  sky_fill_host, alias_table_build_host_sky   rsrt_sky_fill (CPU) and the host alias builder over its texels: what the same sky would
                 cost through the host path (both alias builders take a time that depends on the texels, not only on their number)
A third, small size (512x256) shows what a sun that moves every frame can afford today.
Prints one JSON line and writes it to profiles/sky_house_1080p.json (--out; the name keeps the pattern of the other passes' profiles,
the content is the environment sizes).  The per-kernel split — the fill kernel on its own — comes from
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/sky_time.py --device-only --sizes WxH --reps 10 --out ''
and is folded in with --kernel-stats WxH=CSV (the kernels' averages over the warm-up and the timed calls).
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SKY_KERNELS = ("rt_sky_shares_kernel", "rt_sky_fill_kernel")
ALIAS_KERNELS = ("rt_alias_weights_kernel", "rt_alias_sum_kernel", "rt_alias_normalise_kernel", "rt_alias_scan_kernel", "rt_alias_scatter_kernel",
                 "rt_alias_vose_kernel", "rt_alias_pmf_kernel", "rt_env_pack_texels_kernel", "rt_env_pack_alias_kernel")


def fold_kernel_stats(out, specs):
    """WxH=CSV ...: the sky's and the alias builder's rows of a rocprofv3 kernel_stats.csv taken with --device-only --sizes WxH."""
    for spec in specs:
        size, path = spec.split("=", 1)
        with open(path) as f:
            rows = [r for r in csv.DictReader(ln for ln in f if not ln.startswith("#"))]
        k = out.setdefault("kernels_rocprofv3", {}).setdefault(size, {})
        for r in rows:
            for name in SKY_KERNELS + ALIAS_KERNELS:
                if name in r["Name"]:
                    k[name] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"])}
        w, h = (int(v) for v in size.split("x"))
        if "rt_sky_fill_kernel" in k:
            # the floor of the fill is its store: 16 B a texel at the device's published 8 TB/s
            k["fill_store_floor_ns"] = w * h * 16 / 8.0e12 * 1e9
            k["fill_over_store_floor"] = k["rt_sky_fill_kernel"]["average_ns"] / k["fill_store_floor_ns"]
        k["sky_kernels_ns"] = sum(k[n]["average_ns"] for n in SKY_KERNELS if n in k)
        k["alias_kernels_ns"] = sum(k[n]["average_ns"] for n in ALIAS_KERNELS if n in k)


def summary(ts):
    ms = [t * 1e3 for t in ts]
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_all": [round(t, 4) for t in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x256,2048x1024,4096x2048")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--device-only", action="store_true", help="the sky call and the alias build alone (under rocprofv3)")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="WxH=CSV: fold a rocprofv3 kernel_stats.csv into --out and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky_house_1080p.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.loads(f.readline())
        fold_kernel_stats(out, a.kernel_stats)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        return
    import rsoderh_raytracing_amd as R
    from rsoderh_raytracing_amd import host as H
    st = R.State()
    L = st._L
    L.rsrt_environment_build_alias.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    out = {"reps": a.reps, "params": "SKY_DEFAULTS", "sizes": {}}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        kept = {}

        def sky_call():
            st.environment_sky(0, w, h)

        def alias_build():
            st._check(L.rsrt_environment_build_alias(st._ctx, 0, None, 0, None), "rsrt_environment_build_alias")

        def synth():
            kept["rgba"] = H.synth_environment(w, h)

        def host_alias():
            kept["env"] = R.Environment(kept["rgba"])

        def upload():
            st.upload_environment(1, kept["env"])

        def upload_no_table():
            rgba = kept["rgba"]
            st._check(L.rsrt_upload_environment(st._ctx, 1, w, h, rgba.ctypes.data_as(C.c_void_p), None), "rsrt_upload_environment")

        def sky_fill_host():
            kept["sky"] = H.sky_fill(w, h)

        def host_alias_sky():
            R.Environment(kept["sky"])

        steps = [("sky_call", sky_call), ("alias_build", alias_build)]
        if not a.device_only:
            steps += [("synth_environment_host", synth), ("alias_table_build_host", host_alias), ("upload_environment", upload),
                      ("upload_no_table", upload_no_table), ("sky_fill_host", sky_fill_host), ("alias_table_build_host_sky", host_alias_sky)]
        times = {n: [] for n, _ in steps}
        for rep in range(3 + a.reps):  # the calls alternate within a round; the first 3 rounds are warm-up
            for n, fn in steps:
                st.synchronize()
                t0 = time.perf_counter()
                fn()
                st.synchronize()
                if rep >= 3:
                    times[n].append(time.perf_counter() - t0)
        r = {n: summary(ts) for n, ts in times.items()}
        r["texels_mib"] = w * h * 16 / 2.0 ** 20
        if not a.device_only:
            r["host_path_ms_median"] = sum(r[n]["ms_median"] for n in ("synth_environment_host", "alias_table_build_host", "upload_environment"))
            r["sky_call_over_upload"] = r["sky_call"]["ms_median"] / r["upload_environment"]["ms_median"]
            r["sky_call_over_host_path"] = r["sky_call"]["ms_median"] / r["host_path_ms_median"]
            r["sky_through_host_path_ms_median"] = sum(r[n]["ms_median"] for n in ("sky_fill_host", "alias_table_build_host_sky", "upload_environment"))
            assert np.array_equal(st.environment_download(0).view(np.uint32), H.sky_fill(w, h).view(np.uint32))  # what was timed is the sky
        out["sizes"][size] = r
    st.close()
    out["build_id"] = R.state.build_id()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
