"""AliasTable::build_by_luminance on the device (csrc/hip/rt_alias_device.h) against the host builder
rsrt_alias_table_build and the oracle's restatement: every field of every entry, bit for bit, on the 8x4, 64x32 and
2048x1024 environments — plus the CPU-side demonstration of WHY the sum and the pairing stay sequential."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host, state, types as T


def test_a_tree_reduction_is_not_the_reference_sum():
    """The counter-example that closes "bit-identical with a parallel sum": the reference adds the W*H weights left to
    right in f32 (src/environments.rs:110).  A pairwise (tree) f32 reduction of the same weights gives a different sum
    already on the 64x32 environment, and with it a different table (p = w*N/sum feeds every entry)."""
    env = R.Environment.synthetic(64, 32)
    rgb = env.rgba[:, :, :3]
    y = (np.arange(32, dtype=np.float32) + np.float32(0.5))
    row_sin = np.array([oracle.detmath("sin", float(np.float32(np.pi) * v / np.float32(32))) for v in y], np.float32)
    w = ((np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1]) + np.float32(0.0722) * rgb[..., 2]) * row_sin[:, None]
    w = w.astype(np.float32).reshape(-1)
    seq = np.float32(0)
    for v in w:
        seq = np.float32(seq + v)
    tree = w.copy()
    while len(tree) > 1:
        tree = (tree[0::2] + tree[1::2]).astype(np.float32)
    assert seq != tree[0], "this input happens to sum the same both ways: pick another counter-example"
    # and the table really is built from the sequential sum: reproduce entry pmfs of the small entries from it
    table, _ = R.AliasTable.build_by_luminance(rgb)
    p = (w * np.float32(len(w)) / seq).astype(np.float32)
    small = p < 1
    assert np.array_equal(table["pmf"][small & (table["alias_index"] != np.arange(len(w)))],
                          (p / np.float32(len(w))).astype(np.float32)[small & (table["alias_index"] != np.arange(len(w)))])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kind", [(8, 4, "sun"), (64, 32, "sun"), (2048, 1024, "sun"), (100, 37, "sun"), (256, 128, "flat"), (300, 200, "noise"), (64, 1, "flat"), (1, 1, "sun"), (128, 64, "wild"), (96, 48, "zero"), (512, 256, "spike"), (64, 64, "equal"),
                                      (2, 1, "noise"), (1, 2, "noise"), (2, 2, "noise"), (3, 2, "noise"), (1, 37, "noise"), (5, 3, "noise"), (5, 3, "zero"), (5, 3, "spike")])
def test_device_alias_table_is_the_host_table_bit_for_bit(w, h, kind):
    """kind: "sun" = the synthetic HDRI (a few hundred very large entries each pair with thousands of small ones: long runs of one
    large), "flat" = every texel within a few per cent of the mean (half the entries are larges that take one small or two and are
    used up: long chains of demoted larges), "noise" = log-uniform texels over four decades (everything in between),
    "wild" = the same with one texel in fifty negative (no HDRI has that; the device builder's shortcut for 1 - p <= 1 must step aside)."""
    rgba = host.synth_environment(w, h)
    if kind != "sun":
        rng = np.random.default_rng(w * 1000 + h)
        v = rng.uniform(0.97, 1.03, (h, w, 3)) if kind == "flat" else 10.0 ** rng.uniform(-2, 2, (h, w, 3))
        if kind == "wild":  # negative texels (weights below zero: 1 - p above 1) among ordinary ones
            v = np.where(rng.uniform(size=(h, w, 1)) < 0.02, -v, v)
        if kind == "zero":  # a black map: the sum is 0, every p is NaN, nothing is small
            v = np.zeros((h, w, 3))
        if kind == "spike":  # one lit texel in a black map: one large takes every small there is
            v = np.zeros((h, w, 3)); v[h // 3, w // 5] = 7.0
        if kind == "equal":  # the same colour everywhere (the weights still differ by row)
            v = np.full((h, w, 3), 0.5)
        rgba = np.ascontiguousarray(np.concatenate([v, np.zeros((h, w, 1))], axis=2).astype(np.float32))
    ref, left_ref = R.AliasTable.build_by_luminance(rgba[:, :, :3])
    oref, oleft = oracle.alias_table(rgba[:, :, :3])
    assert util.fields_equal(ref, oref) and left_ref == oleft
    L = state.lib()
    L.rsrt_environment_build_alias.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    sc = R.Scene.load_toml(util.scene_path("default"))
    st = R.State(0)
    st.upload_scene(sc)
    # alias = NULL: upload the texels and build on the device
    assert L.rsrt_upload_environment(st._ctx, 0, w, h, rgba.ctypes.data_as(C.c_void_p), None) == 0, L.rsrt_last_error(st._ctx)
    out = np.zeros(w * h, T.ALIAS_ENTRY)
    left = C.c_uint32(0)
    t = time.perf_counter()
    assert L.rsrt_environment_build_alias(st._ctx, 0, out.ctypes.data_as(C.c_void_p), out.size, C.byref(left)) == 0, L.rsrt_last_error(st._ctx)
    dt = time.perf_counter() - t
    t = time.perf_counter()
    R.AliasTable.build_by_luminance(rgba[:, :, :3])
    dt_host = time.perf_counter() - t
    print("alias table %dx%d: device %.1f ms (incl. copy back), host %.1f ms, leftover %d" % (w, h, dt * 1e3, dt_host * 1e3, left.value))
    assert left.value == left_ref
    for name in ("probability", "alias_index", "pmf"):
        a, b = out[name], ref[name]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    # and a render with the device-built table is the oracle's picture
    st.resize(64, 40)
    st.camera = np.array(sc.camera_uniform()).view(T.CAMERA).reshape(1).copy()
    st.render_samples(3)
    img = st.download()
    st.close()
    env = R.Environment(rgba, ref)
    want, _ = oracle.render(util.oracle_scene(sc), util.oracle_env(env), sc.camera_uniform().view(oracle.CAMERA), 64, 40, 0, 3, 10)
    assert np.array_equal(util.bits(img), util.bits(want))
