"""rsrt_sincosf on the device.  The fused sine and cosine (include/rsrt_detmath.h) against the two separate functions for all 2^32
inputs (rsrt_selftest_sincos), and the render kernels that use it — the flat kernel, the fixed-order walk and the cooperative walk —
against the checker, bit for bit with the checker's ray counts, on a power-of-two map (sample_environment_finish splits a pick into
column and row by mask and shift) and on a 100 x 37 one (by division): the pixel jitter of start_path, theta and phi of an environment pick with the sine the
solid angle takes over, and the azimuth both BSDF lobes share, drawn once ahead of the lobe branch."""
import functools

import numpy as np
import pytest

import oracle
import util
import rsoderh_raytracing_amd as R

pytestmark = pytest.mark.gpu

F = np.float32
# name, width, height, samples, bounces
FRAMES = [("house", 64, 36, 4, 8), ("default", 48, 48, 4, 3), ("spheres_only", 32, 32, 2, 4)]
ENVS = [(64, 32), (100, 37)]
# RSRT_TRAVERSAL / RSRT_FLAT as tests/test_gpu_parity.py forces them: the product's choice (these scenes: the flat kernel), the fixed-order
# walk, the cooperative walk
KERNELS = {"flat": {}, "fixed-order walk": {"RSRT_TRAVERSAL": "3", "RSRT_FLAT": "0"}, "cooperative walk": {"RSRT_TRAVERSAL": "6", "RSRT_FLAT": "0"}}
LAST_SAMPLE = 0xfffffffe  # the last sample index rsrt_render accepts (begin + count must not reach 2^32: tests/test_scene_edges_gpu.py)


@functools.lru_cache(maxsize=None)
def scene(name):
    return R.Scene.load_toml(util.scene_path(name))


@functools.lru_cache(maxsize=None)
def env(size):
    return R.Environment.synthetic(*size)


@functools.lru_cache(maxsize=None)
def reference(name, w, h, begin, count, mb, size):
    sc = scene(name)
    return oracle.render(util.oracle_scene(sc), util.oracle_env(env(size)), sc.camera_uniform().view(oracle.CAMERA), w, h, begin, count, mb)


def lobe_probabilities(materials):
    """(spec_prob, diff_prob) of every material, as rsrt_upload_scene forms them (rsrt_api.hip make_material_record)"""
    t = np.clip(materials["metallic"].astype(F), F(0), F(1))
    f0 = (F(1) - t)[:, None] * F(0.04) + t[:, None] * materials["color"].astype(F)
    ps = np.clip(F(0.2126) * f0[:, 0] + F(0.7152) * f0[:, 1] + F(0.0722) * f0[:, 2], F(0), F(1))
    return ps, F(1) - ps


def render(name, w, h, begin, count, mb, size):
    st = R.State.new(scene(name), env(size), w, h)
    try:
        st.max_bounces = mb
        st.render_range(begin, count)
        return st.download(), st.stats()
    finally:
        st.close()


def check(name, w, h, begin, count, mb, size, kernel):
    ref, ost = reference(name, w, h, begin, count, mb, size)
    img, s = render(name, w, h, begin, count, mb, size)
    same = util.bits(img) == util.bits(ref)
    assert same.all(), (name, size, kernel, int((~same).any(axis=2).sum()))
    assert (s["paths"], s["ext_rays"], s["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"]), (name, size, kernel)
    assert (s["traversal_steps"] == 0) == (kernel == "flat"), (name, kernel, s["traversal_steps"])  # the flat loop counts no steps, the walks do
    return ost


def test_fused_form_equals_sin_and_cos_for_every_input():
    st = R.State.new(scene("spheres_only"), env((64, 32)), 16, 16)
    try:
        r = st.selftest_sincos()
    finally:
        st.close()
    assert r["checked"] == 1 << 32, r
    assert r["mismatches"] == 0, "first failing input %08x" % r["first_bad"]
    assert r["first_bad"] == (1 << 64) - 1, r


@pytest.mark.parametrize("size", ENVS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_renders_keep_the_checkers_bits(kernel, size, monkeypatch):
    for name, _, _, _, _ in FRAMES:  # both lobes, and so the pair drawn ahead of their branch, are exercised
        ps, pd = lobe_probabilities(scene(name).materials)
        assert ((ps > 0) & (pd > 0)).any(), name
    for k, v in KERNELS[kernel].items():
        monkeypatch.setenv(k, v)
    for name, w, h, spp, mb in FRAMES:
        ost = check(name, w, h, 0, spp, mb, size, kernel)
        assert ost["shadow_rays"] > 0, name  # environment picks were made


@pytest.mark.parametrize("begin", [0, LAST_SAMPLE])
def test_one_sample_at_the_ends_of_the_index_range(begin, monkeypatch):
    """start_path's pair at the sample-index edges: one sample a pixel, index 0 and the last one, every kernel."""
    for kernel, knobs in KERNELS.items():
        with monkeypatch.context() as m:
            for k, v in knobs.items():
                m.setenv(k, v)
            check("house", 64, 36, begin, 1, 8, (64, 32), kernel)
