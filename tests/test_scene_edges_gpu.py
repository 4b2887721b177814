"""The render kernels, the ray probe, the AOV pass and the device BVH builder on the edge cases of tests/edge_scenes.py, against the
checker (test_scene_edges.py shows without a GPU that each case reaches its edge).  Image sums are compared bit for bit, a NaN of the
checker's being a NaN in the same element (util.same_bits_or_nan; edge_scenes' docstring lists the cases that hold any), and the ray
counts must match: every case under the default kernel selection and under the forced cooperative walk, a subset through the small
form and the other traversals, with and without FLAG_REFERENCE_TRAVERSAL."""
import numpy as np
import pytest

import bvh_ref
import denoise_ref as D
import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in E.cases()]
FLAGS = (0, R.state.FLAG_REFERENCE_TRAVERSAL)
# the cold-reciprocal case, one scale-subnormal and one scale-overflow case, the material grid, the pole camera: through the small form and the other traversals
SUBSET = ["cold_rcp_huge_triangle", "scale_default_2^-70_sky", "scale_default_2^64_sky"] + [c.name for c in E.family("materials")] + ["camera_fov_1e-4_pole_down"]
FORMS = [("2", "6"), ("2", "4"), ("4", "4"), ("2", "4-noflat"), ("2", "3"), ("4", "3"), ("4", "3-noflat"), ("2", "1"), ("4", "1"), ("2", "0")]


def render(c, flags, ranges=None, coop=False):
    """Case c's sample range (or `ranges`: (begin, count) pairs into one accumulator) -> sums, counters.  coop: the context must be
    one whose renders take the cooperative walk — rsrt_render falls back to another walk without a word when the tree does not qualify,
    rsrt_cast_rays refuses traversal 6 under exactly the same condition, so one probe ray through it tells."""
    st = R.State.new(c.scene, c.env, c.w, c.h, camera=c.camera)
    try:
        st.max_bounces, st.flags = c.max_bounces, flags
        for begin, count in ranges or [(c.sample_begin, c.sample_count)]:
            st.render_range(begin, count)
        img, stats = st.download(), st.stats()
        if coop:
            st.cast_rays(np.zeros((1, 3), np.float32), np.float32([[0, 0, -1]]), 6 << 1, 0)
            assert stats["traversal_steps"] > 0, c.name  # a walk, not the flat loop
        return img, stats
    finally:
        st.close()


def check(c, what=(), coop=False):
    """-> the counters of the two runs (flags 0, FLAG_REFERENCE_TRAVERSAL)."""
    ref, ost = E.reference(c.name)
    out = []
    for flags in FLAGS:
        img, st = render(c, flags, coop=coop)
        nan = np.isnan(ref)
        diff = int(((util.bits(img) != util.bits(ref)) & ~nan).sum()) + int((np.isnan(img) != nan).sum())
        assert util.same_bits_or_nan(img, ref), (c.name, flags, what, diff)
        assert (st["paths"], st["ext_rays"], st["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"]), (c.name, flags, what)
        out.append(st)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_case_under_the_default_kernel_selection(name):
    check(E.case(name))


@pytest.mark.parametrize("name", NAMES)
def test_case_under_the_cooperative_walk(name, monkeypatch):
    monkeypatch.setenv("RSRT_TRAVERSAL", "6")
    monkeypatch.setenv("RSRT_FLAT", "0")
    check(E.case(name), "coop", coop=True)


@pytest.mark.parametrize("variant,traversal", FORMS)
def test_subset_through_the_other_kernel_forms(variant, traversal, monkeypatch):
    monkeypatch.setenv("RSRT_KERNEL", variant)
    monkeypatch.setenv("RSRT_TRAVERSAL", traversal[0])
    if traversal.endswith("noflat"):
        monkeypatch.setenv("RSRT_FLAT", "0")
    for name in SUBSET:
        check(E.case(name), (variant, traversal))


def test_bounce_limit_switches_from_the_flat_kernel_to_a_walk():
    """max_bounces fills the packed path state's 16-bit bounce field at 0xffff, where the flat loop still runs (it counts no traversal
    steps); one more and rsrt_render takes a walk (which does).  Both give the checker's image — the same image, paths end by escape."""
    steps = {mb: [st["traversal_steps"] for st in check(E.case("bounces_0x%x" % mb))] for mb in E.BOUNCES}
    for k in range(len(FLAGS)):
        assert steps[1][k] == steps[2][k] == steps[0xffff][k] == 0, steps
        assert steps[0x10000][k] > 0 and steps[0xffffffff][k] > 0, steps


def test_last_sample_indices_compose_and_the_overflow_is_rejected():
    c = E.case("samples_high")
    ref, ost = E.reference(c.name)
    for flags in FLAGS:
        img, st = render(c, flags, [(E.HIGH_BEGIN, 6), (E.HIGH_BEGIN + 6, E.HIGH_COUNT - 6)])
        assert util.same_bits_or_nan(img, ref), flags
        assert (st["ext_rays"], st["shadow_rays"]) == (ost["ext_rays"], ost["shadow_rays"])
    st = R.State.new(c.scene, c.env, c.w, c.h, camera=c.camera)
    try:
        st.max_bounces = c.max_bounces
        for begin, count in ((E.HIGH_BEGIN, 16), (0xffffffff, 1), (1, 0xffffffff)):
            with pytest.raises(R.RsrtError, match="sample range overflows u32"):
                st.render_range(begin, count)
            with pytest.raises(R.RsrtError, match="sample range overflows u32"):
                st.render_aov(begin, count)
        assert st.stats()["paths"] == 0  # nothing was launched
        st.render_range(0xfffffffe, 1)  # the last index on its own
        one = oracle.render(util.oracle_scene(c.scene), util.oracle_env(c.env), c.camera.view(oracle.CAMERA), c.w, c.h, 0xfffffffe, 1, c.max_bounces)[0]
        assert util.same_bits_or_nan(st.download(), one)
    finally:
        st.close()


PROBE_REFUSED = {"scale_suzanne_2^64_sky": {16, 17, 18, 19, 20, 21}}  # traversals 0, 1, 2 with the scene read from LDS


@pytest.mark.parametrize("name", [c.name for c in E.family("scale")])
def test_probe_on_scaled_scenes(name):
    """Camera-like rays (and the exact centre ray) through EVERY probe mode: the scaled trees keep short leaves and nested, finite
    boxes, so the flat loop (default), both wide walks and the LDS forms take them all.  The one exception is pinned in PROBE_REFUSED:
    suzanne at 2^64, whose boxes have infinite areas, is staged in LDS for the wide walks only, and the LDS form of the three tree
    walks is refused with the probe's documented message.  Any other refusal, or a pinned one that does not happen, fails the test."""
    c = E.case(name)
    o, d = E.probe_rays(c)
    osc = util.oracle_scene(c.scene)
    want = {b: oracle.cast_rays(osc, o, d, b, 0).view(np.uint32).reshape(-1, 9) for b in (0, 1)}
    modes = util.probe_modes(name, flat="default" in name)
    assert len(modes) == (28 if "default" in name else 24)
    st = R.State.new(c.scene, c.env, 16, 16, camera=c.camera)
    try:
        for mode in modes:
            if mode in PROBE_REFUSED.get(name, ()):
                with pytest.raises(R.RsrtError, match="this scene is not staged in LDS by the production kernel"):
                    st.cast_rays(o, d, mode, 0)
                continue
            got = np.ascontiguousarray(st.cast_rays(o, d, mode, 0))
            a, b = got.view(np.uint32).reshape(-1, 9), want[mode & 1]
            fa, fb = got.view(np.float32).reshape(-1, 9), want[mode & 1].view(np.float32)
            hit = b[:, 0] != 0
            assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[hit, 8], b[hit, 8]), (name, mode)
            assert util.same_bits_or_nan(fa[hit, 1:8], fb[hit, 1:8]), (name, mode)
            assert np.array_equal(a[~hit], b[~hit]), (name, mode)
    finally:
        st.close()


AOV_CASES = [c.name for c in E.family("cold", "scale", "normals", "camera")] + ["samples_high"]


@pytest.mark.parametrize("name", AOV_CASES)
def test_aov_pass_on_edge_cases(name):
    c = E.case(name)
    st = R.State.new(c.scene, c.env, c.w, c.h, camera=c.camera)
    try:
        st.render_aov(c.sample_begin, c.sample_count)
        got = st.download_aov()
    finally:
        st.close()
    want = D.aov_records(c.scene, util.oracle_scene(c.scene), c.camera[0], c.w, c.h, c.sample_begin, c.sample_count)
    assert util.same_bits_or_nan(got, want), name
    assert 4 * int(np.isnan(want).any(axis=-1).sum()) <= c.w * c.h


def test_device_builder_on_scaled_scenes():
    """Node for node the host builder's tree (values: a zero bound's sign may differ, test_bvh_device.py), or the documented refusal of
    an empty split side — whichever tests/bvh_ref.py says: the refusal exactly where the restatement meets an empty side (only a
    centroid span that overflows does that; overflowing and vanishing surface areas make NaN costs, which never win, and no empty
    side), the tree everywhere else.  The ordinary scales are built."""
    st = R.State.new(E.plain("default"), util.small_env(), 16, 16)
    outcome = {}
    try:
        for name in ("default", "suzanne", "house"):
            for k in E.SCALES:
                sc = E.scaled_scene(name, k)
                a = (sc.spheres, sc.plane_descs, sc.vertices, sc.triangles)
                if bvh_ref.build(*a)[3]:
                    with pytest.raises(R.RsrtError, match="a split left one side empty"):
                        st.build_bvh_device(*a)
                    outcome[name, k] = "refused"
                    continue
                p, n, d, _ = st.build_bvh_device(*a)
                assert util.fields_equal(p, sc.primitives) and util.fields_equal(n, sc.bvh_nodes) and d == sc.bvh_depth, (name, k)
                outcome[name, k] = "built"
    finally:
        st.close()
        print(outcome)
    for name in ("default", "suzanne", "house"):  # the controls are ordinary scenes: they are built
        assert outcome[name, 20] == outcome[name, -20] == "built", outcome
