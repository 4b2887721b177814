"""The device BVH builder (rsrt_build_bvh_device, csrc/hip/rt_bvh_device.h) on the catalogue of tests/edge_trees.py, and the trees
these inputs give through kernel selection and traversal.  What a case must do is decided by tests/bvh_ref.py, never by the code
under test: where the restatement meets no empty split side the device must return the host builder's tree node for node (values:
a zero bound's sign is the documented exception, test_bvh_device.py), where it does the device must refuse with its documented
message — and go on building on the same context."""
import time

import numpy as np
import pytest

import bvh_ref
import edge_trees as ET
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host
from test_edge_trees import BOUNCES, H, REFUSALS, SPP, W, image_info, probe_refusal, reference  # (the checker's answers: computed once, shared)

pytestmark = pytest.mark.gpu


def test_device_builder_on_the_catalogue():
    st = R.State.new(R.Scene.load_toml(util.scene_path("default")), util.small_env(), 16, 16)
    report, after_refusal, refused = [], False, 0
    try:
        for c in ET.cases():
            a = (c.spheres, c.plane_descs, c.vertices, c.triangles)
            fallback = bvh_ref.build(*a)[3]
            if fallback:
                with pytest.raises(R.RsrtError, match="a split left one side empty"):
                    st.build_bvh_device(*a)
                report.append("%-24s refused" % c.name)
                after_refusal, refused = True, refused + 1
                continue
            ref = host.build_bvh(*a)  # (test_edge_trees.py holds it to bvh_ref on this very case)
            t = time.perf_counter()
            p, n, d, ms = st.build_bvh_device(*a)
            wall = (time.perf_counter() - t) * 1e3
            report.append("%-24s %5d nodes, depth %2d, longest leaf %3d, device %.2f ms (call %.1f ms)%s"
                          % (c.name, len(n), d, ET.longest_leaf(n), ms, wall, "  [after a refusal]" if after_refusal else ""))
            assert util.fields_equal(p, ref[0]), c.name
            assert util.fields_equal(n, ref[1]), c.name
            assert d == ref[2], c.name
            after_refusal = False
    finally:
        st.close()
        print("\n".join(report))
    assert refused == 2 and not after_refusal  # both refusals happened, and a case was built after the last one


# ---------------------------------------------------------------------------------------------------- the trees, traversed
def words(records):
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 9)


@pytest.mark.parametrize("name", ET.TRAVERSED)
def test_probe_on_the_builder_s_trees(name):
    """1,024 rays (ET.probe_rays) through all 28 probe modes.  Which modes run and which are refused, and with which documented
    message, is what include/rsrt.h's rule gives for the scene's image info (test_edge_trees.probe_refusal; the info itself is pinned
    there): a mode that runs must give the checker's records bit for bit, a mode that must be refused must be refused with exactly
    that message, and a refusal the rule does not give fails the test."""
    info = image_info(name)
    o, d = ET.probe_rays(name)
    want = [words(h) for h in reference(name)[3]]
    every = util.probe_modes(name, flat=True)
    qualifies = set(util.probe_modes(name, flat=bool(info.flat_ok), wide=bool(info.wide_ok)))
    assert len(every) == 28
    ran, refused = [], {}
    st = R.State.new(ET.scene(name), util.small_env(), 16, 16)
    try:
        for mode in every:
            why = probe_refusal(info, mode)
            assert why is not None or mode in qualifies, mode
            if why is not None:
                with pytest.raises(R.RsrtError, match=REFUSALS[why]):
                    st.cast_rays(o, d, mode, 0)
                refused[mode] = why
                continue
            got = words(st.cast_rays(o, d, mode, 0))
            bad = np.nonzero((got != want[mode & 1]).any(axis=1))[0]
            assert len(bad) == 0, "%s mode %d (traversal %d%s%s): %d of %d rays differ, first ray %d o=%r d=%r\n  probe   %r\n  checker %r" % (
                name, mode, mode >> 1 & 7, ", LDS" if mode & 16 else "", ", cast_ray_bvh" if mode & 1 else "", len(bad), len(o), bad[0],
                o[bad[0]].tolist(), d[bad[0]].tolist(), got[bad[0]], want[mode & 1][bad[0]])
            ran.append(mode)
    finally:
        st.close()
    print("%s: ran modes %s; refused %s" % (name, ran, refused))
    assert {m for m in every if m not in qualifies} <= set(refused)


def production_traversal(info):
    """What rsrt_render took (select_traversal's rule, csrc/hip/rsrt_api.hip), for the report; the flat loop is checked from the counters."""
    if info.flat_ok:
        return "flat loop"
    if info.wide_ok and info.coop_ok:
        return "cooperative wide walk"
    if info.wide_ok:
        return "wide walk"
    return "fixed-order walk" if info.typed_leaves else "generic tree walk"


@pytest.mark.parametrize("kernel", ["default", "2"])
@pytest.mark.parametrize("name", ET.TRAVERSED)
def test_render_and_aov_of_the_builder_s_trees(name, kernel, monkeypatch):
    """48 x 32, 2 samples, 4 bounces and the AOV pass under the default kernel selection and under RSRT_KERNEL=2 (the small form):
    image sums and AOV records bit for bit the checker's, the ray counts equal, and the flat loop exactly where the image says so."""
    if kernel != "default":
        monkeypatch.setenv("RSRT_KERNEL", kernel)
    img, ost, aov, _ = reference(name)
    info = image_info(name)
    st = R.State.new(ET.scene(name), util.small_env(), W, H)
    try:
        st.max_bounces = BOUNCES
        st.render_range(0, SPP)
        got, stats = st.download(), st.stats()
        st.render_aov(0, SPP)
        got_aov = st.download_aov()
    finally:
        st.close()
    print("%s, RSRT_KERNEL %s: %s, %d traversal steps, %d paths, %d extension rays, %d shadow rays"
          % (name, kernel, production_traversal(info), stats["traversal_steps"], stats["paths"], stats["ext_rays"], stats["shadow_rays"]))
    diff = int((util.bits(got) != util.bits(img)).sum())
    assert diff == 0, (name, kernel, "image words that differ", diff)
    assert (stats["paths"], stats["ext_rays"], stats["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"]), (name, kernel)
    assert (stats["traversal_steps"] == 0) == bool(info.flat_ok), (name, kernel, stats["traversal_steps"])
    assert np.array_equal(util.bits(got_aov), util.bits(aov)), (name, kernel, "aov")
