"""The ray probe, the render kernels, the AOV pass and the device BVH builder on tests/feature_rays.py, against the checker
(test_feature_rays.py shows without a GPU that every ray class reaches its edge, and holds the checker itself to an exact second
reading there).  Every record is finite, so all nine words of every record are compared bit for bit (util.bits).  A mismatch names
the ray class, the probe mode and the first differing ray with both records."""
import numpy as np
import pytest

import denoise_ref as D
import feature_rays as FR
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host

pytestmark = pytest.mark.gpu

SCENES = ("small", "large")
N_MODES = {"small": 28, "large": 24}
# scene -> {probe mode: the library's documented message}: the modes rsrt_cast_rays refuses for that scene.  None: large is not staged
# whole in LDS, but each traversal's own LDS form (the tree walks' nodes + escape links, the fixed-order walk's top block, the wide
# walks' head of wide nodes) has room for it
PROBE_REFUSED = {}
W, H, SPP, BOUNCES = 48, 32, 2, 4


def words(records):
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 9)


def explain(name, got, want, mode, n):
    """The class, the mode and the first differing ray with both records (rows 0 .. n - 1 of the concatenated set)."""
    o, d, where = FR.all_rays(name)
    bad = np.nonzero((words(got) != words(want)[:n]).any(axis=1))[0]
    g = int(bad[0])
    cname = next(c for c, s in where.items() if s.start <= g < s.stop)
    return "scene %s class %s mode %d (traversal %d%s%s): %d of %d rays differ, first ray %d (%d of its class) o=%r d=%r\n  probe   %r\n  checker %r" % (
        name, cname, mode, mode >> 1 & 7, ", LDS" if mode & 16 else "", ", cast_ray_bvh" if mode & 1 else "", len(bad), n, g, g - where[cname].start,
        o[g].tolist(), d[g].tolist(), got[g], want[g])


def check_probe(st, name, mode, n=None):
    o, d, _ = FR.all_rays(name)
    n = len(o) if n is None else n
    got = st.cast_rays(o[:n], d[:n], mode, 0)
    want = FR.answers(name, mode & 1)
    assert np.isfinite(got.view(np.float32).reshape(-1, 9)[:, 1:8]).all()
    assert np.array_equal(words(got), words(want)[:n]), explain(name, got, want, mode, n)


def new_state(name, w=16, h=16):
    return R.State.new(FR.scene(name), util.small_env(), w, h)


def check_modes(name, modes):
    st = new_state(name)
    try:
        for mode in modes:
            if mode in PROBE_REFUSED.get(name, {}):
                with pytest.raises(R.RsrtError, match=PROBE_REFUSED[name][mode]):
                    check_probe(st, name, mode)
                continue
            check_probe(st, name, mode)
    finally:
        st.close()


@pytest.mark.parametrize("name", SCENES)
def test_every_class_through_every_probe_mode(name):
    """All twelve classes through the seven traversals (six for large, which the flat loop does not take), the scene read from global
    memory and from LDS, cast_ray and cast_ray_bvh: the equal side of every comparison of the three routines, the sphere's
    `discriminant == 0` branch, and at every shared edge and vertex a tie that each traversal settles by its own visiting order.
    No mode is skipped; a refusal that is not pinned in PROBE_REFUSED, or a pinned one that does not happen, fails."""
    modes = util.probe_modes(name, flat=(name == "small"))
    assert len(modes) == N_MODES[name] and set(PROBE_REFUSED.get(name, {})) <= set(modes)
    check_modes(name, modes)


@pytest.mark.parametrize("name,mode", [("small", 3 << 1), ("small", 6 << 1), ("large", 6 << 1)])
def test_ragged_batches(name, mode):
    """The probe runs fixed 64-ray batches by index: the first 1, 63, 64, 65 and 129 rays and the whole set, each against the same prefix
    of the checker's answer.  The cooperative walk's partial batch (lanes without a ray beside lanes with one) is the case of interest."""
    st = new_state(name)
    try:
        for n in (1, 63, 64, 65, 129, None):
            check_probe(st, name, mode, n)
    finally:
        st.close()


@pytest.mark.parametrize("knob,value", [("RSRT_FLAT_ORIENTED", "0"), ("RSRT_FLAT_QUORUM", "0"), ("RSRT_FLAT_QUORUM", "100")])
def test_small_under_the_flat_loop_s_knobs(knob, value, monkeypatch):
    """Without the per-octant leaf tables the flat loop orders each box's slab values itself; with the triangle loop's vote at 0 no ray is
    ever cut short, at 100 every ray is, and resumes with a best hit from an earlier trip — a tie against an incumbent.  The probe's
    modes and a render."""
    monkeypatch.setenv(knob, value)
    check_modes("small", util.probe_modes("small", flat=True))
    check_render("small", flat=True)


@pytest.mark.parametrize("knob,value", [("RSRT_COOP_NARROW_AT", "0"), ("RSRT_COOP_LDS_CAP", "64")])
def test_large_under_the_cooperative_walk_s_knobs(knob, value, monkeypatch):
    """One node item a trip, always the newest (a depth-first walk of the whole batch), and the node ring capped at one block (its items
    spill to the arena and come back): which items travel together, and in which order, must not show in which of two equal hits wins."""
    monkeypatch.setenv(knob, value)
    check_modes("large", [(6 << 1) | lds | bvh for lds in (0, 16) for bvh in (0, 1)])
    check_render("large", flat=False)


# ---------------------------------------------------------------------------------------------------- renders
def reference(name):
    """The checker's image sums, counters and AOV records of scene `name` under its own camera (computed once per scene)."""
    if name not in reference.cache:
        sc, env = FR.scene(name), util.small_env()
        cam = sc.camera_uniform()
        img, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(env), cam.view(oracle.CAMERA), W, H, 0, SPP, BOUNCES)
        aov = D.aov_records(sc, util.oracle_scene(sc), cam[0], W, H, 0, SPP)
        assert np.isfinite(img).all() and np.isfinite(aov).all()
        assert 4 * int((aov[..., 3] > 0).sum()) >= W * H  # the camera sees the scene
        reference.cache[name] = (img, ost, aov)
    return reference.cache[name]


reference.cache = {}


def check_render(name, flat, coop=False):
    """48 x 32, 2 spp, 4 bounces and the AOV pass under the context's kernel selection: sums bit for bit, the ray counts, and whether it was
    the flat loop (which counts no traversal steps) that ran.  coop: the context must be one that takes the cooperative walk."""
    ref, ost, aov = reference(name)
    for flags in (0, R.state.FLAG_REFERENCE_TRAVERSAL):
        st = new_state(name, W, H)
        try:
            st.max_bounces, st.flags = BOUNCES, flags
            st.render_range(0, SPP)
            img, stats = st.download(), st.stats()
            st.render_aov(0, SPP)
            got_aov = st.download_aov()
            if coop:
                st.cast_rays(np.zeros((1, 3), np.float32), np.float32([[0, 0, -1]]), 6 << 1, 0)  # (refused where renders do not take it)
        finally:
            st.close()
        diff = int((util.bits(img) != util.bits(ref)).sum())
        assert diff == 0, (name, flags, "image words that differ", diff)
        assert (stats["paths"], stats["ext_rays"], stats["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"]), (name, flags)
        assert (stats["traversal_steps"] == 0) == flat, (name, flags, stats["traversal_steps"])
        assert np.array_equal(util.bits(got_aov), util.bits(aov)), (name, flags, "aov")
        assert ost["shadow_rays"] > 0


@pytest.mark.parametrize("name", SCENES)
def test_render_and_aov_under_the_default_selection(name):
    """Production kernels take these scenes: small runs the flat loop, large a walk; the shadow query meets lattice geometry."""
    check_render(name, flat=(name == "small"))


def test_render_and_aov_of_large_forced_to_the_cooperative_walk(monkeypatch):
    monkeypatch.setenv("RSRT_TRAVERSAL", "6")
    monkeypatch.setenv("RSRT_FLAT", "0")
    check_render("large", flat=False, coop=True)


# ---------------------------------------------------------------------------------------------------- the device builder
def test_device_builder_on_symmetric_input():
    """A square grid of identical quads gives the binned-SAH builder exactly equal costs at several buckets and centroid boxes as long in x
    as in y (test_feature_rays.py shows where): `first minimum wins` and max_axis's tie rule are decided by exact ties, which random and
    clustered inputs never produce on purpose.  Node for node and record for record the host builder's tree."""
    st = new_state("small")
    try:
        for name in ("small", "large", "bare"):
            sc = FR.scene(name)
            want = host.build_bvh(sc.spheres, sc.plane_descs, sc.vertices, sc.triangles)
            assert util.fields_equal(want[0], sc.primitives) and util.fields_equal(want[1], sc.bvh_nodes) and want[2] == sc.bvh_depth
            p, n, depth, _ = st.build_bvh_device(sc.spheres, sc.plane_descs, sc.vertices, sc.triangles)
            assert util.fields_equal(p, want[0]), name
            assert util.fields_equal(n, want[1]), (name, [i for i in range(min(len(n), len(want[1]))) if n[i] != want[1][i]][:4])
            assert depth == want[2], name
    finally:
        st.close()
