"""The render kernels, the packing of an uploaded environment and the developer views on the environment edge cases of
tests/edge_envs.py, against the checker (test_env_edges.py shows without a GPU that the checker agrees with an independent float64
reading on every case, and that every reference is finite).  Image sums are compared bit for bit (util.bits: the references hold no
NaN), and paths, ext_rays and shadow_rays with the checker's counters.

Which kernel reads what: scene `default` takes the flat kernel, which reads both PACKED pmf copies (a texel's alpha = the pmf of its
entry, an entry's pad word = the pmf of its alias target: env_bilinear_pmf, sample_environment_finish<true>); `suzanne` takes the
cooperative walk, which reads the texels' copy for an escaping ray and gathers an alias target's pmf from the table; the one-ray-a-lane
walks (RSRT_TRAVERSAL=4, 3) read the tables only.  Frames are 48x32, 4 spp, 6 bounces."""
import ctypes as C

import numpy as np
import pytest

import edge_envs as V
import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import types as T

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def render(st, clear=True):
    """-> sums, the counters of this render alone (rsrt_get_stats reports a window since the previous call)."""
    if clear:
        st.clear()
    st.stats()
    st.render_range(0, V.SPP)
    return st.download(), st.stats()


def check(st, ref, what):
    """One render of the context as it stands against a reference of edge_envs (which is finite, or edge_envs raised)."""
    want, ost = ref
    assert np.isfinite(want).all(), what
    img, stats = render(st)
    assert same(img, want), (what, int((util.bits(img) != util.bits(want)).sum()))
    assert V.counters(stats) == V.counters(ost), what
    return stats


def context(scene_name, env=None, camera=None):
    sc = E.plain(scene_name)
    st = R.State.new(sc, env if env is not None else [], V.W, V.H, camera=camera)
    st.max_bounces = V.BOUNCES
    return st


# ---------------------------------------------------------------------------------------------------- a: render parity
@pytest.mark.parametrize("name", V.NAMES)
def test_case_renders_the_checkers_picture(name):
    for scene in V.SCENES:
        st = context(scene, V.case(name).env)
        try:
            stats = check(st, V.reference(name, scene), (name, scene))
            # default: the flat loop (it counts no traversal steps), with both packed reads; suzanne: a walk
            assert (stats["traversal_steps"] == 0) == (scene == "default"), (name, scene)
        finally:
            st.close()


# ---------------------------------------------------------------------------------------------------- b: the other kernel forms
FORMS = {"small": ({"RSRT_KERNEL": "2"}, V.SCENES), "noflat": ({"RSRT_FLAT": "0"}, ("default",)),
         "wide": ({"RSRT_TRAVERSAL": "4"}, ("suzanne",)), "fixed": ({"RSRT_TRAVERSAL": "3"}, ("suzanne",))}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["quad", "odd6", "spike", "chain", "never_self"])
def test_case_through_the_other_kernel_forms(name, form, monkeypatch):
    """small: 256-thread workgroups, both scenes; noflat: `default` through the cooperative walk instead of the flat loop; wide, fixed:
    `suzanne` through the one-ray-a-lane wide walk and the fixed-order walk.  (The knobs are read when the context is made.)"""
    knobs, scenes = FORMS[form]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for scene in scenes:
        st = context(scene, V.case(name).env)
        try:
            stats = check(st, V.reference(name, scene), (name, form, scene))
            if form == "noflat":
                assert stats["traversal_steps"] > 0
        finally:
            st.close()


# ---------------------------------------------------------------------------------------------------- c: open sky
@pytest.mark.parametrize("camera", sorted(V.SKY_CAMERAS))
@pytest.mark.parametrize("name", ["quad", "strip", "pillar", "odd_noise"])
def test_open_sky_through_the_poles_and_the_seam(name, camera):
    """Scene `cube` looking straight up, straight down and exactly along -x: camera rays and first bounces land on the poles (v just
    outside [0, 1]: RT_INV_PI is not 1 / pi) and on the u = 0 / u = 1 seam, where every fetch takes a clamp-to-edge tap."""
    st = context("cube", V.case(name).env, camera=V.SKY_CAMERAS[camera])
    try:
        check(st, V.reference(name, "cube", camera), (name, camera))
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- d: repacking
def upload(st, slot, env, with_table=True):
    L = R.state.lib()
    rgba = np.ascontiguousarray(env.rgba, np.float32)
    alias = np.ascontiguousarray(env.alias) if with_table else None
    rc = L.rsrt_upload_environment(st._ctx, slot, env.width, env.height, rgba.ctypes.data_as(C.c_void_p),
                                   alias.ctypes.data_as(C.c_void_p) if with_table else None)
    assert rc == 0, L.rsrt_last_error(st._ctx)


@pytest.mark.parametrize("scene", V.SCENES)
def test_packed_words_follow_every_change_of_a_slots_table(scene):
    """One context, slot 0: a caller's table; the library's own table built over it on the device (the packed words of the caller's
    table must go); another map of another size, uploaded without a table; a caller's table again.  Each render is the checker's
    picture under the table the slot holds at that moment."""
    L = R.state.lib()
    L.rsrt_environment_build_alias.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    chain = V.case("chain").env
    st = context(scene, chain)
    try:
        check(st, V.reference("chain", scene), "1 chain")
        n = chain.width * chain.height
        out, left = np.zeros(n, T.ALIAS_ENTRY), C.c_uint32(0xffffffff)
        assert L.rsrt_environment_build_alias(st._ctx, 0, out.ctypes.data_as(C.c_void_p), n, C.byref(left)) == 0, L.rsrt_last_error(st._ctx)
        host = V.rebuilt("chain")
        for f in ("probability", "alias_index", "pmf"):
            assert np.array_equal(out[f].view(np.uint32), host.alias[f].view(np.uint32)), f
        assert left.value == host.leftover
        assert not np.array_equal(host.alias["pmf"], chain.alias["pmf"])  # (the step changes what a stale copy would hold)
        check(st, V.reference("rebuilt:chain", scene), "2 rebuilt on the device")
        upload(st, 0, V.case("odd_noise").env, with_table=False)
        check(st, V.reference("odd_noise", scene), "3 odd_noise, no table given")
        upload(st, 0, V.case("uniform").env)
        check(st, V.reference("uniform", scene), "4 uniform")
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- e: slots
@pytest.mark.parametrize("scene", V.SCENES)
def test_every_slot_renders_its_own_environment(scene):
    st = context(scene)
    try:
        held = {0: "one", 5: "odd6", 63: "strip"}
        for slot, name in held.items():
            st.upload_environment(slot, V.case(name).env)
        for round_ in range(2):
            for slot, name in held.items():
                st.environment_index = slot
                check(st, V.reference(name, scene), (round_, slot, name))
            held[5] = "spike"
            st.upload_environment(5, V.case("spike").env)
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- f: developer views
@pytest.mark.parametrize("name", V.NAMES)
def test_developer_views_of_every_case(name):
    """View 3 shows the texels (alpha 0 everywhere: the pmf packed into a texel's alpha on the device does not leak), view 2 the
    alias table's draws, on a frame smaller than strip, pillar and odd_noise and larger than the other maps (16x8), and on 4x2."""
    env = V.case(name).env
    oenv = util.oracle_env(env)
    st = context("default", env)
    try:
        for w, h in ((16, 8), (4, 2)):
            st.resize(w, h)
            got3, want3 = st.debug_view(3), oracle.debug_view(3, oenv, w, h, 0)
            assert np.array_equal(got3.view(np.uint16), want3.view(np.uint16)), (name, w, h)
            assert (got3[..., 3].view(np.uint16) == 0).all(), (name, w, h)
            got2, want2 = st.debug_view(2, sample_count=0), oracle.debug_view(2, oenv, w, h, 0)
            assert np.array_equal(got2.view(np.uint16), want2.view(np.uint16)), (name, w, h)
            again = st.debug_view(2, out_texture=got2, sample_count=1)
            want_again = oracle.debug_view(2, oenv, w, h, 1, out_texture=want2)
            assert np.array_equal(again.view(np.uint16), want_again.view(np.uint16)), (name, w, h)
    finally:
        st.close()
