"""The fog march on the GPU at the edges of tests/edge_fog.py: rt_fog_kernel's records against the numpy restatement (tests/fog_ref.py on
the checker's hits and shadow queries) bit for bit, one case a render of at most 1,536 pixels x 2 samples x 64 steps — scenes scaled
until squared lengths leave the format, cameras inside and on surfaces, degenerate and hand-edited trees in both forms of the kernel
(the scene in LDS, or in global memory), axis-parallel lights, march points 3e38 units away, transmittance exactly 0 part-way; split
sample ranges; nothing else written; a clear medium; the refused parameter sets.  test_fog_edges.py shows, without a GPU, that the
cases reach these edges.

Why the shadow walk ends whatever its slab tests return (a march point may be +-inf or NaN): trace_threaded's cursor moves only to the
node's near child or along its escape link, both fixed at upload for the ray's sign octant from a tree validate_tree has shown to be
one (every node reached exactly once); in that octant's visiting order either move goes strictly forward, so a walk takes at most
n_nodes box steps, and its leaf loop at most the leaves' record counts, which the upload bounds by the primitive array."""
import ctypes as C

import numpy as np
import pytest

import edge_fog as EF
import fog_ref
import util
import rsoderh_raytracing_amd as R
from test_denoise_gpu import DeviceArray
from test_bloom_gpu import raises
from test_fog_edges import REFUSED

pytestmark = pytest.mark.gpu

INVALID = 1
F = np.float32


def equal(a, b):
    return a.shape == b.shape and np.array_equal(util.bits(a), util.bits(b))


def new_state(c):
    return R.State.new(c.scene, util.small_env(), c.w, c.h, camera=c.camera)


def compare(name):
    """One case: the records of [3, 5) in one call and in two, against the restatement; finite; the transmittance sums within [0, n];
    the accumulator, the AOV buffer and the guide as they were."""
    c = EF.case(name)
    want, lit = EF.reference(name)
    st = new_state(c)
    try:
        st.render_samples(1, aov=True)
        st.render_guide(c.w, c.h, 0, 1)
        before = [st.download(), st.download_aov(), st.download_guide()]
        st.render_fog(c.sample_count, c.sample_begin, **c.params)
        got = st.download_fog()
        print("%s: %s form, lit %.3f, mixed %.3f, %d of %d record floats differ" % ((name, EF.kernel_form(name)) + EF.shares(lit) +
                                                                                   (int((util.bits(got) != util.bits(want)).sum()), got.size)))
        assert equal(got, want)
        assert np.isfinite(got).all() and (got[..., 3] >= 0).all() and (got[..., 3] <= c.sample_count).all()
        assert st.fog_sample_count == c.sample_count and (st.fog_width, st.fog_height) == (c.w, c.h)
        st.clear_fog()
        st.render_fog(1, c.sample_begin, **c.params)  # [3, 4) then [4, 5) gives the bits of [3, 5)
        st.render_fog(1, c.sample_begin + 1)
        assert equal(st.download_fog(), want)
        for a, b in zip(before, [st.download(), st.download_aov(), st.download_guide()]):
            assert a.tobytes() == b.tobytes()
    finally:
        st.close()


@pytest.mark.parametrize("name", EF.names("scene"))
def test_scene_family_records_equal_the_restatement_bit_for_bit(name):
    compare(name)


@pytest.mark.parametrize("name", EF.names("tree"))
def test_tree_family_records_equal_the_restatement_bit_for_bit(name):
    compare(name)


@pytest.mark.parametrize("name", EF.names("param"))
def test_param_family_records_equal_the_restatement_bit_for_bit(name):
    compare(name)


def test_the_tree_family_runs_both_forms_of_the_kernel():
    forms = {n: EF.kernel_form(n) for n in EF.names("tree")}
    print(forms)
    assert set(forms.values()) == {"lds", "global"}


@pytest.mark.parametrize("scene", list(EF.PARAM_SCENES))
@pytest.mark.parametrize("edge", EF.CLEAR)
def test_a_clear_medium_leaves_the_source_as_it_is(scene, edge):
    """density 0: every record is (0, 0, 0, n), and the fog image of a bound accumulator is its mean bit for bit, a -0.0 included."""
    for jitter in (0, 1):
        c = EF.param_case(scene, edge, jitter)
        st = new_state(c)
        try:
            st.render_fog(c.sample_count, c.sample_begin, **c.params)
            rec = st.download_fog()
            assert equal(rec, np.broadcast_to(F([0, 0, 0, c.sample_count]), rec.shape))
            rng = np.random.default_rng(c.w + jitter)
            sums = (rng.random((c.h, c.w, 4)) * 8).astype(F)
            sums[0, 0, :3], sums[-1, -1, :3], sums[..., 3] = (-0.0, 0.0, 1.0), (3.0, -0.0, -0.0), 3.0
            mine = DeviceArray(sums)
            st.bind_accumulator(mine.data_ptr(), c.w, c.h)
            st.fog("mean", sample_total=3)
            got = st.fog_download()
            assert equal(got[..., :3], fog_ref.source_colour(sums, 3)) and (got[..., 3] == 1).all()
            assert util.bits(got[0, 0, 0]) == 0x80000000 and util.bits(got[-1, -1, 1]) == 0x80000000
        finally:
            st.close()


def test_refused_parameter_sets_leave_records_image_and_parameters_as_they_were():
    c = EF.param_case("default", "g_+0.95", 1)
    st = new_state(c)
    try:
        st.render_samples(2, aov=True)
        st.render_fog(c.sample_count, c.sample_begin, **c.params)
        st.fog("mean")
        rec, img, remembered = st.download_fog(), st.fog_download(), bytes(st.fog_params)
        for kw in REFUSED:
            bad = dict(c.params, **{k: fog_ref.params(**kw)[k] for k in kw})  # the case's set with the refused fields over it
            assert not fog_ref.params_ok(bad), kw
            raises(INVALID, lambda: st.render_fog(1, c.sample_begin + c.sample_count, **bad))
            cp = R.state.FogParams.of(**bad)
            raises(INVALID, lambda: st._check(st._L.rsrt_fog_apply_upsampled(st._ctx, 0, 2, c.sample_count, 2, C.byref(cp), None, None), "rsrt_fog_apply_upsampled"))
            assert st.fog_sample_count == c.sample_count and bytes(st.fog_params) == remembered
            assert equal(st.download_fog(), rec) and equal(st.fog_download(), img)
        st.render_fog(1)  # the remembered parameters still serve
        assert st.fog_sample_count == c.sample_count + 1
    finally:
        st.close()
