"""One rsrt_context across scene, size, accumulator, tile, environment and job-size changes (tests/lifecycle_cases.py), against the
checker: every image bit for bit (util.bits), every ray count equal to the checker's counters, rsrt_get_stats read after each step (it
reports a window since the previous call).  test_lifecycle.py shows without a GPU that the cases reach what they aim at.

The chains (parts A, B, C) keep ONE context per chain in a module-scoped fixture and walk it through their steps as the cases of a
parametrised test, in order.  A case run on its own is a chain of one step, and any subset is a shorter chain: a step takes nothing
from the one before it but the context (a size step whose context already has its size clears first).  After a failed step the
later ones still run on that context, and may fail for what it left behind."""
import torch  # (before librsrt is loaded: the library then shares torch's HIP runtime, and a tensor's memory is the library's own kind)

import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref
import lifecycle_cases as L
import temporal_ref
import test_display
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import partition

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(util.bits(a), util.bits(b))


def render(st, begin, count, clear=True):
    """-> sums, the counters of this render alone."""
    if clear:
        st.clear()
    st.stats()  # (closes the window of whatever ran before)
    st.render_range(begin, count)
    return st.download(), st.stats()


def refused(call, status, match):
    with pytest.raises(R.RsrtError, match=match) as e:
        call()
    assert e.value.status == status, e.value


# ---------------------------------------------------------------------------------------------------- A: a chain of scenes
@pytest.fixture(scope="module", params=["default", "small"])
def chain(request, tmp_path_factory):
    """The chain's context under the default kernel selection, and under RSRT_KERNEL=2: every job runs the small form of the kernels
    (other workgroup sizes and pools, so other occupancies in the same cache rows).  The knob is read once, when the context is made."""
    L.scene("big", tmp_path_factory.mktemp("big"))
    before = os.environ.get("RSRT_KERNEL")
    if request.param == "small":
        os.environ["RSRT_KERNEL"] = "2"
    try:
        st = R.State(0)
    finally:
        if before is None:
            os.environ.pop("RSRT_KERNEL", None)
        else:
            os.environ["RSRT_KERNEL"] = before
    for slot, name in enumerate(L.CHAIN_ENVS):
        st.upload_environment(slot, L.env(name))
    st.resize(L.W, L.H)
    yield st
    st.close()


def check_step(st, step, uploaded=True):
    sc = L.scene(step.scene)
    if uploaded:
        st.upload_scene(sc)
    st.camera, st.max_bounces, st.environment_index = L.camera(sc), step.max_bounces, step.env_index
    ref, ost = L.step_reference(step)
    img, stats = render(st, 0, L.SPP)
    assert same(img, ref), (step.scene, int((util.bits(img) != util.bits(ref)).sum()))
    assert L.counters(stats) == L.counters(ost), step.scene
    # the class the scene was chosen for
    one = (np.zeros((1, 3), np.float32), np.float32([[0, 0, -1]]))
    if step.klass == "flat":
        assert stats["traversal_steps"] == 0, step.scene
    else:
        assert stats["traversal_steps"] > 0, step.scene
        if step.klass == "coop":
            st.cast_rays(one[0], one[1], 6 << 1, 0)
        else:
            refused(lambda: st.cast_rays(one[0], one[1], 6 << 1, 0), L.INVALID, L.COOP_REFUSED)
    # the probe, every way the scene qualifies for
    o, d, want = L.probe(step.scene)
    for mode in L.probe_modes(step):
        got = np.ascontiguousarray(st.cast_rays(o, d, mode, 0)).view(np.uint32).reshape(-1, 9)
        assert np.array_equal(got, want[mode & 1]), (step.scene, mode)
    if step.scene == "big":
        for mode in L.BIG_LDS_REFUSED:
            refused(lambda: st.cast_rays(o, d, mode, 0), L.INVALID, L.NOT_STAGED)
    assert st.walk_counters()["overflows"] == 0, step.scene  # (cumulative since the context was made: no batch abandoned along the chain)


CHAIN_IDS = []
for _i, _s in enumerate(L.CHAIN):
    CHAIN_IDS.append("%d_%s" % (_i, _s.scene))
    if _i == L.REFUSED_AFTER:
        CHAIN_IDS.append("%d_refused" % _i)


@pytest.mark.parametrize("what", CHAIN_IDS)
def test_scene_chain(chain, what):
    """Step `what` of lifecycle_cases.CHAIN on the chain's context: upload, then the render (image, counters), the kernel class and
    the probe.  "refused" (behind suzanne): an upload with a vertex index out of range raises and leaves suzanne in place, image
    and counters (include/rsrt.h: the arguments are checked before the scene is touched; only the temporal history is dropped); an upload of a valid
    tree deeper than the traversal stack raises after the old scene is gone, and the context has no scene until the next step."""
    st = chain
    i = int(what.split("_")[0])
    step = L.CHAIN[i]
    if not what.endswith("refused"):
        check_step(st, step)
        return
    sc = L.scene(step.scene)
    st.camera, st.max_bounces, st.environment_index = L.camera(sc), step.max_bounces, step.env_index
    st.upload_scene(sc)
    st.render_temporal(1)
    history = st.download_temporal()
    assert history[..., 3].any()
    refused(lambda: st.upload_scene(L.out_of_range_copy(sc)), L.INVALID, "vertex index out of range")
    refused(st.download_temporal, L.NOT_READY, "no temporal frame since the last reset")  # (the one thing a refused upload does drop)
    check_step(st, step, uploaded=False)
    refused(lambda: st.upload_scene(util.deck_scene(L.TOO_DEEP_LEVELS)), L.INVALID, "exceeds the supported traversal stack")
    before = st.download()
    o, d, _ = L.probe(step.scene)
    refused(lambda: st.render_range(0, 1), L.NOT_READY, "no scene uploaded")
    refused(lambda: st.cast_rays(o, d, 0, 0), L.NOT_READY, "no scene uploaded")
    refused(lambda: st.render_aov(0, 1), L.NOT_READY, "no scene uploaded")
    assert same(st.download(), before)


# ---------------------------------------------------------------------------------------------------- B: a chain of sizes
@pytest.fixture(scope="module", params=L.SIZE_ENVS)
def sized(request):
    sc = L.scene("default")
    st = R.State.new(sc, L.env(request.param), *L.SIZES[0])
    st.max_bounces = L.MB
    st.env_name = request.param
    yield st
    st.close()


@pytest.mark.parametrize("k", range(len(L.SIZES)), ids=["%d_%dx%d" % (k, w, h) for k, (w, h) in enumerate(L.SIZES)])
def test_size_chain(sized, k):
    """Size k of lifecycle_cases.SIZES on the chain's context.  No clear before a new size: its buffer must come zeroed, and a
    resize to the size the context has must keep the samples.  The four host-bound passes share one grow-only scratch buffer with four
    layouts (half4; half4 + a count word; two bytes4); their order rotates from size to size.  Then the AOV pass, the filter and a
    first temporal frame, whose buffers must follow the size."""
    st, en = sized, sized.env_name
    w, h = L.SIZES[k]
    ref2, ost2 = L.reference("default", en, w, h, 0, 2)
    ref4, ost4 = L.reference("default", en, w, h, 0, 4)
    had_size = (st.width, st.height) == (w, h)
    st.resize(w, h)
    if had_size:  # (the chain's first step, or a subset of it: a resize to the same size rightly keeps what the context holds)
        st.clear()
    img, stats = render(st, 0, 2, clear=False)
    assert same(img, ref2), (w, h, int((util.bits(img) != util.bits(ref2)).sum()))
    assert L.counters(stats) == L.counters(ost2)
    st.resize(w, h)
    img, stats = render(st, 2, 2, clear=False)
    assert same(img, ref4), (w, h)
    assert tuple(a + b for a, b in zip(L.counters(stats), L.counters(ost2))) == L.counters(ost4)

    def mean():
        m = st.download_mean_f16(4)
        want = (ref4[..., :3] / np.float32(4)).astype(np.float16)
        assert np.array_equal(m[..., :3].view(np.uint16), want.view(np.uint16)) and (m[..., 3] == 1.0).all(), (w, h)

    def display():
        assert np.array_equal(st.display_srgb8(4), test_display.display_numpy(ref4, 4)), (w, h)

    def view3():
        assert np.array_equal(st.debug_view(3).view(np.uint16), L.dev_view(en, 3, w, h, 0).view(np.uint16)), (w, h)

    def view2():
        assert np.array_equal(st.debug_view(2, sample_count=4).view(np.uint16), L.dev_view(en, 2, w, h, 4).view(np.uint16)), (w, h)

    passes = [mean, display, view3, view2]
    for f in passes[k % 4:] + passes[:k % 4]:
        f()
    assert same(st.download(), ref4)  # (the passes read the accumulator only)

    st.render_aov(0, 2)  # (no clear: the AOV buffer of a new size comes zeroed, the last size's temporal frame left a sample in the old one)
    aov = L.aov_reference("default", w, h, 0, 2)
    assert same(st.download_aov(), aov), (w, h)
    got = st.denoise(sample_total=4, aov_sample_total=2)
    assert same(got[..., :3], denoise_ref.denoise(ref4, aov, 4, 2)) and (got[..., 3] == 1.0).all(), (w, h)

    st.render_temporal(1)  # (clears the accumulator and the AOV buffer, renders sample 0 of a new history: the size is part of its key)
    sums, aov1, frame = st.download(), st.download_aov(), st.download_temporal()
    assert same(sums, L.reference("default", en, w, h, 0, 1)[0]) and same(aov1, L.aov_reference("default", w, h, 0, 1)), (w, h)
    want, _ = temporal_ref.Sequence().frame(sums, aov1, 1, 1, temporal_ref.Camera.from_record(st.camera))
    assert same(frame, want), (w, h)


def test_accumulator_ownership_chain():
    """owned -> bound to a zeroed torch tensor of another size -> unbound (the next render allocates) -> bound to a tensor of the
    first size.  Each state renders the checker's image; a bound tensor read through torch holds what download() returns."""
    sc = L.scene("default")
    (w0, h0), (w1, h1) = (64, 40), (48, 32)
    st = R.State.new(sc, L.env("small"), w0, h0)
    st.max_bounces = L.MB
    tensors = []
    try:
        def check(w, h, tensor):
            ref, ost = L.reference("default", "small", w, h, 0, 2)
            st.stats()
            st.render_range(0, 2)
            img, stats = st.download(), st.stats()
            assert same(img, ref) and L.counters(stats) == L.counters(ost), (w, h)
            if tensor is not None:
                assert same(tensor.cpu().numpy(), img), (w, h)

        check(w0, h0, None)
        for w, h in ((w1, h1), (0, 0), (w0, h0)):
            if w == 0:  # unbound: the context owns nothing now, the render allocates
                st.bind_accumulator(None, w0, h0)
                check(w0, h0, None)
                continue
            t = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            tensors.append(t)
            st.bind_accumulator(t.data_ptr(), w, h)
            check(w, h, t)
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- C: tile shapes
@pytest.fixture(scope="module", params=L.TILE_SCENES)
def tiled(request):
    sc = L.scene(request.param)
    st = R.State.new(sc, L.env("small"), *L.FRAMES[0])
    st.max_bounces = L.MB
    st.scene_name = request.param
    yield st
    st.close()


@pytest.mark.parametrize("frame", L.FRAMES, ids=["%dx%d" % f for f in L.FRAMES])
def test_tile_shapes(tiled, frame):
    """Every tile shape x world x rank of lifecycle_cases on one context per scene, set_partition and clear between the renders,
    against partition.tile_owner_map — the numpy formula, not the library's mask: owned pixels are the checker's, every other pixel is
    exactly zero, paths = owned pixels x samples, and the ranks of a world add up to the whole image and the checker's ray counts."""
    st, name = tiled, tiled.scene_name
    w, h = frame
    st.resize(w, h)
    try:
        for begin, count in L.RANGES:
            ref, ost = L.reference(name, "small", w, h, begin, count)
            for tw, th in L.tiles_of(frame):
                for world, skew in L.WORLDS.items():
                    assert partition.skew(world) == skew
                    owner = partition.tile_owner_map(w, h, world, tw, th)
                    total, rays = np.zeros_like(ref), 0
                    for rank in range(world):
                        what = (name, frame, begin, count, tw, th, world, rank)
                        st.set_partition(rank, world, tw, th)
                        img, stats = render(st, begin, count)
                        m = owner == rank
                        assert same(img[m], ref[m]), what
                        assert not util.bits(img[~m]).any(), what
                        assert stats["paths"] == int(m.sum()) * count, what
                        total += img
                        rays += stats["ext_rays"] + stats["shadow_rays"]
                    assert same(total, ref), what[:-1]
                    assert rays == ost["ext_rays"] + ost["shadow_rays"], what[:-1]
    finally:
        st.set_partition(0, 1)


def test_rejected_partition_leaves_the_previous_one():
    w, h = L.FRAMES[0]
    st = R.State.new(L.scene("default"), L.env("small"), w, h)
    st.max_bounces = L.MB
    try:
        st.set_partition(1, 2, 32, 2)
        for tw, th in L.REJECTED_TILES:
            refused(lambda: st.set_partition(0, 1, tw, th), L.INVALID, "pixel count must be a multiple of 64 and at most 4096")
        refused(lambda: st.set_partition(2, 2, 16, 16), L.INVALID, "rank 2 not in")
        img, stats = render(st, 0, 2)
        ref, _ = L.reference("default", "small", w, h, 0, 2)
        m = partition.tile_owner_map(w, h, 2, 32, 2) == 1
        assert same(img[m], ref[m]) and not util.bits(img[~m]).any() and stats["paths"] == int(m.sum()) * 2
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- D: environment slots
def upload_texels(st, slot, e, alias):
    """rsrt_upload_environment itself: alias None has the library build the table on the device."""
    rgba = np.ascontiguousarray(e.rgba, np.float32)
    a = None if alias is None else np.ascontiguousarray(alias)
    rc = st._L.rsrt_upload_environment(st._ctx, slot, e.width, e.height, rgba.ctypes.data_as(C.c_void_p), None if a is None else a.ctypes.data_as(C.c_void_p))
    st._check(rc, "rsrt_upload_environment")


def test_environment_slots_of_a_live_context():
    sc = L.scene("default")
    st = R.State.new(sc, L.env("small"), L.W, L.H)
    st.max_bounces = L.MB
    try:
        def shows(index, name):
            st.environment_index = index
            ref, ost = L.reference("default", name, L.W, L.H, 0, 3)
            img, stats = render(st, 0, 3)
            assert same(img, ref) and L.counters(stats) == L.counters(ost), (index, name)

        # slot 0 replaced in place: 64x32 with a host table, 100x37 with a table built on the device, 8x4 with a host table
        shows(0, "small")
        upload_texels(st, 0, L.env("odd"), None)
        shows(0, "odd")
        st.upload_environment(0, L.env("tiny"))
        shows(0, "tiny")
        # sparse slots
        st.upload_environment(5, L.env("odd"))
        shows(5, "odd")
        before = st.download()
        st.environment_index = 3
        refused(lambda: st.render_range(3, 1), L.NOT_READY, "environment 3 not uploaded")
        assert same(st.download(), before)
        # slot 64 is refused, a refused re-upload leaves the slot as it was
        refused(lambda: st.upload_environment(64, L.env("small")), L.INVALID, "slot 64 > 63")
        st.environment_index = 5
        st.render_temporal(1)
        assert st.download_temporal()[..., 3].any()
        bad = L.env("small").alias.copy()
        bad["alias_index"][7] = len(bad)
        refused(lambda: upload_texels(st, 5, L.env("small"), bad), L.INVALID, "alias_index")
        refused(lambda: upload_texels(st, 0, L.env("small"), bad), L.INVALID, "alias_index")
        refused(st.download_temporal, L.NOT_READY, "no temporal frame since the last reset")  # (the one thing a refused upload does drop)
        shows(5, "odd")
        shows(0, "tiny")
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------- E: two contexts; mixed jobs
def test_two_contexts_interleaved():
    a = R.State.new(L.scene("default"), L.env("small"), 64, 40)
    b = R.State.new(L.scene("suzanne"), L.env("small"), 48, 32)
    try:
        a.max_bounces = b.max_bounces = L.MB
        for k in range(6):
            a.render_range(k, 1)
            b.render_range(k, 1)
        for st, name, (w, h) in ((a, "default", (64, 40)), (b, "suzanne", (48, 32))):
            ref, ost = L.reference(name, "small", w, h, 0, 6)
            assert same(st.download(), ref), name
            assert L.counters(st.stats()) == L.counters(ost), name  # (its own rays only)
        a.close()
        b.render_range(6, 1)
        ref, ost = L.reference("suzanne", "small", 48, 32, 0, 7)
        assert same(b.download(), ref)
        assert L.counters(b.stats()) == tuple(x - y for x, y in zip(L.counters(ost), L.counters(L.reference("suzanne", "small", 48, 32, 0, 6)[1])))
    finally:
        a.close()
        b.close()


def test_ordinary_and_small_jobs_alternate_in_one_context():
    """default at 1024 x 512: nine samples a call are 4.7 M paths, an ordinary job on lane 0; one sample a call is a small job, which
    is pipelined over the other lanes IF an earlier kernel is still running when it arrives.  Whether that happens depends on timing
    and cannot be forced from here: the six small calls are issued straight behind the ordinary one, which makes it likely, and the
    result — the checker's [0, 24) and its counters — is asserted whichever way they ran."""
    w, h = 1024, 512
    st = R.State.new(L.scene("default"), L.env("small"), w, h)
    try:
        st.max_bounces = L.MB
        st.render_range(0, 9)
        for k in range(6):
            st.render_range(9 + k, 1)
        st.render_range(15, 9)
        img, stats = st.download(), st.stats()
    finally:
        st.close()
    ref, ost = L.reference("default", "small", w, h, 0, 24, L.MB, True)
    assert same(img, ref)
    assert L.counters(stats) == L.counters(ost)
