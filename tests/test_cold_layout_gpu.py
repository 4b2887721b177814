"""The flat kernel keeps a slot's cold path state in one 64-byte record (rt_cold_layout.h: T and last pdf, L and the output slot, the
pending NEE term, the triangles a cut-short ray has left, a 16-byte quad each) instead of one column per field.  Nothing a path computes
moves, so every frame here is the checker's bit for bit with the checker's path and ray counts.  A 64 x 48 frame at 4 spp hands six waves
a full 2,048-path chunk, so every slot of a 192-slot pool is recycled many times: a field that landed in a neighbour's record, or in
another field's dword, shows as a wrong pixel.  Cases: the triangle-loop vote cutting every ray it can (quad 3 is written and read back)
and never; a second call that starts on the records the first left; single-sample calls (the small form, 160-slot pools, an arena per
lane); a ragged frame; a camera whose rays all escape (a new path's output slot waits in a hot cell until its first SHADE stores it
with the radiance, so no record is ever written and MISS takes every slot from the hot cell); one-bounce paths (the first SHADE is the
last); other scenes at ten bounces."""
import functools
import os

import numpy as np
import pytest

import edge_scenes as E
import oracle
import util
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import types as T

pytestmark = pytest.mark.gpu

SKY_CAMERA = ((0.0, 40.0, 3.0), 0.0, 1.2, 1.2)  # high above house, looking up: no camera ray hits anything


@functools.lru_cache(maxsize=None)
def golden_env():
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "env_64x32.npz"))
    return R.Environment(g["rgba"], g["alias"].view(T.ALIAS_ENTRY).reshape(-1))


def camera_of(sc, sky):
    return E.camera(*SKY_CAMERA) if sky else sc.camera_uniform()


@functools.lru_cache(maxsize=None)
def reference(name, sky, w, h, count, mb):
    """The checker's sums and counters of samples [0, count) of scene `name` under the golden environment (computed once, read-only)."""
    sc = E.plain(name)
    img, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(golden_env()), np.asarray(camera_of(sc, sky)).view(oracle.CAMERA), w, h, 0, count, mb)
    img.setflags(write=False)
    return img, ost


def check(name, w, h, spp, mb, sky=False, ranges=None):
    """(begin, count) ranges into one accumulator of one context, enqueued back to back, against the checker's [0, spp)."""
    ref, ost = reference(name, sky, w, h, spp, mb)
    sc = E.plain(name)
    st = R.State.new(sc, golden_env(), w, h, camera=camera_of(sc, sky))
    try:
        st.max_bounces = mb
        for begin, count in ranges or [(0, spp)]:
            st.render_range(begin, count)
        img, s = st.download(), st.stats()
    finally:
        st.close()
    eq = util.bits(img) == util.bits(ref)
    assert eq.all(), int((~eq).any(axis=2).sum())
    assert (s["paths"], s["ext_rays"], s["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"])
    assert s["traversal_steps"] == 0  # the flat kernel ran (the tree walks count their steps)
    return ost


@pytest.mark.parametrize("quorum", ["100", "0"])
def test_triangle_vote_cuts_every_ray_or_none(quorum, monkeypatch):
    """RSRT_FLAT_QUORUM is read when the context is made.  100: a ray is cut short at every opportunity, its untested triangles parked in
    quad 3 of its record and read back by the TRACE trip that resumes it.  0: nothing ever touches quad 3."""
    monkeypatch.setenv("RSRT_FLAT_QUORUM", quorum)
    check("house", 64, 48, 4, 8)


def test_two_ranges_on_one_context():
    """[0, 5) then [5, 12): the second call's paths take slots whose records hold what the first call's last paths left"""
    check("house", 64, 48, 12, 8, ranges=[(0, 5), (5, 7)])


def test_twelve_single_sample_calls():
    """One sample a call: the small form of the kernel (160-slot pools), calls pipelined over the context's lanes, an arena per lane"""
    check("house", 64, 48, 12, 8, ranges=[(k, 1) for k in range(12)])


def test_ragged_frame():
    """67 x 35 at 3 spp: edge tiles in both directions, pools that are never full"""
    check("house", 67, 35, 3, 8)


def test_sky_camera():
    """Every camera ray escapes: MISS takes the output slot from the hot cell GEN left it in, next to a record no path of this frame
    ever wrote"""
    ost = check("house", 64, 48, 4, 8, sky=True)
    assert ost["ext_rays"] == ost["paths"] and ost["shadow_rays"] == 0


def test_one_bounce():
    """The first SHADE is the last: quads 1 and 2 are written for FINISH, quad 0 never"""
    ost = check("house", 64, 48, 4, 1)
    assert ost["shadow_rays"] > 0 and ost["ext_rays"] == ost["paths"]


@pytest.mark.parametrize("name", ["default", "cube"])
def test_other_scenes(name):
    check(name, 64, 48, 4, 10)
