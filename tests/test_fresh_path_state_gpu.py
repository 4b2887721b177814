"""The flat kernel writes nothing of a new path's constant state (throughput 1, radiance 0, last pdf 1) to the arena: the stage that
picks a path up first — SHADE, or MISS when the camera ray escapes — takes the constants because the bounce count in the slot's tag
word is still 0, and reads past whatever the slot's previous path left in the columns (rt_wavepool.h, kFreshInCt).  Every frame here is
the checker's bit for bit with the checker's path and ray counts: frames whose camera rays all escape (MISS is every path's first and
only stage), frames that mix escapes and hits, one-bounce paths (first SHADE is the last), paths that end at their first vertex on a
debug colour, inf and NaN throughputs left behind in a slot by the path before, slots that are reused many times within a call and
across calls, single-sample calls (the small form of the kernel on pipelined lanes, an arena each), a ragged frame."""
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
HOUSE_CAMERAS = {"own": None, "sky": SKY_CAMERA, "ground": ((0.0, 6.0, 12.0), 0.0, -0.6, 1.2)}


@functools.lru_cache(maxsize=None)
def golden_env():
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "env_64x32.npz"))
    return R.Environment(g["rgba"], g["alias"].view(T.ALIAS_ENTRY).reshape(-1))


def camera_of(sc, view):
    return sc.camera_uniform() if HOUSE_CAMERAS[view] is None else E.camera(*HOUSE_CAMERAS[view])


@functools.lru_cache(maxsize=None)
def reference(name, view, w, h, begin, count, mb):
    """The checker's sums and counters of scene `name` under the golden environment (computed once; callers must not write into it)."""
    sc = E.plain(name)
    img, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(golden_env()), np.asarray(camera_of(sc, view)).view(oracle.CAMERA), w, h, begin, count, mb)
    img.setflags(write=False)
    return img, ost


def render(sc, env, w, h, ranges, mb, cam):
    """(begin, count) ranges into one accumulator, enqueued back to back -> sums, the counters of all the calls together."""
    st = R.State.new(sc, env, w, h, camera=cam)
    try:
        st.max_bounces = mb
        for begin, count in ranges:
            st.render_range(begin, count)
        return st.download(), st.stats()
    finally:
        st.close()


def same(img, s, ref, ost, nan_policy=False):
    if nan_policy:
        assert util.same_bits_or_nan(img, ref)
    else:
        eq = util.bits(img) == util.bits(ref)
        assert eq.all(), int((~eq).any(axis=2).sum())
    assert (s["paths"], s["ext_rays"], s["shadow_rays"]) == (ost["paths"], ost["ext_rays"], ost["shadow_rays"])
    assert s["traversal_steps"] == 0  # the flat kernel ran (the tree walks count their steps)


def check(name, w, h, spp, mb, view="own", ranges=None):
    ref, ost = reference(name, view, w, h, 0, spp, mb)
    sc = E.plain(name)
    img, s = render(sc, golden_env(), w, h, ranges or [(0, spp)], mb, camera_of(sc, view))
    same(img, s, ref, ost)
    return ost


def test_every_camera_ray_escapes():
    """MISS is the first and the last stage of every path: throughput 1, radiance 0 and last pdf 1 all come from the bounce count."""
    ost = check("house", 64, 48, 4, 8, view="sky")
    assert ost["ext_rays"] == ost["paths"] and ost["shadow_rays"] == 0


@pytest.mark.parametrize("mb", [1, 2, 8])
@pytest.mark.parametrize("view", ["own", "ground"])
def test_house_hits_and_escapes(view, mb):
    """Escapes next to hits in one wave's pool: slots whose last path went eight bounces deep are handed to paths that end at once.
    At one bounce the first SHADE is the path's last stage but for its shadow ray."""
    ost = check("house", 64, 48, 4, mb, view=view)
    assert ost["shadow_rays"] > 0 and ost["ext_rays"] > ost["paths"] * (mb > 1)


@pytest.mark.parametrize("name", ["spheres_only", "cube", "default"])
def test_open_scenes(name):
    check(name, 64, 48, 4, 10)


@pytest.mark.parametrize("name", [c.name for c in E.family("materials", "normals")])
def test_slots_left_with_inf_and_nan(name):
    """edge_scenes' material grid (emission 3e38, colour 1.5: inf radiance and throughputs above 1 stay behind in a slot; debug colours
    end a path at its first vertex) and its wall of zero-length and cancelling vertex normals (NaN throughput stays behind): the next
    path in the slot must not see any of it.  The checker's result as edge_scenes keeps it, under its NaN policy."""
    c = E.case(name)
    ref, ost = E.reference(name)
    img, s = render(c.scene, c.env, c.w, c.h, [(c.sample_begin, c.sample_count)], c.max_bounces, c.camera)
    same(img, s, ref, ost, nan_policy=name in E.NAN_OR_INF_CASES)


def test_ragged_frame():
    """67 x 35, 3 spp: edge tiles in both directions (slots offered an out-of-frame pixel stay free and are offered again)"""
    check("house", 67, 35, 3, 8)


def test_sixteen_single_sample_calls_equal_one_call():
    """One sample a call: the small form of the kernel, calls pipelined over the context's lanes, each lane's arena holding what the
    call before it on that lane left there."""
    check("house", 64, 48, 16, 8)
    check("house", 64, 48, 16, 8, ranges=[(k, 1) for k in range(16)])


def test_split_sample_ranges_compose():
    """[0, 5) then [5, 12) into one accumulator == the checker's twelve samples: the second call starts on the first call's arena"""
    check("house", 64, 48, 12, 8, ranges=[(0, 5), (5, 7)])
