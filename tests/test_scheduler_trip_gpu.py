"""The flat kernel's scheduler keeps its five stage counts from trip to trip (rt_wavepool.h, settle: the slots that ran leave the stage,
a ballot over their new tags says where to), picks the stage on packed keys (rt_pool_pick.h) and compacts with v_mbcnt.  None of that
may move a scheduling decision, and nothing a path computes depends on it: every frame here is the checker's bit for bit, with the
checker's path and ray counts.  A count that drifted would show as a wrong frame — a stage run past the end of its list takes a
slot twice, and a pool that believes itself empty ends with paths missing — so the cases are chosen where the bookkeeping can go
wrong, not by the workload's shape:
  underfilled pools   1 x 1 and 7 x 5 at 1 spp: a wave's pool is never filled, exhaustion arrives with most slots FREE, they are
                      parked IDLE, and what finishes later becomes FREE without reviving GEN
  ragged edges        33 x 17 at 9 spp: partial edge tiles (out-of-frame slots stay FREE and are offered again: GEN's count takes
                      them back) and a partial last sample block
  stage runs > 64     64 x 48 at 16 spp: more than 64 slots wait in one stage; the `pos < 64` cut, the second trip, n_run < best_n
  stage coverage      1 bounce (every path ends in FINISH or at its first SHADE) and 8 bounces (every stage; in house the
                      triangle-loop vote's resumed rays, a TRACE -> TRACE exit, forced at every opportunity by RSRT_FLAT_QUORUM=100)
  every flat form     rsrt_render can select for these scenes: <1, 1024, 192, 2> (the default), and the small form <1, 256, 160, 2>
                      both through RSRT_KERNEL=2 and through back-to-back single-sample calls.  The all-global and the hybrid flat
                      forms (<0, 256, 160, 2>, <2, 1024, 192, 2>) are compiled but no render call reaches them: a scene the flat
                      traversal accepts (at most 64 records) always fits the LDS whole.  tests/test_code_object.py reads their
                      code objects.
The instrumented build compares the kept counts with a census of every tag on every trip (tools/simd_efficiency.py prints the
mismatches); this file is the product build's check."""
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


@functools.lru_cache(maxsize=None)
def golden_env():
    g = np.load(os.path.join(util.ROOT, "tests", "golden", "env_64x32.npz"))
    return R.Environment(g["rgba"], g["alias"].view(T.ALIAS_ENTRY).reshape(-1))


@functools.lru_cache(maxsize=None)
def reference(name, w, h, count, mb):
    """The checker's sums and counters of samples [0, count) of scene `name` under the golden environment (computed once, read-only)."""
    sc = E.plain(name)
    img, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(golden_env()), sc.camera_uniform().view(oracle.CAMERA), w, h, 0, count, mb)
    img.setflags(write=False)
    return img, ost


def check(name, w, h, spp, mb, ranges=None):
    """(begin, count) ranges into one accumulator of one context, enqueued back to back, against the checker's [0, spp)."""
    ref, ost = reference(name, w, h, spp, mb)
    sc = E.plain(name)
    st = R.State.new(sc, golden_env(), w, h)
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


FORMS = ["default", "small"]


def select_form(monkeypatch, form):
    """RSRT_KERNEL is read when the context is made: 2 = the small form (256-thread workgroups, 160-slot pools) for every job."""
    if form == "small":
        monkeypatch.setenv("RSRT_KERNEL", "2")
    else:
        monkeypatch.delenv("RSRT_KERNEL", raising=False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5)])
@pytest.mark.parametrize("mb", [1, 8])
def test_underfilled_pool(w, h, mb, form, monkeypatch):
    select_form(monkeypatch, form)
    ost = check("house", w, h, 1, mb)
    assert ost["paths"] == w * h


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["house", "default"])
def test_ragged_edges(name, form, monkeypatch):
    select_form(monkeypatch, form)
    check(name, 33, 17, 9, 8)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mb", [1, 8])
@pytest.mark.parametrize("name", ["house", "default", "spheres_only", "cube"])
def test_stage_runs_of_more_than_64_slots(name, mb, form, monkeypatch):
    select_form(monkeypatch, form)
    ost = check(name, 64, 48, 16, mb)
    if mb == 1:
        assert ost["ext_rays"] == ost["paths"]  # the first SHADE is the last: what goes on goes to FINISH


@pytest.mark.parametrize("form", FORMS)
def test_every_ray_resumed(form, monkeypatch):
    """RSRT_FLAT_QUORUM=100 (read when the context is made): the triangle-loop vote cuts a ray short at every opportunity, so TRACE
    leaves slots in TRACE again and again — the one exit that moves no count"""
    select_form(monkeypatch, form)
    monkeypatch.setenv("RSRT_FLAT_QUORUM", "100")
    check("house", 64, 48, 16, 8)


def test_single_sample_calls():
    """One sample a call, sixteen calls back to back: the calls behind a running kernel take the small form on the context's lanes"""
    check("house", 64, 48, 16, 8, ranges=[(k, 1) for k in range(16)])


def test_single_sample_calls_on_a_ragged_frame():
    check("house", 33, 17, 9, 8, ranges=[(k, 1) for k in range(9)])
