"""The fog march's edge catalogue (tests/edge_fog.py) without a GPU: what makes the GPU comparison (test_fog_edges_gpu.py) mean
something.  Every case is one rsrt_fog_params_ok accepts and its restated records are finite; the cases reach the edges they are named
for (visibility mixed where geometry is met, dark inside the sphere, lit under the open sky; transmittance exactly 0 part-way along a
march); the seam between the closest hit (mode 0, with the brute-force fallback) and the shadow query (mode 1, the tree alone) is where
the contract puts it; and one sample of the published arithmetic (include/rsrt_fog.h, compiled for the CPU) is finite at every corner
of the accepted parameter set and just inside the bounds of its "Finiteness" rule, and equals the restatement bit for bit there."""
import ctypes as C
import itertools

import numpy as np
import pytest

import edge_fog as EF
import fog_ref
import foreign_trees
import oracle
import sky_ref
import util
from test_fog import c_params, host, ptr  # noqa: F401  (host: the fixture that compiles tests/cpp/fog_host.cpp)

F = np.float32
LARGEST = float(fog_ref.LARGEST)
SKY_ONLY = ("_sky", "camera_pole_up_sky", "camera_fov_1e-4_pole_up", "camera_far_1e6")  # scene-family names: no march meets geometry


# ---------------------------------------------------------------------------------------------------- the catalogue
def test_the_catalogue_holds_what_it_says():
    cases = EF.cases()
    assert len(EF.family("scene")) == len(EF.ES.cases()) == 45 and len(EF.family("tree")) == 15
    assert len(EF.family("param")) == len(EF.PARAM_EDGES) * len(EF.PARAM_SCENES) * 2 == 88
    for c in cases:
        assert (c.sample_begin, c.sample_count) == (3, 2) and c.w * c.h <= 48 * 32, c.name
        assert c.params["steps"] == 4 or any(s in c.name for s in ("steps_", "_steps")), c.name
        if c.family != "scene" or "_shape_" not in c.name:
            assert c.w <= 48 and c.h <= 32, c.name
    assert sorted((c.w, c.h) for c in cases if "_shape_house_" in c.name) == sorted(EF.ES.SHAPES)
    for name, k in EF.SCALED.items():  # the medium scaled with the scene: exact powers of two times 20 and 0.05
        p = EF.case("scene_" + name + ("_all_lit" if name in EF.SCALED_ALL_LIT else "")).params
        assert F(p["max_distance"]) == F(20.0) * F(2.0) ** F(k) and F(p["density"]) * F(2.0) ** F(k) == F(0.05)
    assert {EF.kernel_form(n) for n in EF.names("tree")} == {"lds", "global"}
    assert max(int(c.scene.bvh_nodes["primitives_len"].max()) for c in EF.family("tree")) >= 9  # leaves longer than the typed loops hold


@pytest.mark.parametrize("name", [c.name for c in EF.cases()])
def test_every_case_is_accepted_and_its_records_are_finite(name):
    c = EF.case(name)
    assert fog_ref.params_ok(c.params)
    rec, lit = EF.reference(name)
    assert rec.shape == (c.h, c.w, 4) and lit.shape == (c.sample_count, c.h, c.w, c.params["steps"])
    assert np.isfinite(rec).all() and (rec >= 0).all() and (rec[..., 3] <= c.sample_count).all()


def test_visibility_is_mixed_where_the_march_meets_geometry_and_plain_where_it_cannot():
    """Conditions, not measurements: a comparison in which every march point is lit (or none is) shows nothing about the shadow walk."""
    shares = {c.name: EF.shares(EF.reference(c.name)[1]) for c in EF.family("scene") + EF.family("tree")}
    for n in EF.names("tree"):
        assert shares[n][1] >= 0.1, (n, shares[n])
    assert sum(shares[n][1] >= 0.1 for n in EF.names("scene")) >= 15
    assert shares["scene_camera_inside_sphere"][0] == 0.0
    sky = [n for n in EF.names("scene") if any(s in n for s in SKY_ONLY)]
    assert len(sky) == 13  # nine scales outside SCALE_HIT, two pole-up cameras, two far cameras
    for n in sky:
        assert shares[n][0] == 1.0, (n, shares[n])
    # a scaled scene the checker still hits: mixed, or named for being kept for its march length alone
    for name in EF.SCALED:
        all_lit = name in EF.SCALED_ALL_LIT
        assert (shares["scene_" + name + ("_all_lit" if all_lit else "")][0] == 1.0) == all_lit, name


def test_every_case_is_of_the_recorded_kind():
    """tests/golden/fog_edge_cases.json: for each case the form of the kernel it runs and the restatement's lit and mixed shares, to
    three places, recorded when the catalogue was made — so that a case cannot change kind unnoticed, and a reader sees what each
    comparison on the GPU covers."""
    import json
    import os
    with open(os.path.join(util.ROOT, "tests", "golden", "fog_edge_cases.json")) as f:
        recorded = json.load(f)
    assert list(recorded) == [c.name for c in EF.cases()]
    for name, r in recorded.items():
        lit, mixed = EF.shares(EF.reference(name)[1])
        assert (EF.kernel_form(name), round(lit, 3), round(mixed, 3)) == (r["form"], r["lit"], r["mixed"]), name


def test_the_clamp_density_puts_exact_zeros_part_way_along_a_march():
    assert sky_ref.exp2(F(-EF.EXP2_CLAMP)) > 0 and sky_ref.exp2(np.nextafter(F(-EF.EXP2_CLAMP), F(-np.inf))) == 0
    for scene in EF.PARAM_SCENES:
        for jitter in (0, 1):
            c = EF.param_case(scene, "density_clamp_midway", jitter)
            k = fog_ref.prepare(c.params)
            T = np.concatenate([fog_ref.transmittance(k, t) for _, _, _, t, _ in EF.march(c.name)])  # [pixels, steps] of both samples
            some = (T == 0).any(axis=1) & (T > 0).any(axis=1)
            assert (T == 0).any() and (T > 0).any() and some.mean() > 0.25, (c.name, some.mean())


# ---------------------------------------------------------------------------------------------------- the fallback seam
def test_a_sphere_no_leaf_holds_ends_a_march_but_casts_no_shaft():
    """The closest hit is rsrt_cast_rays mode 0 (the tree, then every sphere and plane when the tree gave nothing); the shadow query is
    mode 1 (the tree alone).  In the scene with 60 spheres behind a 10-sphere tree some marches end on one of the 60, some march points
    have one of the 60 between them and the light — and are lit all the same: wherever the 60 stand, `lit` is what it was."""
    c = EF.case("tree_foreign_hidden_spheres")
    hidden = c.scene.spheres[foreign_trees.HIDDEN_FIRST:]
    centres, radius = hidden["pos"].astype(np.float64), hidden["radius"].astype(np.float64)
    away = foreign_trees.hidden_spheres_scene([(1.0e4 + 10.0 * i, -1.0e4, 1.0e4) for i in range(len(hidden))])
    light = np.asarray(c.params["light_dir"], np.float64)
    ended, shadowed = 0, 0
    _, lit = EF.reference(c.name)
    for s, (o, d, hits, t, pts) in enumerate(EF.march(c.name)):
        tree_alone = oracle.cast_rays(util.oracle_scene(c.scene), o, d, mode=1)
        on = (hits["did_hit"] != 0) & (tree_alone["did_hit"] == 0) & (hits["distance"] < F(c.params["max_distance"]))
        for p in hits["hit_point"][on].astype(np.float64):  # a hit the fallback alone found lies on a sphere of index 10 or more
            assert (np.abs(np.linalg.norm(centres - p, axis=1) - radius) < 1e-4).any()
        ended += int(on.sum())
        # float64: does the ray from a march point along light_dir pass through one of the 60 (by a margin the f32 test cannot undo)
        x = pts.reshape(-1, 1, 3).astype(np.float64)
        along = ((centres[None] - x) * light).sum(axis=-1)
        off = np.linalg.norm(centres[None] - x - along[..., None] * light, axis=-1)
        blocked = ((along > 0) & (off < 0.9 * radius)).any(axis=1).reshape(lit[s].reshape(len(o), -1).shape)
        shadowed += int((blocked & lit[s].reshape(blocked.shape)).sum())
        # the same shadow queries against the scene with the 60 moved far away
        dirs = np.broadcast_to(np.asarray(c.params["light_dir"], F), pts.shape)
        moved = oracle.cast_rays(util.oracle_scene(away), pts.reshape(-1, 3), dirs.reshape(-1, 3), mode=1)["did_hit"] == 0
        assert np.array_equal(moved.reshape(blocked.shape), lit[s].reshape(blocked.shape))
    assert ended >= 1 and shadowed >= 1, (ended, shadowed)


# ---------------------------------------------------------------------------------------------------- finiteness
CORNER_FIELDS = {"density": (0.0, 1.0e6), "albedo_r": (0.0, 1.0), "albedo_g": (0.0, 1.0), "albedo_b": (0.0, 1.0), "anisotropy": (-0.95, 0.95),
                 "light_irradiance": (0.0, LARGEST), "ambient": (0.0, LARGEST), "max_distance": (float(np.nextafter(F(0), F(1))), LARGEST),
                 "steps": (1, 64), "flags": (0, 1)}


def corner_sets():
    """Every combination of each scalar field at its least and its greatest accepted value (1024 of them), the light along SLANT."""
    for values in itertools.product(*CORNER_FIELDS.values()):
        kw = dict(zip(CORNER_FIELDS, values))
        kw["albedo"] = (kw.pop("albedo_r"), kw.pop("albedo_g"), kw.pop("albedo_b"))
        yield dict(kw, light_dir=EF.SLANT)


def probe_rays(p):
    """54 marches of one sample: d along the light, against it and across; a hit at 0, a hit at max_distance, a miss; xi 0, 0.5 and 1;
    every point lit, or none.  -> d, hit, t_hit, xi, lit"""
    light = np.asarray(p["light_dir"], F)
    combos = list(itertools.product((light, -light, F([1, 0, 0])), ((1, 0.0), (1, p["max_distance"]), (0, 0.0)), (0.0, 0.5, 1.0), (True, False)))
    d = np.ascontiguousarray([c[0] for c in combos], F)
    hit = np.array([c[1][0] for c in combos], np.int32)
    t_hit = np.array([c[1][1] for c in combos], F)
    xi = np.array([c[2] for c in combos], F)
    lit = np.repeat(np.array([c[3] for c in combos], bool)[:, None], p["steps"], axis=1)
    return d, hit, t_hit, xi, lit


def one_sample(host, p, rec=None):
    """(rsrt_fog_sample through the host library, fog_ref.sample) over probe_rays(p), each added to `rec` (zeros when None)."""
    d, hit, t_hit, xi, lit = probe_rays(p)
    got = np.zeros((len(d), 4), F) if rec is None else np.array(rec, F)
    want = got.copy()
    host.fog_sample(C.byref(c_params(p)), ptr(d), ptr(hit), ptr(t_hit), ptr(xi), ptr(np.ascontiguousarray(lit, np.uint8)), len(d), ptr(got))
    with np.errstate(all="ignore"):
        want = fog_ref.sample(fog_ref.prepare(p), d, hit != 0, t_hit, xi, lit, want)
    return got, want


def corner_report(host, accepts):
    """[(kw, NaN count, inf count)] of the corner sets `accepts` takes whose one-sample records are not all finite; the sets taken."""
    bad, taken = [], 0
    for kw in corner_sets():
        p = fog_ref.params(**kw)
        if not accepts(p):
            continue
        taken += 1
        got, want = one_sample(host, p)
        assert util.same_bits_or_nan(got, want), kw
        if not np.isfinite(got).all():
            bad.append((kw, int(np.isnan(got).sum()), int(np.isinf(got).sum())))
    return bad, taken


def test_one_sample_is_finite_at_every_corner_of_the_accepted_set(host):
    for kw in corner_sets():  # the header's check and its restatement agree on all 1024
        p = fog_ref.params(**kw)
        assert bool(host.fog_params_ok(C.byref(c_params(p)))) == fog_ref.params_ok(p), kw
    bad, taken = corner_report(host, fog_ref.params_ok)
    assert 200 <= taken <= 1024 and not bad, (taken, bad[:3])


ISSUE_SETTING = dict(light_dir=EF.SLANT, max_distance=20.0, steps=5, flags=0)
REFUSED = [{"light_irradiance": LARGEST, "density": 1.0e6}, {"ambient": LARGEST, "density": 1.0e6}, {"light_irradiance": LARGEST, "anisotropy": 0.95, "density": 1.0}]


def test_products_of_accepted_values_that_overflow_are_refused(host):
    """Each field alone is within its range; S_sun or S_amb is inf (and T_i exactly 0 beyond the clamp: NaN), or the phase of 62 times
    the largest irradiance is.  The same sets with the other factor small are accepted and finite."""
    for kw in REFUSED:
        for base in ({}, ISSUE_SETTING):
            p = fog_ref.params(**dict(base, **kw))
            assert not fog_ref.params_ok(p) and not host.fog_params_ok(C.byref(c_params(p))), kw
            got, _ = one_sample(host, p)
            assert not np.isfinite(got).all()  # (what the rule is there to keep out)
    for kw in ({"light_irradiance": LARGEST}, {"ambient": LARGEST}, {"light_irradiance": LARGEST, "anisotropy": 0.95, "density": 1.0e-4}):
        p = fog_ref.params(**dict(ISSUE_SETTING, **dict(kw, max_distance=1.0)))
        assert fog_ref.params_ok(p) and host.fog_params_ok(C.byref(c_params(p))), kw
        assert np.isfinite(one_sample(host, p)[0]).all()


def last_accepted(field, lo, hi, **kw):
    """The greatest float32 value of `field` in [lo, hi] that rsrt_fog_params_ok accepts beside `kw` (lo is accepted, hi is not)."""
    lo, hi = F(lo), F(hi)
    ok = lambda v: fog_ref.params_ok(fog_ref.params(**dict(kw, **{field: float(v)})))  # noqa: E731
    assert ok(lo) and not ok(hi)
    while np.nextafter(lo, hi) != hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return float(lo)


@pytest.mark.parametrize("field,lo,hi,kw", [
    ("light_irradiance", 1.0, LARGEST, {"density": 1.0e6}), ("light_irradiance", 1.0, LARGEST, {"density": 1.0e6, "steps": 64, "max_distance": 1.0e-30}),
    ("ambient", 1.0, LARGEST, {"density": 1.0e6}), ("ambient", 1.0, LARGEST, {"density": 1.0e6, "steps": 1, "max_distance": 1.0e30}),
    ("light_irradiance", 1.0, LARGEST, {"density": 1.0, "anisotropy": 0.95}), ("light_irradiance", 1.0, LARGEST, {"density": 1.0, "anisotropy": -0.95, "steps": 1}),
    ("density", 0.0, 1.0e6, {"light_irradiance": LARGEST}), ("density", 0.0, 1.0e6, {"ambient": LARGEST}), ("density", 0.0, 1.0e6, {"ambient": LARGEST, "steps": 1}),
    ("density", 0.0, 1.0e6, {"ambient": LARGEST, "steps": 64, "max_distance": 3.0e4}), ("max_distance", 1.0, 1.0e30, {"ambient": 1.0e38, "density": 1.0e-3, "steps": 2}),
    ("ambient", 1.0, LARGEST, {"albedo": (0.0, 1.0, 0.0), "density": 3.0})])
def test_one_sample_is_finite_just_inside_the_rule(host, field, lo, hi, kw):
    """The last parameter set the rule accepts along one field, found by bisection: the march itself — every point lit, xi = 0, along
    the light — is finite there, so the rule's bounds hold where they bind, and the header's check agrees with the restatement at both
    neighbours."""
    kw = dict(kw, light_dir=EF.SLANT)
    v = last_accepted(field, lo, hi, **kw)
    inside, outside = fog_ref.params(**dict(kw, **{field: v})), fog_ref.params(**dict(kw, **{field: float(np.nextafter(F(v), F(hi)))}))
    assert host.fog_params_ok(C.byref(c_params(inside))) and not host.fog_params_ok(C.byref(c_params(outside)))
    got, want = one_sample(host, inside)
    assert util.bits(got).tolist() == util.bits(want).tolist() and np.isfinite(got).all()
    # a record summed over many samples may overflow: to +inf, never to NaN
    rec = got
    for _ in range(200):
        rec, want = one_sample(host, inside, rec)
        assert util.same_bits_or_nan(rec, want)
    assert not np.isnan(rec).any() and (rec >= 0).all()
    if fog_ref.source_bound(inside) * fog_ref.length_bound(inside) > F(1.0e37):
        assert np.isinf(rec[..., :3]).any()
