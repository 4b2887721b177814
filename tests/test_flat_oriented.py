"""The flat traversal's per-octant leaf tables (rt_scene_image.h build_scene_image, rt_device.h trace_flat): each leaf box stored once per ray-sign
octant with its corners in slab order, so the leaf loop needs no min / max to order a box's slab values.

CPU: the oriented slab decision equals the min / max one bit for bit on adversarial (box, ray) pairs, and the table layout (which
corner goes where, the stride that keeps a wave's eight octant reads in different LDS cells).  GPU: the flat probe and a house frame
against the oracle, on waves of mixed octants, of one octant and of nearly axis-parallel rays, and on a scene whose tables do not fit
beside the pools (it keeps the loop that orders the values itself)."""
import numpy as np
import pytest

F = np.float32
RT_INFINITY = F(1.70141183460469231732e+38)
SMALL_IMAGE_BYTES = 24 * 1024  # (rsrt_api.hip kSmallImageBytes: the whole image goes to LDS up to this size; test_scene_image.py holds it against what the library reports)


def minmax_miss(lo, hi, o, inv):
    """The loop without tables: both corners, each axis's two values put in order by min / max."""
    a, b = (lo - o) * inv, (hi - o) * inv
    t0 = np.maximum(np.maximum(np.maximum(np.minimum(a[:, 0], b[:, 0]), np.minimum(a[:, 1], b[:, 1])), np.minimum(a[:, 2], b[:, 2])), F(0))
    t1 = np.minimum(np.minimum(np.minimum(np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])), np.maximum(a[:, 2], b[:, 2])), RT_INFINITY)
    return t0 > t1, t0, t1


def oriented_miss(near, far, o, inv):
    """The loop with tables: near corner, far corner, no ordering."""
    a, b = (near - o) * inv, (far - o) * inv
    t0 = np.maximum(np.maximum(np.maximum(a[:, 0], a[:, 1]), a[:, 2]), F(0))
    t1 = np.minimum(np.minimum(np.minimum(b[:, 0], b[:, 1]), b[:, 2]), RT_INFINITY)
    return t0 > t1, t0, t1


def octant_of(inv):
    return (inv[:, 0] < 0).astype(np.uint32) | ((inv[:, 1] < 0).astype(np.uint32) << 1) | ((inv[:, 2] < 0).astype(np.uint32) << 2)


def orient(lo, hi, q):
    """The corners of box (lo, hi) for octant q (bit 0 x, bit 1 y, bit 2 z): near = the max corner on the axes whose bit is set."""
    bits = np.stack([(q >> k) & 1 for k in range(3)], axis=-1).astype(bool)
    return np.where(bits, hi, lo), np.where(bits, lo, hi)


def build_tables(lo, hi, lo_mask, hi_mask):
    """Python statement of build_scene_image's table builder (test_scene_image.py compares the two): [8 octants][stride] float4, leaf k at 2k: {near.xyz, mask lo}{far.xyz, mask hi}."""
    n = len(lo)
    stride = 2 * (n | 1)
    t = np.zeros((8 * stride, 4), np.float32)
    for q in range(8):
        near, far = orient(lo, hi, np.uint32(q))
        t[q * stride + 2 * np.arange(n), :3] = near
        t[q * stride + 2 * np.arange(n) + 1, :3] = far
        t[q * stride + 2 * np.arange(n), 3] = lo_mask.view(np.float32)
        t[q * stride + 2 * np.arange(n) + 1, 3] = hi_mask.view(np.float32)
    return t, stride


def adversarial_pairs(n, rng):
    """Boxes with zero extent on an axis, origins on a face, direction components down to near-subnormal (1/d huge but finite), huge
    coordinates (slab values past RT_INFINITY or overflowing to infinity), every octant."""
    lo = rng.uniform(-4, 4, (n, 3)).astype(F)
    ext = rng.uniform(0, 3, (n, 3)).astype(F)
    flat_axis = rng.integers(0, 4, n)  # 3: no flat axis
    for k in range(3):
        ext[flat_axis == k, k] = 0
    hi = (lo + ext).astype(F)
    o = rng.uniform(-6, 6, (n, 3)).astype(F)
    face = rng.integers(0, 7, n)  # origin on a face of the box (0..5), or anywhere (6)
    for k in range(3):
        o[face == 2 * k, k] = lo[face == 2 * k, k]
        o[face == 2 * k + 1, k] = hi[face == 2 * k + 1, k]
    d = rng.normal(size=(n, 3)).astype(F)
    kind = rng.integers(0, 6, n)
    tiny = rng.integers(0, 3, n)
    scale = np.where(kind == 1, F(1e-37), np.where(kind == 2, F(3e-39), np.where(kind == 3, F(1e-20), F(1))))  # near-subnormal components: 1/d up to ~1e38
    d[np.arange(n), tiny] *= scale
    huge = kind == 4  # coordinates near the top of the f32 range
    lo[huge] *= F(1e37)
    hi[huge] *= F(1e37)
    o[huge] *= F(1e37)
    hi = np.maximum(hi, lo)
    signs = rng.integers(0, 8, n)  # every octant equally often, whatever the draws above
    for k in range(3):
        d[:, k] = np.abs(d[:, k]) * np.where((signs >> k) & 1, F(-1), F(1))
    d[d == 0] = F(1e-30)
    with np.errstate(divide="ignore", over="ignore"):
        inv = (F(1) / d).astype(F)
    ok = np.all(np.isfinite(inv), axis=1)  # the flat loop only takes rays whose 1/d is finite
    return lo[ok], hi[ok], o[ok], inv[ok]


def test_oriented_slab_decision_equals_minmax_decision_bit_for_bit():
    rng = np.random.default_rng(2026)
    total, octants = 0, set()
    with np.errstate(over="ignore", invalid="raise"):
        for _ in range(6):
            lo, hi, o, inv = adversarial_pairs(200_000, rng)
            q = octant_of(inv)
            near, far = orient(lo, hi, q)
            m0, a0, b0 = minmax_miss(lo, hi, o, inv)
            m1, a1, b1 = oriented_miss(near, far, o, inv)
            assert np.array_equal(m0, m1), int((m0 != m1).sum())
            # (the values themselves agree too, up to the sign of a zero)
            assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
            total += len(q)
            octants |= set(np.unique(q).tolist())
            assert m0.any() and (~m0).any()
    assert total >= 1_000_000 and octants == set(range(8))


def test_rt_infinity_clamp_is_part_of_the_decision():
    """t_1's min with RT_INFINITY is not a no-op: a box entered beyond RT_INFINITY is a miss (the loop keeps it)."""
    lo, hi = np.array([[3e38, -1, -1]], F), np.array([[3.2e38, 1, 1]], F)
    o, inv = np.zeros((1, 3), F), np.ones((1, 3), F)
    m, t0, t1 = oriented_miss(lo, hi, o, inv)
    assert m[0] and t0[0] > RT_INFINITY


def test_table_builder_puts_each_corner_in_place():
    rng = np.random.default_rng(7)
    for n in (1, 5, 8, 20, 32):
        lo = rng.uniform(-5, 5, (n, 3)).astype(F)
        hi = (lo + rng.uniform(0, 2, (n, 3))).astype(F)
        ml, mh = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        t, stride = build_tables(lo, hi, ml, mh)
        assert stride % 2 == 0 and (stride // 2) % 2 == 1 and stride >= 2 * n
        for q in range(8):
            for k in range(n):
                c0, c1 = t[q * stride + 2 * k], t[q * stride + 2 * k + 1]
                for ax in range(3):
                    near, far = (hi[k, ax], lo[k, ax]) if (q >> ax) & 1 else (lo[k, ax], hi[k, ax])
                    assert c0[ax] == near and c1[ax] == far
                assert c0[3:].view(np.uint32)[0] == ml[k] and c1[3:].view(np.uint32)[0] == mh[k]
        # a wave of mixed octants reads leaf k of up to eight tables at once: eight different 16-byte cells of the 256-byte bank row
        for k in range(n):
            for half in (0, 1):
                cells = {(q * stride + 2 * k + half) % 16 for q in range(8)}  # (float4 index mod 16: the cell of the row)
                assert len(cells) == 8


def image_f4(sc, tables):
    """float4s of the scene's LDS image (rt_scene_image.h build_scene_image): what decides whether the tables fit."""
    nn = len(sc.bvh_nodes)
    leaves = int((sc.bvh_nodes["primitives_len"] > 0).sum())
    f4 = (2 * nn + 4 * len(sc.primitives) + 3 * len(sc.triangles) + 4 * len(sc.materials) + 4 * len(sc.spheres) + 4 * len(sc.planes)
          + (8 * nn + 3) // 4 + 2 * leaves)
    return f4 + (8 * 2 * (leaves | 1) if tables else 0)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
FLAT_PROBES = (3 << 1, (3 << 1) | 16)  # flat traversal, scene from global memory / from LDS as the production kernel stages it


def _rays(kind, n, rng, center):
    o = (rng.uniform(-3, 3, (n, 3)) + center).astype(F)
    d = rng.normal(size=(n, 3))
    if kind == "single":  # every wave of 64 rays in one octant (a different one each wave)
        q = (np.arange(n) // 64) % 8
        for k in range(3):
            d[:, k] = np.abs(d[:, k]) * np.where((q >> k) & 1, -1.0, 1.0)
    elif kind == "axis":  # nearly axis-parallel: two tiny components, 1/d large but finite, signs mixed within the wave
        axis = rng.integers(0, 3, n)
        tiny = rng.choice([1e-3, 1e-7, 1e-12, 1e-20, 1e-30], size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
        d = tiny
        d[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(F)


def _probe_all(sc, rng, n=8192):
    import oracle
    import util
    import rsoderh_raytracing_amd as R
    osc = util.oracle_scene(sc)
    st = R.State.new(sc, util.small_env(), 16, 16)
    try:
        center = (sc.bvh_nodes[0]["bounds_min"] + sc.bvh_nodes[0]["bounds_max"]) / 2
        for kind in ("mixed", "single", "axis"):
            o, d = _rays(kind, n, rng, center)
            for mode in FLAT_PROBES:
                for bvh_only in (0, 1):
                    ref = oracle.cast_rays(osc, o, d, bvh_only, 0).view(np.uint32).reshape(-1, 9)
                    got = np.ascontiguousarray(st.cast_rays(o, d, mode | bvh_only, 0)).view(np.uint32).reshape(-1, 9)
                    assert np.array_equal(got, ref), (kind, mode | bvh_only, int((got != ref).any(axis=1).sum()))
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["house", "default", "cube"])
def test_flat_probe_with_tables_matches_oracle(name):
    import util
    import rsoderh_raytracing_amd as R
    sc = R.Scene.load_toml(util.scene_path(name))
    assert image_f4(sc, True) * 16 <= SMALL_IMAGE_BYTES  # (the tables are staged)
    _probe_all(sc, np.random.default_rng(31))


def _house_without_room():
    """house with extra (unused) materials: its image still fits LDS beside the pools, the image with the tables does not."""
    import util
    import rsoderh_raytracing_amd as R
    sc = R.Scene.load_toml(util.scene_path("house"))
    mats = np.zeros(len(sc.materials) + 180, sc.materials.dtype)
    mats[:len(sc.materials)] = sc.materials
    mats[len(sc.materials):] = sc.materials[0]
    big = R.Scene(mats, sc.spheres, sc.plane_descs, sc.vertices, sc.normals, sc.triangles, sc.camera_desc, planes=sc.planes,
                  primitives=sc.primitives, bvh_nodes=sc.bvh_nodes, bvh_depth=sc.bvh_depth)
    assert image_f4(big, False) * 16 <= SMALL_IMAGE_BYTES < image_f4(big, True) * 16
    return big


@pytest.mark.gpu
def test_scene_without_room_for_tables_keeps_the_minmax_loop_exact():
    import oracle
    import util
    sc = _house_without_room()
    _probe_all(sc, np.random.default_rng(32), n=4096)
    env = util.small_env()
    img, stats = _render(sc, env, 64, 36, 2, 8)
    ref, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(env), sc.camera_uniform().view(oracle.CAMERA), 64, 36, 0, 2, 8)
    assert np.array_equal(util.bits(img), util.bits(ref))
    assert (stats["ext_rays"], stats["shadow_rays"]) == (ost["ext_rays"], ost["shadow_rays"])


def _render(sc, env, w, h, spp, bounces):
    import rsoderh_raytracing_amd as R
    st = R.State.new(sc, env, w, h, device=0)
    try:
        st.max_bounces = bounces
        st.render_samples(spp)
        return st.download(), st.stats()
    finally:
        st.close()


@pytest.mark.gpu
def test_house_frame_with_tables_matches_oracle_bit_for_bit():
    import oracle
    import util
    import rsoderh_raytracing_amd as R
    sc = R.Scene.load_toml(util.scene_path("house"))
    env = R.Environment.synthetic(256, 128)
    w, h, spp, bounces = 160, 90, 4, 8
    img, stats = _render(sc, env, w, h, spp, bounces)
    ref, ost = oracle.render(util.oracle_scene(sc), util.oracle_env(env), sc.camera_uniform().view(oracle.CAMERA), w, h, 0, spp, bounces)
    assert np.array_equal(util.bits(img), util.bits(ref))
    assert (stats["ext_rays"], stats["shadow_rays"]) == (ost["ext_rays"], ost["shadow_rays"])
