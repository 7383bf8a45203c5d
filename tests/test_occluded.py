"""-m gpu: the any-hit occlusion query (rtmi_occluded / rtmi_occluded_device) against its definition (tests/occluded_ref.py, from
the oracle's closest hits), every byte: the octree walk's any-hit mode (k_occluded_oct), the linear list (k_occluded_linear) and
the closest-hit + k_occl_from_hits path (generic tree, BVH mode, analytic spheres)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import (TEAPOT, OracleApi, ProductApi, build_pair, recipe_axis_box, recipe_canonical, recipe_circles_analytic)
import occluded_ref as OR

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _check(c, sp, o4, d4, tmax, want, what):
    got, st = c.occluded(sp, o4, d4, tmax)
    assert got.dtype == np.uint8 and got.shape == want.shape and got.max(initial=0) <= 1, what
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} answers differ, first rays {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"
    assert st["rays"] == len(want) and st["trace_launches"] == 1 and st["streams"] == 1 and st["trace_ms"] > 0 and st["kernel_ms"] > 0
    return got, st


def _families(c, so, sp, o4, d4, what, spheres=False, names=None, tri_t=None):
    """Every tmax family against the definition; (tri, t): the closest hits the definition starts from (default: the oracle's)"""
    tri, t = tri_t if tri_t is not None else OR.closest_hits(so, o4, d4, spheres)[:2]
    fam = OR.tmax_families(t, seed=len(t))
    for name in (names or fam):
        _check(c, sp, o4, d4, fam[name], OR.from_hits(tri, t, fam[name]), f"{what}, tmax {name}")
    return tri, t, fam


@pytest.fixture(scope="module")
def primary(canonical_pair):
    orc = _orc()
    o4, d4 = orc.primary_rays(64, 64, orc.canonical_viewport(64, 64), 1)
    return o4, d4


def test_primary_rays_canonical_every_tmax_family(canonical_pair, primary):
    so, sp = canonical_pair
    o4, d4 = primary
    c = _R().HipRayCaster()
    tri, t, fam = _families(c, so, sp, o4, d4, "primary rays")
    hit = tri != 0
    assert hit.sum() > 500
    # what the families must give whatever the oracle says: nothing at tmax = t, every hit ray one ulp further
    assert not c.occluded(sp, o4, d4, fam["t"])[0].any()
    assert np.array_equal(c.occluded(sp, o4, d4, fam["nextafter"])[0] != 0, hit)
    assert np.array_equal(c.occluded(sp, o4, d4, None)[0], c.occluded(sp, o4, d4, fam["inf"])[0])


def test_random_rays_canonical_random_tmax(canonical_pair):
    so, sp = canonical_pair
    o4, d4, rng = OR.random_rays_canonical()
    tmax = rng.uniform(0, 20, o4.shape[0]).astype(F32)
    want = OR.expected(so, o4, d4, tmax)
    assert 0.02 < want.mean() < 0.98
    _check(_R().HipRayCaster(), sp, o4, d4, tmax, want, "random rays")


def test_shadow_segments(canonical_pair, primary):
    so, sp = canonical_pair
    so4, sd4, dist = OR.shadow_segments(so, *primary)
    want = OR.expected(so, so4, sd4, dist)
    assert 0.05 <= want.mean() <= 0.95
    c = _R().HipRayCaster()
    _check(c, sp, so4, sd4, dist, want, "shadow segments")
    _check(c, sp, so4, sd4, None, OR.expected(so, so4, sd4, None), "shadow rays without a limit")


def test_edge_case_rays_axis_box():
    """Zero direction components, origins on planes, NaN / inf rays, and hit times that are NaN or inf: a NaN accumulator
    sticks, so a real hit found behind it must not answer 1."""
    so, sp = build_pair(recipe_axis_box())
    o4, d4 = OR.edge_case_rays()
    tri, t, _ = _families(_R().HipRayCaster(), so, sp, o4, d4, "axis box", names=("null", "inf", "t", "nextafter", "mix"))
    assert (tri != 0).sum() > 100 and (~np.isfinite(t[tri != 0])).any()  # the degenerate "hits" are in the set


def test_linear_list_scene():
    """BASELINE config 2's recipe at the small size of test_render_linear_list_config2_small: one leaf, k_occluded_linear; and
    the axis-box scene as one list (NaN / inf hit times, ties) with a ragged last block"""
    orc, R = _orc(), _R()
    so, sp = build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))
    o4, d4 = orc.primary_rays(33, 31, orc.canonical_viewport(33, 31), 1)
    c = R.HipRayCaster()
    tri, _, _ = _families(c, so, sp, o4, d4, "linear list")
    assert (tri != 0).sum() > 100

    def relist(api):
        s = recipe_axis_box()(api)
        s.build_trivial_bounding_box([0.0, 0.0, 4.0], 4.0)
        return s
    so, sp = relist(OracleApi(orc)), relist(ProductApi(R))
    o4, d4 = OR.edge_case_rays()
    _families(c, so, sp, o4, d4, "axis box as one list", names=("null", "t", "nextafter", "mix"))


def test_option_generic_against_the_oracle(canonical_pair, primary):
    so, sp = canonical_pair
    R = _R()
    _families(R.HipRayCaster(options=R.OPT_GENERIC), so, sp, *primary, "RTMI_OPT_GENERIC", names=("null", "t", "nextafter", "half", "mix"))


@pytest.mark.parametrize("opt", ["OPT_BVH", "OPT_FAST"])
def test_options_bvh_and_fast_against_their_own_trace(canonical_pair, opt):
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(options=getattr(R, opt))
    o4, d4, _ = OR.random_rays_canonical(n=6000)
    tri, t, _, _ = c.trace(sp, o4, d4)
    assert (tri != 0).sum() > 200
    _families(c, so, sp, o4, d4, opt, names=("null", "t", "nextafter", "half", "mix"), tri_t=(tri, t))


def test_analytic_spheres():
    """The circles scene with analytic spheres: a sphere hit that replaces the tree's is the (tri, t) of the rule"""
    so, sp = build_pair(recipe_circles_analytic())
    rng = np.random.default_rng(4)
    n = 4000
    o4 = np.zeros((n, 4), F32)
    d4 = np.zeros((n, 4), F32)
    o4[:, :3] = rng.uniform(-3, 3, (n, 3)) + np.array([0.5, 0.5, 5.0])
    d = rng.normal(size=(n, 3))
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    tri, t, _ = _families(_R().HipRayCaster(), so, sp, o4, d4, "analytic spheres", spheres=True)
    ntris = so.num_tris()
    assert (tri >= ntris).sum() > 300 and ((tri > 0) & (tri < ntris)).sum() > 100


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_triangle_soups(seed):
    orc, R = _orc(), _R()
    recipe, (w, h, pos, aim) = OR.soup_recipe(seed)
    so, sp = recipe(OracleApi(orc)), recipe(ProductApi(R))
    assert so.num_tris() == sp.num_tris()
    vo = orc.create_viewport(w, h, (1.0, 0.7), pos, orc.unit(aim), 75.0, 0.1)
    o4, d4 = orc.primary_rays(w, h, vo, 1)
    _families(R.HipRayCaster(), so, sp, o4, d4, f"soup {seed}", names=("null", "t", "nextafter", "half", "mix"))


def test_counters_report_the_work_done(canonical_pair, primary):
    so, sp = canonical_pair
    o4, d4 = primary
    R = _R()
    c = R.HipRayCaster(options=R.OPT_COUNTERS)
    n = o4.shape[0]
    _, _, _, cn = so.trace(o4, d4)
    for name, tmax in (("zero", np.zeros(n, F32)), ("nan", np.full(n, np.nan, F32))):
        got, st = c.occluded(sp, o4, d4, tmax)
        assert not got.any()
        for k in COUNTERS:  # no ray leaves early: the closest-hit walk, step for step
            assert st[k] == cn[k], f"tmax {name}, {k}: {st[k]} vs the oracle's {cn[k]}"
    _, _, _, tr = c.trace(sp, o4, d4)
    got, st = c.occluded(sp, o4, d4, None)
    assert np.array_equal(got, OR.expected(so, o4, d4, None))
    for k in COUNTERS:
        assert st[k] <= tr[k], f"{k}: {st[k]} > rtmi_trace's {tr[k]}"
    print("NULL tmax, any-hit / closest-hit:", {k: (st[k], tr[k]) for k in COUNTERS})
    assert st["tri_tests"] < tr["tri_tests"]
    # the linear list counts the same way
    so2, sp2 = build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))
    o2, d2 = _orc().primary_rays(33, 31, _orc().canonical_viewport(33, 31), 1)
    _, _, _, cn2 = so2.trace(o2, d2)
    got, st = c.occluded(sp2, o2, d2, np.zeros(o2.shape[0], F32))
    assert not got.any()
    for k in COUNTERS:
        assert st[k] == cn2[k], k
    got, st = c.occluded(sp2, o2, d2, None)
    for k in COUNTERS:
        assert st[k] <= cn2[k], k
    assert st["tri_tests"] < cn2["tri_tests"]


def test_any_hit_kernels_agree_with_closest_hit_plus_k_occl_from_hits(primary):
    """RTMI_OCCLUDED_ANYHIT=0 (read when a scene handle is created) sends every scene through the closest-hit launch and
    k_occl_from_hits: the cross-check of the any-hit kernels inside this build"""
    R = _R()
    o4, d4, rng = OR.random_rays_canonical(n=8000)
    tmax = rng.uniform(0, 20, o4.shape[0]).astype(F32)
    tmax[::7] = np.nan
    res = {}
    old = os.environ.get("RTMI_OCCLUDED_ANYHIT")
    try:
        for mode in ("1", "0"):
            os.environ["RTMI_OCCLUDED_ANYHIT"] = mode
            sp = recipe_canonical()(ProductApi(R))  # a fresh scene: a fresh handle
            c = R.HipRayCaster(options=R.OPT_COUNTERS)
            res[mode] = [c.occluded(sp, o4, d4, tm) for tm in (tmax, None)]
    finally:
        if old is None:
            del os.environ["RTMI_OCCLUDED_ANYHIT"]
        else:
            os.environ["RTMI_OCCLUDED_ANYHIT"] = old
    for (a, sa), (b, sb) in zip(res["1"], res["0"]):
        assert np.array_equal(a, b) and a.any() and not a.all()
        assert sa["tri_tests"] < sb["tri_tests"] and sa["box_tests"] <= sb["box_tests"]  # "0" really ran the whole walk


def test_device_variant_on_torch_tensors(canonical_pair, primary):
    import torch
    so, sp = canonical_pair
    so4, sd4, dist = OR.shadow_segments(so, *primary)
    R = _R()
    c = R.HipRayCaster(seed=3)
    n = so4.shape[0]
    host, _ = c.occluded(sp, so4, sd4, dist)
    host_null, _ = c.occluded(sp, so4, sd4, None)
    vp = R.canonical_viewport(48, 32, 5, 2)
    before = np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, before, 1, False)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t_o = torch.from_numpy(so4).to("cuda:0", non_blocking=False)
        t_d = torch.from_numpy(sd4).to("cuda:0")
        t_m = torch.from_numpy(dist).to("cuda:0")
        t_o2 = t_o * 1.0  # produced on the stream: the call must wait for it
        out = torch.full((n + 128,), 0xAA, dtype=torch.uint8, device="cuda:0")
        stats = c.occluded_device(sp, n, t_o2.data_ptr(), t_d.data_ptr(), t_m.data_ptr(), out.data_ptr() + 64, stream=st.cuda_stream)
        total = out[64:64 + n].sum(dtype=torch.int64)  # queued behind the call on the same stream
        out2 = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda:0")
        c.occluded_device(sp, n, t_o2.data_ptr(), t_d.data_ptr(), None, out2.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[64:64 + n], host) and int(total) == int(host.sum())
    assert (got[:64] == 0xAA).all() and (got[64 + n:] == 0xAA).all()
    assert np.array_equal(out2.cpu().numpy(), host_null)
    assert stats["rays"] == n and stats["trace_launches"] == 1 and stats["kernel_ms"] > 0 and stats["trace_ms"] > 0
    # the caller's rays are read in place and left alone
    assert np.array_equal(t_o2.cpu().numpy().view(np.uint32), so4.view(np.uint32))
    assert np.array_equal(t_d.cpu().numpy().view(np.uint32), sd4.view(np.uint32))
    assert np.array_equal(t_m.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    # and the handle's render workspace is not disturbed: the next render is the one before, bit for bit
    after = np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, after, 1, False)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(c.occluded(sp, so4, sd4, dist)[0], host)


@pytest.mark.parametrize("tuning", [dict(refill_min0=1, refill_min=1), dict(refill_min0=16, refill_min=64), dict(xcd_aware=0),
                                    dict(xcd_aware=1), dict(xcd_aware=2), dict(oct_waves_per_cu=3), dict(oct_waves_per_cu=32),
                                    dict(batch_paths=1000, streams=2)])
def test_tuning_changes_no_byte(canonical_pair, tuning):
    so, sp = canonical_pair
    o4, d4, rng = OR.random_rays_canonical(n=5000)
    tmax = rng.uniform(0, 20, o4.shape[0]).astype(F32)
    R = _R()
    try:
        _check(R.HipRayCaster(tuning=tuning), sp, o4, d4, tmax, OR.expected(so, o4, d4, tmax), f"tuning {tuning}")
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_ragged_sizes_and_guard_bytes(canonical_pair, primary, n):
    """The byte stores touch the n answers and nothing beside them (host variant: the copy out; device variant: the kernel's
    own stores into a torch tensor with guard bytes on both sides)"""
    import torch
    from rust_raytrace_amd import _ffi
    so, sp = canonical_pair
    o4, d4 = primary
    o4, d4 = np.ascontiguousarray(o4[1500:1500 + n]), np.ascontiguousarray(d4[1500:1500 + n])  # rows that cross the teapot
    want = OR.expected(so, o4, d4, None)
    if n > 1:
        assert want.any()
    R = _R()
    c = R.HipRayCaster()
    c.upload(sp)
    buf = np.full(n + 128, 0xAA, np.uint8)
    st = _ffi.Stats()
    rc = _ffi.lib().rth_caster_occluded(sp.h, n, o4.ctypes.data_as(C.c_void_p), d4.ctypes.data_as(C.c_void_p), None,
                                        C.c_void_p(buf.ctypes.data + 64), C.byref(st))
    assert rc == 0 and st.rays == n
    assert np.array_equal(buf[64:64 + n], want) and (buf[:64] == 0xAA).all() and (buf[64 + n:] == 0xAA).all()
    t_o, t_d = torch.from_numpy(o4).to("cuda:0"), torch.from_numpy(d4).to("cuda:0")
    out = torch.full((n + 128,), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.occluded_device(sp, n, t_o.data_ptr(), t_d.data_ptr(), None, out.data_ptr() + 61)  # an odd address: plain byte stores
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[61:61 + n], want) and (got[:61] == 0xAA).all() and (got[61 + n:] == 0xAA).all()
