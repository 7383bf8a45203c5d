"""-m gpu: the ambient-occlusion buffer (rtmi_render_ao / rtmi_render_ao_device, HipRayCaster.walk_rays_ao*) against its
definition, every float bit for bit: tests/ao_ref.py restates include/rtmi.h in float32 NumPy on the oracle's primary rays,
closest hits, triangle records and RNG, so no expected value comes from the code under test (the two modes that are not
bit-exact by design, RTMI_OPT_BVH and RTMI_OPT_FAST, are held against the product's own rtmi_trace / rtmi_occluded)."""
import numpy as np
import pytest

from conftest import TEAPOT, ProductApi, assert_bits_equal, build_pair, recipe_canonical, recipe_circles_analytic
import ao_ref as AR

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
FULL = None  # tile: the whole frame through the host variant


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _render(c, sp, w, h, spp, K, radius=INF, bias=None, sample0=0, nsamples=None, tile=FULL):
    """(ao (rows, w), stats) of one call: the host variant for the whole frame, the device variant on a torch tensor for a tile"""
    vp = _R().canonical_viewport(w, h, 5, spp)
    if tile is FULL:
        img, ctx = c.walk_rays_ao(vp, sp, rays=K, radius=radius, bias=bias, sample0=sample0, nsamples=nsamples)
        return img, ctx.stats
    import torch
    out = torch.full((tile[1] * w,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_ao_device(vp, sp, out, tile=tile, rays=K, radius=radius, bias=bias, sample0=sample0, nsamples=nsamples)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(tile[1], w), ctx.stats


def _check(c, so, sp, w, h, spp, K, seed, what, **kw):
    """One call against the restatement: the image, stats.rays and the launch bookkeeping.  -> (reference, stats)"""
    orc = _orc()
    ref_kw = {k: v for k, v in kw.items() if k != "bias"}
    ref = AR.ao_ref(orc, so, w, h, orc.canonical_viewport(w, h), spp, seed, K, bias=kw.get("bias") or 0.001, **ref_kw)
    img, st = _render(c, sp, w, h, spp, K, **kw)
    assert img.dtype == np.float32
    assert_bits_equal(img, ref.ao, what)
    assert st["rays"] == ref.npaths + ref.nhit * K, f"{what}: rays {st['rays']} vs {ref.npaths} + {ref.nhit} * {K}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0 and st["trace_launches"] >= 2 and st["trace_launches"] % 2 == 0
    assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] > 0
    assert abs(st["trace_ms"] - (st["primary_ms"] + st["bounce_ms"])) <= 1e-3 * st["trace_ms"]
    return ref, st


@pytest.mark.parametrize("radius", [INF, 1.0, 0.0])
def test_canonical_octree_every_radius(canonical_pair, radius):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, f"radius {radius}", radius=radius)
    assert ref.nhit == 417
    if radius == 0.0:
        assert (ref.ao == 1.0).all()
    else:
        assert ref.occ.any() and (ref.ao < 1.0).any()


def test_one_sample_of_a_jittered_frame(canonical_pair):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "sample 1 of 2", sample0=1, nsamples=1)


def test_centred_ray_frame(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 48, 48, 1, 8, 1, "S = 1, 48 x 48, K = 8")
    assert ref.nhit > 400 and ref.occ.any()


@pytest.mark.parametrize("K", [1, 3, 64])
def test_ray_counts(canonical_pair, K):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, K, 1, f"K = {K}")


def test_striped_tile(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "tile {1, 12, 3, 8}", tile=(1, 12, 3, 8))
    assert ref.nhit > 100 and (ref.ao < 1.0).any()


def test_odd_width(canonical_pair):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 33, 32, 2, 4, 1, "width 33")


def test_second_seed_and_bias(canonical_pair):
    so, sp = canonical_pair
    a, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 4, 7, "seed 7")
    b, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 4, 7, "seed 7, bias 0.05", bias=0.05)
    one = AR.ao_ref(_orc(), so, 32, 32, _orc().canonical_viewport(32, 32), 2, 1, 4)
    assert not np.array_equal(a.ao, one.ao) and not np.array_equal(a.o4, b.o4)


def test_composition_with_rtmi_occluded(canonical_pair):
    """The restatement's rays through rtmi_occluded, reduced on the host, are the image the one call renders"""
    so, sp = canonical_pair
    orc = _orc()
    c = _R().HipRayCaster(seed=1)
    for radius in (INF, 1.0):
        ref = AR.ao_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 2, 1, 4, radius=radius,
                        occluded=lambda o, d, tm: c.occluded(sp, o, d, None if radius == INF else tm)[0])
        img, _ = _render(c, sp, 32, 32, 2, 4, radius=radius)
        assert_bits_equal(img, ref.ao, f"composition, radius {radius}")


def test_linear_list_scene():
    so, sp = build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))
    for radius in (INF, 1.0):
        ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 2, 4, 1, f"linear list, radius {radius}", radius=radius)
    assert ref.nhit > 50


def test_option_generic_against_the_oracle(canonical_pair):
    so, sp = canonical_pair
    R = _R()
    for radius in (INF, 1.0):
        _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 2, 4, 1, f"RTMI_OPT_GENERIC, radius {radius}", radius=radius)


@pytest.mark.parametrize("opt", ["OPT_BVH", "OPT_FAST"])
def test_options_bvh_and_fast_against_their_own_trace_and_occluded(canonical_pair, opt):
    so, sp = canonical_pair
    R, orc = _R(), _orc()
    c = R.HipRayCaster(seed=1, options=getattr(R, opt))
    for radius in (INF, 1.0):
        ref = AR.ao_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 2, 1, 4, radius=radius,
                        trace=lambda o, d: c.trace(sp, o, d)[:3], occluded=lambda o, d, tm: c.occluded(sp, o, d, tm)[0])
        assert ref.nhit > 300 and ref.occ.any()
        img, st = _render(c, sp, 32, 32, 2, 4, radius=radius)
        assert_bits_equal(img, ref.ao, f"{opt}, radius {radius}")
        assert st["rays"] == ref.npaths + ref.nhit * 4


def test_analytic_spheres_are_unsupported():
    R = _R()
    sp = recipe_circles_analytic()(ProductApi(R))
    with pytest.raises(RuntimeError, match="analytic spheres"):
        R.HipRayCaster().walk_rays_ao(R.canonical_viewport(16, 16, 5, 1), sp)


def test_counters_report_the_work_done(canonical_pair):
    """Radius 0: no AO ray leaves its walk early, so all six counters are the oracle's for the primaries plus the compacted AO
    rays (walking the samples that missed would add their rays' work).  Radius +inf: never more, and fewer plane tests."""
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS)
    ref, st0 = _check(c, so, sp, 32, 32, 2, 4, 1, "counters, radius 0", radius=0.0)
    want = {k: ref.cn_primary[k] + ref.cn_ao[k] for k in COUNTERS}
    for k in COUNTERS:
        assert st0[k] == want[k], f"radius 0, {k}: {st0[k]} vs the oracle's {ref.cn_primary[k]} + {ref.cn_ao[k]}"
    _, st = _check(c, so, sp, 32, 32, 2, 4, 1, "counters, radius inf")
    print("radius inf / radius 0:", {k: (st[k], st0[k]) for k in COUNTERS})
    for k in COUNTERS:
        assert st[k] <= want[k], k
    assert st["tri_tests"] < want["tri_tests"]
    # the linear list counts the same way
    so2, sp2 = build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))
    ref2, st2 = _check(c, so2, sp2, 16, 16, 2, 4, 1, "linear counters, radius 0", radius=0.0)
    for k in COUNTERS:
        assert st2[k] == ref2.cn_primary[k] + ref2.cn_ao[k], k


TUNINGS = [dict(batch_paths=2500, streams=1), dict(streams=1, subtile_min_paths=1), dict(streams=3, subtile_min_paths=1),
           dict(batch_paths=3000, streams=3, subtile_min_paths=1),
           # the eight of tests/test_occluded.py
           dict(refill_min0=1, refill_min=1), dict(refill_min0=16, refill_min=64), dict(xcd_aware=0), dict(xcd_aware=1),
           dict(xcd_aware=2), dict(oct_waves_per_cu=3), dict(oct_waves_per_cu=32), dict(batch_paths=1000, streams=2)]


@pytest.mark.parametrize("tuning", TUNINGS, ids=lambda t: ",".join(f"{k}={v}" for k, v in t.items()))
def test_tuning_changes_no_bit(canonical_pair, tuning):
    so, sp = canonical_pair
    R = _R()
    try:
        _, st = _check(R.HipRayCaster(seed=1, tuning=tuning), so, sp, 32, 32, 2, 4, 1, f"tuning {tuning}", radius=1.0)
        if tuning.get("batch_paths") == 2500:  # 8 AO rays per pixel at most: 312 pixels per batch, four batches of two walks
            assert st["trace_launches"] >= 6 and st["streams"] == 1
        if tuning.get("streams") == 3:
            assert st["streams"] == 3
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


def test_generic_fallback_in_batches(canonical_pair):
    """The closest-hit fallback with its device-side count, over several batches and streams"""
    so, sp = canonical_pair
    R = _R()
    try:
        c = R.HipRayCaster(seed=1, options=R.OPT_GENERIC, tuning=dict(batch_paths=3000, streams=2, subtile_min_paths=1))
        _, st = _check(c, so, sp, 32, 32, 2, 4, 1, "generic, batches")
        assert st["trace_launches"] >= 6
    finally:
        R.HipRayCaster().upload(sp)


def test_device_variant_on_a_torch_stream(canonical_pair):
    import torch
    so, sp = canonical_pair
    R, orc = _R(), _orc()
    c = R.HipRayCaster(seed=1)
    small = AR.ao_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 2, 1, 4, radius=1.0)
    large = AR.ao_ref(orc, so, 48, 48, orc.canonical_viewport(48, 48), 1, 1, 8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        buf = torch.full((32 * 32 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
        ctx = c.walk_rays_ao_device(R.canonical_viewport(32, 32, 5, 2), sp, buf[64:64 + 1024], rays=4, radius=1.0, stream=st)
        total = buf[64:64 + 1024].sum(dtype=torch.float64)  # queued behind the call on the same stream
        # a second, larger call on the same handle: the AO queue grows (2304 paths x 8 rays against 2048 x 4)
        buf2 = torch.full((48 * 48 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
        c.walk_rays_ao_device(R.canonical_viewport(48, 48, 5, 1), sp, buf2[64:64 + 2304], rays=8, stream=st)
        # and the small one again, after the growth
        buf3 = torch.full((1024,), 7.5, dtype=torch.float32, device="cuda:0")
        c.walk_rays_ao_device(R.canonical_viewport(32, 32, 5, 2), sp, buf3, rays=4, radius=1.0, stream=st.cuda_stream)
    st.synchronize()
    got, got2 = buf.cpu().numpy(), buf2.cpu().numpy()
    assert_bits_equal(got[64:64 + 1024].reshape(32, 32), small.ao, "device variant, 32 x 32")
    assert (got[:64] == 7.5).all() and (got[64 + 1024:] == 7.5).all()
    assert float(total) == float(small.ao.astype(np.float64).sum())
    assert_bits_equal(got2[64:64 + 2304].reshape(48, 48), large.ao, "device variant, 48 x 48")
    assert (got2[:64] == 7.5).all() and (got2[64 + 2304:] == 7.5).all()
    assert_bits_equal(buf3.cpu().numpy().reshape(32, 32), small.ao, "device variant, 32 x 32 again")
    assert ctx.stats["rays"] == small.npaths + small.nhit * 4 and ctx.total_rays == ctx.stats["rays"]
    # the handle's render workspace is left usable: the next render equals a fresh handle's, bit for bit
    vp = R.canonical_viewport(48, 32, 5, 2)
    after = np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, after, 1, False)
    fresh = np.zeros((32, 48, 4), F32)
    R.HipRayCaster(seed=1).walk_rays(vp, recipe_canonical()(ProductApi(R)), fresh, 1, False)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32))
