"""-m gpu: the direct-light buffer (rtmi_render_light / rtmi_render_light_device, HipRayCaster.walk_rays_light*) against its
definition, every float of both planes bit for bit: tests/light_ref.py restates include/rtmi.h in float32 NumPy on the oracle's
primary rays, closest hits, triangle records and RNG, so no expected value comes from the code under test (the two modes that
are not bit-exact by design, RTMI_OPT_BVH and RTMI_OPT_FAST, are held against the product's own rtmi_trace / rtmi_occluded).
The references are computed once per case and shared."""
import numpy as np
import pytest

from conftest import TEAPOT, ProductApi, assert_bits_equal, build_pair, recipe_canonical, recipe_circles_analytic
import light_ref as LR
import occluded_ref as OR

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
FULL = None  # tile: the whole frame through the host variant
LIGHT = OR.LIGHT  # (-3, 6, 1)
CAMERA = (2.0, 0.0, 0.0)       # a point light at the camera: every candidate is live
BEHIND_CAMERA = (2.0, 0.0, -3.0)  # ... and behind it on its axis: live, and the oracle finds none of them occluded
FAR_BEHIND = (2.0, 0.0, 1.0e6)  # far behind the scene on the camera's axis
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _ref(so, w, h, spp, seed, K, orig=LIGHT, len2=0.5, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), w, h, spp, seed, K, tuple(orig), len2, tuple(sorted(kw.items())))
    if key not in _REFS:
        orc = _orc()
        _REFS[key] = LR.light_ref(orc, so, w, h, orc.canonical_viewport(w, h), spp, seed, K, orig, len2, **kw)
    return _REFS[key]


def _render(c, sp, w, h, spp, K, orig=LIGHT, len2=0.5, bias=None, flags=0, sample0=0, nsamples=None, tile=FULL, planes=(True, True)):
    """(shadow, irradiance (rows, w) or None, stats) of one call: the host variant for the whole frame, the device variant on
    torch tensors with guard floats for a tile"""
    vp = _R().canonical_viewport(w, h, 5, spp)
    lk = dict(orig=orig, len2=len2, rays=K, unbounded=bool(flags & LR.UNBOUNDED), bias=bias, sample0=sample0, nsamples=nsamples)
    if tile is FULL:
        sh, ir, ctx = c.walk_rays_light(vp, sp, shadow=planes[0], irradiance=planes[1], **lk)
        return sh, ir, ctx.stats
    import torch
    n = tile[1] * w
    bufs = [torch.full((n + 128,), 7.5, dtype=torch.float32, device="cuda:0") if p else None for p in planes]
    torch.cuda.synchronize()
    ctx = c.walk_rays_light_device(vp, sp, *[b[64:64 + n] if b is not None else None for b in bufs], tile=tile, **lk)
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        g = b.cpu().numpy()
        assert (g[:64] == 7.5).all() and (g[64 + n:] == 7.5).all(), "guard floats"
        out.append(g[64:64 + n].reshape(tile[1], w))
    return out[0], out[1], ctx.stats


def _check(c, so, sp, w, h, spp, K, seed, what, planes=(True, True), ref=None, **kw):
    """One call against the restatement: both planes, stats.rays and the launch bookkeeping.  -> (reference, stats)"""
    if ref is None:
        ref_kw = {k: v for k, v in kw.items() if k != "bias" or v is not None}
        ref = _ref(so, w, h, spp, seed, K, **ref_kw)
    sh, ir, st = _render(c, sp, w, h, spp, K, planes=planes, **kw)
    for name, got, want in (("shadow", sh, ref.shadow), ("irradiance", ir, ref.irradiance)):
        if got is not None:
            assert got.dtype == np.float32
            assert_bits_equal(got, want, f"{what}: {name}")
    assert (sh is not None) == bool(planes[0]) and (ir is not None) == bool(planes[1])
    assert st["rays"] == ref.npaths + ref.nlive, f"{what}: rays {st['rays']} vs {ref.npaths} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0 and st["trace_launches"] >= 2 and st["trace_launches"] % 2 == 0
    assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] >= 0
    assert abs(st["trace_ms"] - (st["primary_ms"] + st["bounce_ms"])) <= 1e-3 * st["trace_ms"]
    return ref, st


def test_canonical_case(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "canonical")
    assert (ref.nhit, ref.nculled, ref.nlive, int(ref.occ.sum())) == (417, 385, 1283, 224)


def test_unbounded_light_and_point_light(canonical_pair):
    so, sp = canonical_pair
    u, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "unbounded", flags=LR.UNBOUNDED)
    assert u.tmax is None and u.occ.any()
    p, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "len2 = 0", len2=0.0)
    assert p.nculled > 0 and p.occ.any() and (p.occ == 0).any()


@pytest.mark.parametrize("planes", [(True, False), (False, True)], ids=["shadow", "irradiance"])
def test_each_plane_alone(canonical_pair, planes):
    """The other pointer NULL; the device variant, with guard floats round the plane"""
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, f"planes {planes}", planes=planes, tile=(0, 32, 32, 0))
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, f"planes {planes}, host variant", planes=planes)


def test_one_sample_of_a_jittered_frame(canonical_pair):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "sample 1 of 2", sample0=1, nsamples=1)


def test_centred_ray_frame(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 48, 48, 1, 8, 1, "S = 1, 48 x 48, K = 8")
    assert ref.nhit > 400 and ref.occ.any() and ref.nculled > 0


@pytest.mark.parametrize("K", [1, 3, 64])
def test_ray_counts(canonical_pair, K):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, K, 1, f"K = {K}")


def test_striped_tile(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "tile {1, 12, 3, 8}", tile=(1, 12, 3, 8))
    assert ref.nhit == 173 and ref.nlive == 520 and ref.occ.any()  # paths and candidates per block: no multiple of 64


def test_odd_width(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 33, 32, 2, 4, 1, "width 33")
    assert ref.nhit == 440 and ref.nlive == 1354


def test_a_tile_of_sky_rows(canonical_pair):
    """Zero hits: no candidate, the walk is launched with a count of 0, shadow 1 and irradiance 0 everywhere"""
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "sky rows", tile=(24, 8, 8, 0))
    assert ref.nhit == 0 and st["rays"] == 512
    assert (ref.shadow == 1.0).all() and (ref.irradiance == 0.0).all()


def test_a_light_behind_every_surface(canonical_pair):
    """Hits, but every candidate is culled: zero live rays, RTMI_OK, shadow 0 on the pixels that hit and 1 on the sky"""
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 4, 1, "light far behind", orig=FAR_BEHIND, tile=(6, 10, 10, 0))
    assert ref.nhit == 233 and ref.nlive == 0 and st["rays"] == ref.npaths == 640
    tri = ref.tri.reshape(320, 2)
    hit, sky = (tri != 0).all(axis=1).reshape(10, 32), (tri == 0).all(axis=1).reshape(10, 32)
    assert hit.any() and (ref.shadow[hit] == 0.0).all() and (ref.shadow[sky] == 1.0).all() and (ref.irradiance == 0.0).all()


def test_second_seed_and_bias(canonical_pair):
    so, sp = canonical_pair
    a, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 4, 7, "seed 7")
    b, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 4, 7, "seed 7, bias 0.05", bias=0.05)
    one = _ref(so, 32, 32, 2, 1, 4)
    assert not np.array_equal(a.irradiance, one.irradiance) and a.nlive == b.nlive and not np.array_equal(a.o4, b.o4)


def test_composition_with_rtmi_occluded(canonical_pair):
    """The restatement's live rays through rtmi_occluded give the restatement's bytes"""
    so, sp = canonical_pair
    c = _R().HipRayCaster(seed=1)
    for flags in (0, LR.UNBOUNDED):
        ref = _ref(so, 32, 32, 2, 1, 4, flags=flags) if flags else _ref(so, 32, 32, 2, 1, 4)
        occ = c.occluded(sp, ref.o4, ref.d4, ref.tmax)[0]
        assert np.array_equal(np.asarray(occ, np.uint8), ref.occ), f"flags {flags}"


@pytest.fixture(scope="module")
def linear_pair():
    return build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))


def test_linear_list_scene(linear_pair):
    so, sp = linear_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 2, 4, 1, "linear list", len2=0.0)
    assert ref.nhit == 97 and ref.nculled > 0 and ref.occ.any() and (ref.occ == 0).any()
    _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 2, 4, 1, "linear list, unbounded", len2=0.0, flags=LR.UNBOUNDED)


def test_option_generic_against_the_oracle(canonical_pair):
    so, sp = canonical_pair
    R = _R()
    _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 2, 4, 1, "RTMI_OPT_GENERIC")
    _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 2, 4, 1, "RTMI_OPT_GENERIC, unbounded", flags=LR.UNBOUNDED)


@pytest.mark.parametrize("opt", ["OPT_BVH", "OPT_FAST"])
def test_options_bvh_and_fast_against_their_own_trace_and_occluded(canonical_pair, opt):
    so, sp = canonical_pair
    R, orc = _R(), _orc()
    c = R.HipRayCaster(seed=1, options=getattr(R, opt))
    ref = LR.light_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 2, 1, 4, LIGHT, 0.5,
                       trace=lambda o, d: c.trace(sp, o, d)[:3], occluded=lambda o, d, tm: c.occluded(sp, o, d, tm)[0])
    assert ref.nhit > 300 and ref.occ.any() and ref.nculled > 0
    _check(c, so, sp, 32, 32, 2, 4, 1, opt, ref=ref)


def test_analytic_spheres_are_unsupported():
    R = _R()
    sp = recipe_circles_analytic()(ProductApi(R))
    with pytest.raises(RuntimeError, match="analytic spheres"):
        R.HipRayCaster().walk_rays_light(R.canonical_viewport(16, 16, 5, 1), sp, orig=LIGHT)


def test_counters_report_the_work_done(canonical_pair, linear_pair):
    """The any-hit walk leaves a ray's walk early only to answer 1.  With a point light behind the camera every candidate is
    live and the oracle finds none of them occluded, so no walk ends early and all six counters are the oracle's for the
    primaries plus its closest-hit trace of the live rays (walking culled candidates or the rays of missed samples would add
    their work; `rays` shows them too).  With the canonical light, where rays are occluded, each counter is at most that."""
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS)
    ref, st0 = _check(c, so, sp, 32, 32, 2, 4, 1, "counters, nothing occluded", orig=BEHIND_CAMERA, len2=0.0)
    assert ref.nlive == 1668 and not ref.occ.any()
    for k in COUNTERS:
        assert st0[k] == ref.cn_primary[k] + ref.cn_light[k], f"{k}: {st0[k]} vs the oracle's {ref.cn_primary[k]} + {ref.cn_light[k]}"
    ref, st = _check(c, so, sp, 32, 32, 2, 4, 1, "counters, canonical light")
    assert ref.occ.any() and ref.nculled > 0
    print("canonical light:", {k: (st[k], ref.cn_primary[k] + ref.cn_light[k]) for k in COUNTERS})
    for k in COUNTERS:
        assert st[k] <= ref.cn_primary[k] + ref.cn_light[k], k
    assert st["rays"] == ref.cn_primary["rays"] + ref.cn_light["rays"] == 2048 + 1283
    # the linear list counts the same way
    so2, sp2 = linear_pair
    ref2, st2 = _check(c, so2, sp2, 16, 16, 2, 4, 1, "linear counters, nothing occluded", orig=CAMERA, len2=0.0)
    assert ref2.nlive == 384 and ref2.nculled == 4 and not ref2.occ.any()
    for k in COUNTERS:
        assert st2[k] == ref2.cn_primary[k] + ref2.cn_light[k], k
    ref3, st3 = _check(c, so2, sp2, 16, 16, 2, 4, 1, "linear counters, canonical light", len2=0.0)
    for k in COUNTERS:
        assert st3[k] <= ref3.cn_primary[k] + ref3.cn_light[k], k


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
        _, st = _check(R.HipRayCaster(seed=1, tuning=tuning), so, sp, 32, 32, 2, 4, 1, f"tuning {tuning}")
        if tuning.get("batch_paths") == 2500:  # 8 candidates per pixel: 312 pixels per batch, four batches of two walks
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
    R = _R()
    c = R.HipRayCaster(seed=1)
    small, large = _ref(so, 32, 32, 2, 1, 4), _ref(so, 48, 48, 1, 1, 8)
    lk = dict(orig=LIGHT, len2=0.5)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        buf = torch.full((2 * 1024 + 192,), 7.5, dtype=torch.float32, device="cuda:0")
        sh, ir = buf[64:64 + 1024], buf[128 + 1024:128 + 2048]
        ctx = c.walk_rays_light_device(R.canonical_viewport(32, 32, 5, 2), sp, sh, ir, rays=4, stream=st, **lk)
        total = sh.sum(dtype=torch.float64)  # queued behind the call on the same stream (eighths: exact in any order)
        # a second, larger call on the same handle: the light queue grows (2304 paths x 8 candidates against 2048 x 4)
        buf2 = torch.full((2 * 2304 + 192,), 7.5, dtype=torch.float32, device="cuda:0")
        c.walk_rays_light_device(R.canonical_viewport(48, 48, 5, 1), sp, buf2[64:64 + 2304], buf2[128 + 2304:128 + 4608], rays=8, stream=st, **lk)
        # and the small one again, after the growth
        buf3 = torch.full((2048,), 7.5, dtype=torch.float32, device="cuda:0")
        c.walk_rays_light_device(R.canonical_viewport(32, 32, 5, 2), sp, buf3[:1024], buf3[1024:], rays=4, stream=st.cuda_stream, **lk)
    st.synchronize()
    got, got2, got3 = buf.cpu().numpy(), buf2.cpu().numpy(), buf3.cpu().numpy()
    assert_bits_equal(got[64:64 + 1024].reshape(32, 32), small.shadow, "device variant, 32 x 32: shadow")
    assert_bits_equal(got[128 + 1024:128 + 2048].reshape(32, 32), small.irradiance, "device variant, 32 x 32: irradiance")
    assert (got[:64] == 7.5).all() and (got[64 + 1024:128 + 1024] == 7.5).all() and (got[128 + 2048:] == 7.5).all()
    assert float(total) == float(small.shadow.astype(np.float64).sum())
    assert_bits_equal(got2[64:64 + 2304].reshape(48, 48), large.shadow, "device variant, 48 x 48: shadow")
    assert_bits_equal(got2[128 + 2304:128 + 4608].reshape(48, 48), large.irradiance, "device variant, 48 x 48: irradiance")
    assert (got2[:64] == 7.5).all() and (got2[64 + 2304:128 + 2304] == 7.5).all() and (got2[128 + 4608:] == 7.5).all()
    assert_bits_equal(got3[:1024].reshape(32, 32), small.shadow, "device variant, 32 x 32 again: shadow")
    assert_bits_equal(got3[1024:].reshape(32, 32), small.irradiance, "device variant, 32 x 32 again: irradiance")
    assert ctx.stats["rays"] == small.npaths + small.nlive and ctx.total_rays == ctx.stats["rays"]
    # the handle's render workspace is left usable: the next render equals a fresh handle's, bit for bit
    vp = R.canonical_viewport(48, 32, 5, 2)
    after = np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, after, 1, False)
    fresh = np.zeros((32, 48, 4), F32)
    R.HipRayCaster(seed=1).walk_rays(vp, recipe_canonical()(ProductApi(R)), fresh, 1, False)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32))
