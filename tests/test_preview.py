"""-m gpu: the shaded preview (rtmi_render_preview / rtmi_render_preview_device, HipRayCaster.walk_rays_preview*) against its
definition, every float of every requested output bit for bit: tests/preview_ref.py restates include/rtmi.h in float32 NumPy on
the oracle's primary rays, closest hits, triangle records and RNG and on the restatements of the three layers, so no expected
value comes from the code under test (the two modes that are not bit-exact by design, RTMI_OPT_BVH and RTMI_OPT_FAST, are held
against the product's own rtmi_trace / rtmi_occluded).  The references are computed once per case and shared."""
import numpy as np
import pytest

from conftest import TEAPOT, ProductApi, assert_bits_equal, build_pair, recipe_canonical, recipe_circles_analytic
import denoise_ref as DR
import light_ref as LR
import occluded_ref as OR
import preview_ref as PR

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = ("rays", "box_tests", "tri_tests", "full_tests", "nodes", "leaves")
ALL = ("color", "albedo", "normal", "ids", "ao", "shadow", "irradiance")
FULL = None  # tile: the whole frame through the host variant
AMBIENT = (0.25, 0.25, 0.3)
A = dict(orig=OR.LIGHT, len2=0.5, rays=4, color=(1.0, 0.9, 0.8))            # the canonical box light (-3, 6, 1)
B = dict(orig=(2.0, 0.0, -3.0), len2=0.0, rays=4, color=(0.2, 0.3, 0.5))    # a point light behind the camera: nothing occludes it
FAR_BEHIND = dict(orig=(2.0, 0.0, 1.0e6), len2=0.5, rays=4)                 # behind every surface: every candidate is culled
GUARD = 64
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _freeze(x):
    if isinstance(x, dict):
        return tuple(sorted((k, _freeze(v)) for k, v in x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(v) for v in x)
    return x


def _ref(so, w, h, spp, seed, ao=None, lights=(A, B), **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), w, h, spp, seed, _freeze(ao), _freeze(lights), _freeze(kw))
    if key not in _REFS:
        orc = _orc()
        _REFS[key] = PR.preview_ref(orc, so, w, h, orc.canonical_viewport(w, h), spp, seed, AMBIENT, ao, lights, **kw)
    return _REFS[key]


def _api_lights(lights):
    """The restatement's light dicts as walk_rays_preview takes them (flags -> unbounded)"""
    out = []
    for li in lights:
        d = {k: v for k, v in li.items() if k != "flags"}
        d["unbounded"] = bool(li.get("flags", 0) & LR.UNBOUNDED)
        out.append(d)
    return out


def _render(c, sp, w, h, spp, ao=None, lights=(A, B), outputs=ALL, sample0=0, nsamples=None, tile=FULL, stream=None):
    """({name: array} of the requested outputs, stats) of one call: the host variant for the whole frame, the device variant on
    torch tensors with guard elements round every output for a tile"""
    vp = _R().canonical_viewport(w, h, 5, spp)
    kw = dict(ambient=AMBIENT, ao=ao, lights=_api_lights(lights), sample0=sample0, nsamples=nsamples)
    name_kw = lambda n: "ao_out" if n == "ao" else n
    if tile is FULL:
        r = c.walk_rays_preview(vp, sp, **kw, **{name_kw(n): (n in outputs) for n in ALL})
        return {n: getattr(r, n) for n in outputs}, r.ctx.stats
    import torch
    npix, nl = tile[1] * w, len(lights)
    size = dict(color=4 * npix, albedo=4 * npix, normal=4 * npix, ids=npix, ao=npix, shadow=nl * npix, irradiance=nl * npix)
    shape = dict(color=(tile[1], w, 4), albedo=(tile[1], w, 4), normal=(tile[1], w, 4), ids=(tile[1], w), ao=(tile[1], w),
                 shadow=(nl, tile[1], w), irradiance=(nl, tile[1], w))
    bufs = {}
    for n in outputs:
        if n == "ids":
            bufs[n] = torch.full((size[n] + 2 * GUARD,), 0x7A7A7A7A, dtype=torch.int32, device="cuda:0")
        else:
            bufs[n] = torch.full((size[n] + 2 * GUARD,), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_preview_device(vp, sp, tile=tile, stream=stream, **kw,
                                     **{name_kw(n): bufs[n][GUARD:GUARD + size[n]] for n in outputs})
    torch.cuda.synchronize()
    out = {}
    for n in outputs:
        g = bufs[n].cpu().numpy()
        guard = 0x7A7A7A7A if n == "ids" else 7.5
        assert (g[:GUARD] == guard).all() and (g[GUARD + size[n]:] == guard).all(), f"guard elements of {n}"
        x = g[GUARD:GUARD + size[n]].reshape(shape[n])
        out[n] = x.view(np.uint32) if n == "ids" else x
    return out, ctx.stats


def _compare(got, ref, outputs, what):
    for n in outputs:
        want = getattr(ref, n)
        assert got[n] is not None and want is not None, f"{what}: {n}"
        assert got[n].dtype == want.dtype and got[n].shape == want.shape, f"{what}: {n} {got[n].dtype} {got[n].shape}"
        assert_bits_equal(got[n], want, f"{what}: {n}")


def _check(c, so, sp, w, h, spp, seed, what, ao=None, lights=(A, B), outputs=None, ref=None, batches=None, **kw):
    """One call against the restatement: every requested output, stats.rays and the launch bookkeeping.  -> (reference, stats)"""
    if outputs is None:
        Ka = 4 if ao is None else (0 if ao is False else ao.get("rays", 4))
        outputs = tuple(n for n in ALL if not (n == "ao" and Ka == 0) and not (n in ("shadow", "irradiance") and not lights))
    if ref is None:
        ref_kw = {k: v for k, v in kw.items() if k in ("sample0", "nsamples", "tile") and v is not None}
        if ref_kw.get("tile") == (0, h, h, 0):  # the whole frame: the host variant's reference
            del ref_kw["tile"]
        ref = _ref(so, w, h, spp, seed, ao, lights, **ref_kw)
    got, st = _render(c, sp, w, h, spp, ao, lights, outputs, **kw)
    _compare(got, ref, outputs, what)
    assert st["rays"] == ref.rays, f"{what}: rays {st['rays']} vs {ref.npaths} + {ref.n_ao} + {ref.nlive}"
    per_batch = 2 if _has_secondary(ao, lights) else 1  # the primaries' closest-hit launch and the one shared walk
    assert st["pipeline"] == 1 and st["slow_paths"] == 0 and st["trace_launches"] >= per_batch and st["trace_launches"] % per_batch == 0
    if batches is not None:
        assert st["trace_launches"] == per_batch * batches, f"{what}: {st['trace_launches']} launches for {batches} batches"
    assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] >= 0
    assert abs(st["trace_ms"] - (st["primary_ms"] + st["bounce_ms"])) <= 1e-3 * st["trace_ms"]
    return ref, st


def _has_secondary(ao, lights):
    Ka = 4 if ao is None else (0 if ao is False else ao.get("rays", 4))
    return Ka > 0 or len(lights) > 0


def test_canonical_case_with_all_seven_outputs(canonical_pair):
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "canonical", batches=1)
    assert (ref.nhit, ref.n_ao, ref.ao_occ, ref.nculled, ref.nlive, ref.nocc) == (417, 1668, 195, [385, 0], [1283, 1668], [224, 0])
    assert st["rays"] == 6667 and st["trace_launches"] == 2


def test_layers_equal_the_single_calls_of_the_same_handle(canonical_pair):
    _, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1)
    vp = R.canonical_viewport(32, 32, 5, 2)
    r = c.walk_rays_preview(vp, sp, ambient=AMBIENT, lights=_api_lights((A, B)), albedo=True, normal=True, ids=True, ao_out=True, shadow=True,
                            irradiance=True)
    alb, nrm, ids, _ = c.walk_rays_features(vp, sp)
    assert_bits_equal(r.albedo, alb, "albedo")
    assert_bits_equal(r.normal, nrm, "normal")
    assert np.array_equal(r.ids, ids)
    ao, _ = c.walk_rays_ao(vp, sp)
    assert_bits_equal(r.ao, ao, "ao")
    for l, li in enumerate(_api_lights((A, B))):
        li = {k: v for k, v in li.items() if k != "color"}
        sh, ir, _ = c.walk_rays_light(vp, sp, **li)
        assert_bits_equal(r.shadow[l], sh, f"shadow {l}")
        assert_bits_equal(r.irradiance[l], ir, f"irradiance {l}")


def test_uneven_counts(canonical_pair):
    """Ka 3, K_A 1, K_B 5: every fold runs over its own count"""
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "Ka 3, K 1 and 5", ao=dict(rays=3), lights=(dict(A, rays=1), dict(B, rays=5)))


def test_odd_width(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 33, 32, 2, 1, "width 33")
    assert ref.nhit == 440


def test_centred_ray_frame(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 48, 48, 1, 1, "S = 1, 48 x 48, Ka = 8", ao=dict(rays=8))
    assert ref.nhit > 400 and ref.ao_occ > 0 and ref.nocc[0] > 0


def test_samples_1_to_3_of_a_frame_of_3(canonical_pair):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 3, 1, "samples [1, 3) of 3", sample0=1, nsamples=2)


def test_four_lights(canonical_pair):
    so, sp = canonical_pair
    lights = (A, B, dict(orig=(4.0, 5.0, 2.0), len2=0.25, rays=2, color=(0.5, 0.0, 0.25), flags=LR.UNBOUNDED),
              dict(orig=(-1.0, -4.0, 3.0), len2=1.0, rays=3, color=(0.0, 1.5, 0.0), bias=0.02))
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "four lights", lights=lights)
    assert all(n > 0 for n in ref.nlive) and ref.shadow.shape == (4, 32, 32)


def test_no_ao_rays_with_lights_and_no_lights_with_ao(canonical_pair):
    so, sp = canonical_pair
    a, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "ao.rays = 0", ao=False)
    assert a.n_ao == 0 and a.ao is None and (a.f == 1.0).all()
    b, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "no lights", lights=())
    assert b.shadow is None and b.rays == 2048 + 1668


def test_neither_ao_nor_lights_launches_no_walk(canonical_pair):
    """A flat preview: every sample that hit is albedo * ambient, the sky stays the sky; one launch per batch"""
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "flat", ao=False, lights=(), batches=1)
    assert st["trace_launches"] == 1 and st["rays"] == 2048 and st["bounce_ms"] == 0
    sky = (ref.tri.reshape(1024, 2) == 0).all(axis=1).reshape(32, 32)
    assert_bits_equal(ref.color[sky], np.concatenate([ref.albedo[sky][:, :3], np.zeros((int(sky.sum()), 1), F32)], axis=1), "the sky's pixels")


def test_finite_radius_bounded_and_unbounded_lights_share_the_limits(canonical_pair):
    """One tmax array holds a finite AO radius, a bounded light's distances and an unbounded light's +inf.  The light sits
    inside the scene, where surfaces beyond it shadow only its unbounded twin (the oracle: 21 against 386 occluded rays)."""
    so, sp = canonical_pair
    inside = dict(orig=(3.0, 3.0, 6.0), len2=0.5, rays=4, color=(0.2, 0.3, 0.5))
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "radius 0.5, a bounded and an unbounded light",
                    ao=dict(radius=0.5), lights=(inside, dict(inside, flags=LR.UNBOUNDED, color=(1.0, 0.9, 0.8))))
    full = _ref(so, 32, 32, 2, 1)
    assert 0 < ref.ao_occ < full.ao_occ and ref.nlive[0] == ref.nlive[1] and ref.nocc[1] > ref.nocc[0] > 0
    assert ref.light_rays[1][2] is None and np.isfinite(ref.light_rays[0][2]).all()


@pytest.mark.parametrize("outputs", [("color",), ALL[1:]] + [(n,) for n in ALL[1:]], ids=lambda o: "+".join(o))
def test_subsets_of_the_outputs_through_the_device_variant(canonical_pair, outputs):
    """Colour alone, the layers without colour, each output alone; guard elements round every buffer"""
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, f"outputs {outputs}", outputs=outputs, tile=(0, 32, 32, 0))


def test_striped_tile(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "tile {1, 12, 3, 8}", tile=(1, 12, 3, 8))
    assert ref.nhit == 173 and ref.nlive[0] == 520


def test_a_tile_of_sky_rows(canonical_pair):
    """Zero hits: the walk is launched with a count of 0; the colour is the sky's"""
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "sky rows", tile=(24, 8, 8, 0), batches=1)
    assert ref.nhit == 0 and st["rays"] == 512 and st["trace_launches"] == 2
    assert (ref.color[..., :3] == PR.FR.SKY).all() and (ref.ao == 1.0).all() and (ref.shadow == 1.0).all()


def test_a_light_behind_every_surface_without_ao(canonical_pair):
    """Hits, but every candidate is culled and there are no AO rays: a walk of 0 rays, the ambient term alone on the hits"""
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 2, 1, "light far behind", ao=False, lights=(FAR_BEHIND,), tile=(6, 10, 10, 0))
    assert ref.nhit == 233 and ref.nlive == [0] and st["rays"] == ref.npaths == 640 and st["trace_launches"] == 2
    hit = (ref.tri.reshape(320, 2) != 0).all(axis=1).reshape(10, 32)
    assert hit.any() and (ref.f == 1.0).all() and (ref.g == 0.0).all() and (ref.shadow[0][hit] == 0.0).all() and (ref.irradiance == 0.0).all()
    flat = _ref(so, 32, 32, 2, 1, False, (), tile=(6, 10, 10, 0))  # neither AO nor lights: the same image
    assert_bits_equal(ref.color, flat.color, "the ambient term alone")


def test_second_seed_and_second_biases(canonical_pair):
    so, sp = canonical_pair
    a, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 7, "seed 7")
    b, _ = _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 2, 7, "seed 7, second biases", ao=dict(bias=0.01),
                  lights=(dict(A, bias=0.05), dict(B, bias=0.0005)))
    one = _ref(so, 32, 32, 2, 1)
    # a bias moves a ray's origin (n . dir is taken from the unsmudged point): other rays, and on this view the same answers
    assert not np.array_equal(a.color, one.color) and not np.array_equal(a.ao_rays[0], b.ao_rays[0])
    assert all(not np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a.light_rays, b.light_rays))


@pytest.fixture(scope="module")
def linear_pair():
    return build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))


def test_linear_list_scene(linear_pair):
    so, sp = linear_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 2, 1, "linear list")
    assert ref.nhit == 97 and ref.ao_occ > 0 and ref.nocc[0] > 0


def test_option_generic_against_the_oracle(canonical_pair):
    so, sp = canonical_pair
    R = _R()
    _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 2, 1, "RTMI_OPT_GENERIC")


@pytest.mark.parametrize("opt", ["OPT_BVH", "OPT_FAST"])
def test_options_bvh_and_fast_against_their_own_trace_and_occluded(canonical_pair, opt):
    so, sp = canonical_pair
    R, orc = _R(), _orc()
    c = R.HipRayCaster(seed=1, options=getattr(R, opt))
    ref = PR.preview_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 2, 1, AMBIENT, None, (A, B),
                         trace=lambda o, d: c.trace(sp, o, d)[:3], occluded=lambda o, d, tm: c.occluded(sp, o, d, tm)[0])
    assert ref.nhit > 300 and ref.ao_occ > 0 and ref.nocc[0] > 0
    _check(c, so, sp, 32, 32, 2, 1, opt, ref=ref)


def test_analytic_spheres_are_unsupported():
    R = _R()
    sp = recipe_circles_analytic()(ProductApi(R))
    with pytest.raises(RuntimeError, match="analytic spheres"):
        R.HipRayCaster().walk_rays_preview(R.canonical_viewport(16, 16, 5, 1), sp)


def test_counters_report_the_work_done(canonical_pair):
    """The any-hit walk leaves a ray's walk early only to answer 1.  With an AO radius of 0 and light B alone the oracle finds
    no secondary ray occluded, so no walk ends early and all six counters are the oracle's for the primaries plus its
    closest-hit traces of the AO rays and of the live rays.  With the canonical case, where rays are occluded, each is at most
    that."""
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1, options=R.OPT_COUNTERS)
    ref, st0 = _check(c, so, sp, 32, 32, 2, 1, "counters, nothing occluded", ao=dict(radius=0.0), lights=(B,))
    assert ref.ao_occ == 0 and ref.nocc == [0] and ref.nlive == [1668] and ref.n_ao == 1668
    for k in COUNTERS:
        want = ref.cn_primary[k] + ref.cn_ao[k] + ref.cn_lights[0][k]
        assert st0[k] == want, f"{k}: {st0[k]} vs the oracle's {want}"
    ref, st = _check(c, so, sp, 32, 32, 2, 1, "counters, canonical")
    assert ref.ao_occ > 0 and ref.nocc[0] > 0
    for k in COUNTERS:
        assert st[k] <= ref.cn_primary[k] + ref.cn_ao[k] + sum(cn[k] for cn in ref.cn_lights), k
    assert st["rays"] == 6667


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
        # 24 queue entries per pixel (S = 2, Ka + K_A + K_B = 12): batch_paths 2500 on one stream = 104 pixels a batch, 10 batches
        batches = 10 if tuning.get("batch_paths") == 2500 else None
        _, st = _check(R.HipRayCaster(seed=1, tuning=tuning), so, sp, 32, 32, 2, 1, f"tuning {tuning}", batches=batches)
        if batches:
            assert st["trace_launches"] == 20 and st["streams"] == 1
        if tuning.get("streams") == 3:
            assert st["streams"] == 3
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


def test_generic_fallback_in_batches(canonical_pair):
    """The closest-hit fallback with its device-side count (its hit records sized for the whole queue), over several batches
    and streams"""
    so, sp = canonical_pair
    R = _R()
    try:
        c = R.HipRayCaster(seed=1, options=R.OPT_GENERIC, tuning=dict(batch_paths=3000, streams=2, subtile_min_paths=1))
        _, st = _check(c, so, sp, 32, 32, 2, 1, "generic, batches")
        assert st["trace_launches"] >= 6
    finally:
        R.HipRayCaster().upload(sp)


def test_device_variant_on_a_torch_stream(canonical_pair):
    import torch
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1)
    small, large = _ref(so, 32, 32, 2, 1), _ref(so, 48, 48, 1, 1, dict(rays=8))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got_small, stats = _render(c, sp, 32, 32, 2, tile=(0, 32, 32, 0), stream=st)
        # a second, larger call on the same handle: the queues grow (2304 paths x 16 entries against 2048 x 12)
        got_large, _ = _render(c, sp, 48, 48, 1, ao=dict(rays=8), tile=(0, 48, 48, 0), stream=st)
        # and the small one again, after the growth, on the raw stream pointer
        got_again, _ = _render(c, sp, 32, 32, 2, tile=(0, 32, 32, 0), stream=st.cuda_stream)
    st.synchronize()
    _compare(got_small, small, ALL, "device variant, 32 x 32")
    _compare(got_large, large, ALL, "device variant, 48 x 48")
    _compare(got_again, small, ALL, "device variant, 32 x 32 again")
    assert stats["rays"] == small.rays
    # the handle's render workspace is left usable: the next render equals a fresh handle's, bit for bit
    vp = R.canonical_viewport(48, 32, 5, 2)
    after = np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, after, 1, False)
    fresh = np.zeros((32, 48, 4), F32)
    R.HipRayCaster(seed=1).walk_rays(vp, recipe_canonical()(ProductApi(R)), fresh, 1, False)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32))


def test_composition_with_the_denoiser(canonical_pair):
    """color, albedo and normal of ONE preview call go straight into denoise_device: the result is the restatement of the
    filter on the restatement's three images"""
    import torch
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1)
    ref = _ref(so, 32, 32, 2, 1)
    img = [torch.zeros((32 * 32 * 4,), dtype=torch.float32, device="cuda:0") for _ in range(4)]
    c.walk_rays_preview_device(R.canonical_viewport(32, 32, 5, 2), sp, ambient=AMBIENT, lights=_api_lights((A, B)), color=img[0],
                               albedo=img[1], normal=img[2])
    c.denoise_device(32, 32, img[0].data_ptr(), img[1].data_ptr(), img[2].data_ptr(), img[3].data_ptr(), scene=sp)
    torch.cuda.synchronize()
    want = DR.denoise_ref(ref.color, ref.albedo, ref.normal)
    assert_bits_equal(img[3].cpu().numpy().reshape(32, 32, 4), want, "denoised preview")
