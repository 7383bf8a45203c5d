"""-m gpu: the a-trous denoiser (rtmi_denoise / rtmi_denoise_device / rtmi_render_denoised; HipRayCaster.denoise,
denoise_device, walk_rays_denoised).  Every float of every result is compared with assert_bits_equal against the NumPy
restatement of tests/denoise_ref.py applied to the same three input images; the expected values never come from the filter
under test."""
import numpy as np
import pytest

from conftest import ProductApi, assert_bits_equal, recipe_axis_box, recipe_canonical
import denoise_ref as DR

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def R():
    from rust_raytrace_amd import raytrace as R
    return R


@pytest.fixture(scope="module")
def scene(R):
    return recipe_canonical()(ProductApi(R))


@pytest.fixture(scope="module")
def caster(R, scene):
    c = R.HipRayCaster(seed=1)
    c.upload(scene)
    return c


def _frame(R, c, sp, w, h, spp, vp12=None, depth=5):
    """(color, albedo, normal) of one view, each (h, w, 4) float32: walk_rays and walk_rays_features of the same rays"""
    vp = R.canonical_viewport(w, h, depth, spp) if vp12 is None else R.Viewport(w, h, vp12, depth, spp)
    col = np.zeros((h, w, 4), np.float32)
    c.walk_rays(vp, sp, col)
    alb, nrm, _, _ = c.walk_rays_features(vp, sp, ids=False)
    return col, alb, nrm, vp


def _synthetic(h, w, seed, poison=True):
    """Random colour and guides: coverage in {0, 0.5, 1}, a few flat regions so that every term passes somewhere, and NaN /
    +-inf injected into every buffer."""
    rng = np.random.default_rng(seed)
    col = rng.random((h, w, 4), dtype=np.float32) * np.float32(0.5)
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., 0:3] = np.float32(0.5) + rng.random((h, w, 3), dtype=np.float32) * np.float32(0.25)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((yy // 9) + (xx // 13)) % 3
    alb[..., 3] = region.astype(np.float32) * np.float32(0.5)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., 0:3] = rng.standard_normal((h, w, 3)).astype(np.float32) * np.float32(0.1)
    nrm[..., 2] += region.astype(np.float32)
    nrm[..., 3] = (np.float32(4.0) + rng.random((h, w), dtype=np.float32) * np.float32(0.5)) * alb[..., 3]
    if poison and h * w >= 16:
        k = max(1, h * w // 97)
        for buf, vals in ((col, (np.nan, np.inf, -np.inf)), (alb, (np.nan, np.inf)), (nrm, (np.nan, np.inf, -np.inf))):
            for v in vals:
                idx = rng.integers(0, h * w, k)
                buf.reshape(-1, 4)[idx, rng.integers(0, 4, k)] = v
    return col, alb, nrm


def _check(c, col, alb, nrm, what, **kw):
    out = np.full(col.shape, np.nan, np.float32)
    got = c.denoise(col, alb, nrm, out=out, **kw)
    assert got is out
    ref_kw = {k: v for k, v in kw.items() if k not in ("demodulate", "scene")}
    want = DR.denoise_ref(col, alb, nrm, flags=DR.DEMODULATE if kw.get("demodulate") else 0, **ref_kw)
    assert_bits_equal(out, want, what)
    return out


@pytest.fixture(scope="module")
def canonical_64(R, caster, scene):
    return _frame(R, caster, scene, 64, 64, 4)[:3]


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_canonical_view_for_every_iteration_count(caster, canonical_64, iterations, demodulate):
    """64 x 64 at 4 spp; iteration 4 has tap spacing 16, so a pixel's taps reach 32 pixels: most of them leave the image"""
    col, alb, nrm = canonical_64
    assert (alb[..., 3] == 0).any() and (alb[..., 3] == 1).any()
    out = _check(caster, col, alb, nrm, f"{iterations} iterations, demodulate={demodulate}", iterations=iterations, demodulate=demodulate)
    assert not np.array_equal(out[..., 0:3], col[..., 0:3]) and not out[..., 3].any()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 200), (50, 37), (257, 129)])
@pytest.mark.parametrize("demodulate", [False, True])
def test_sizes_that_end_inside_a_tile(caster, w, h, demodulate):
    col, alb, nrm = _synthetic(h, w, 100 + w, poison=False)
    _check(caster, col, alb, nrm, f"{w}x{h}", iterations=4, demodulate=demodulate)


@pytest.mark.parametrize("w,h", [(50, 37), (257, 129)])
def test_rendered_frames_of_odd_sizes(R, caster, scene, w, h):
    col, alb, nrm, _ = _frame(R, caster, scene, w, h, 2)
    _check(caster, col, alb, nrm, f"rendered {w}x{h}")


def test_axis_box_scene_with_non_finite_depth(R):
    """The centred rays (1 spp) parallel to the walls of the axis-aligned box give t = +-inf / NaN "hits": the depth guide
    holds them"""
    sp = recipe_axis_box()(ProductApi(R))
    c = R.HipRayCaster(seed=1)
    vp12 = R.create_viewport((33, 33), (1.0, 1.0), [0.0, 0.0, 0.0], R.unit([0.0, 0.0, 1.0]), 90.0, 0.0, 1, 1).vp12.copy()
    col, alb, nrm, _ = _frame(R, c, sp, 33, 33, 1, vp12)
    assert not np.isfinite(nrm[..., 3]).all()
    for demodulate in (False, True):
        _check(c, col, alb, nrm, "axis box", iterations=4, demodulate=demodulate)


@pytest.mark.parametrize("demodulate", [False, True])
def test_synthetic_images_with_nan_and_inf(caster, demodulate):
    col, alb, nrm = _synthetic(83, 131, 7)
    assert np.isnan(col).any() and np.isinf(alb).any() and np.isinf(nrm).any()
    out = _check(caster, col, alb, nrm, "synthetic", iterations=4, demodulate=demodulate, sigma_albedo=0.5)
    assert np.isfinite(out).sum() > out.size // 2


@pytest.mark.parametrize("off", ["sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo", "all"])
def test_each_sigma_switched_off(caster, canonical_64, off):
    col, alb, nrm = canonical_64
    kw = dict(sigma_albedo=0.3)
    for name in (("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo") if off == "all" else (off,)):
        kw[name] = INF
    _check(caster, col, alb, nrm, f"{off} = inf", **kw)
    s_col, s_alb, s_nrm = _synthetic(40, 70, 3)
    _check(caster, s_col, s_alb, s_nrm, f"synthetic, {off} = inf", **kw)


def test_1024_square_with_five_iterations(R, caster, scene):
    col, alb, nrm, _ = _frame(R, caster, scene, 1024, 1024, 2)
    _check(caster, col, alb, nrm, "1024 x 1024", iterations=5)


def test_two_sizes_on_one_handle_regrow_the_scratch(R):
    sp = recipe_canonical(maxdepth=6)(ProductApi(R))
    c = R.HipRayCaster(seed=1)
    for k, (w, h) in enumerate(((40, 24), (200, 160), (40, 24), (300, 90))):
        col, alb, nrm = _synthetic(h, w, 20 + k)
        _check(c, col, alb, nrm, f"call {k}: {w}x{h}", scene=sp, iterations=3)


def test_a_render_before_and_after_gives_equal_bits(R):
    sp = recipe_canonical(maxdepth=6)(ProductApi(R))
    c = R.HipRayCaster(seed=3)
    vp = R.canonical_viewport(96, 64, 5, 4)
    before = np.zeros((64, 96, 4), np.float32)
    c.walk_rays(vp, sp, before)
    alb0, nrm0, ids0, _ = c.walk_rays_features(vp, sp)
    _check(c, before, alb0, nrm0, "between the renders", iterations=5, demodulate=True)
    out = np.zeros_like(before)
    c.walk_rays_denoised(vp, sp, out)
    after = np.zeros_like(before)
    c.walk_rays(vp, sp, after)
    alb1, nrm1, ids1, _ = c.walk_rays_features(vp, sp)
    assert_bits_equal(after, before, "render after denoise")
    assert_bits_equal(alb1, alb0, "albedo after denoise")
    assert_bits_equal(nrm1, nrm0, "normal after denoise")
    assert np.array_equal(ids1, ids0)


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_device_variant_on_a_non_default_stream(caster, canonical_64, iterations):
    import torch
    col, alb, nrm = canonical_64
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        t_col, t_alb, t_nrm = (torch.from_numpy(x).to(dev, non_blocking=False) for x in (col, alb, nrm))
        t_out = torch.full(col.shape, float("nan"), dtype=torch.float32, device=dev)
        keep = [t.clone() for t in (t_col, t_alb, t_nrm)]
        caster.denoise_device(64, 64, t_col.data_ptr(), t_alb.data_ptr(), t_nrm.data_ptr(), t_out.data_ptr(), stream=st.cuda_stream,
                              iterations=iterations, demodulate=True)
        t_twice = t_out * 2.0  # queued behind the filter on the same stream
    st.synchronize()
    want = DR.denoise_ref(col, alb, nrm, iterations=iterations, flags=DR.DEMODULATE)
    assert_bits_equal(t_out.cpu().numpy(), want, "device variant")
    assert_bits_equal(t_twice.cpu().numpy(), want * np.float32(2.0), "work queued behind it")
    for t, k in zip((t_col, t_alb, t_nrm), keep):  # the inputs are read only
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))


@pytest.mark.parametrize("kw", [dict(), dict(iterations=4, demodulate=True, sigma_color=0.5)])
def test_walk_rays_denoised_equals_the_three_calls(R, caster, scene, kw):
    w, h, spp = 80, 56, 4
    col, alb, nrm, vp = _frame(R, caster, scene, w, h, spp)
    sep = caster.denoise(col, alb, nrm, **kw)
    one = np.full((h, w, 4), np.nan, np.float32)
    ctx = caster.walk_rays_denoised(vp, scene, one, **kw)
    assert_bits_equal(one, sep, "walk_rays_denoised vs render + features + denoise")
    ref_kw = {k: v for k, v in kw.items() if k != "demodulate"}
    assert_bits_equal(one, DR.denoise_ref(col, alb, nrm, flags=DR.DEMODULATE if kw.get("demodulate") else 0, **ref_kw), "vs the restatement")
    plain = np.zeros_like(col)
    assert ctx.total_rays == caster.walk_rays(vp, scene, plain).total_rays


def test_analytic_spheres_are_refused_by_walk_rays_denoised(R):
    from conftest import recipe_circles_analytic
    sp = recipe_circles_analytic()(ProductApi(R))
    with pytest.raises(RuntimeError, match="analytic spheres"):
        R.HipRayCaster(seed=1).walk_rays_denoised(R.canonical_viewport(16, 16, 5, 2), sp, np.zeros((16, 16, 4), np.float32))
