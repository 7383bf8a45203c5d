"""-m gpu: variance-guided denoising (rtmi_variance* / rtmi_denoise_var* / rtmi_render_adaptive_denoised; HipRayCaster.variance,
variance_device, denoise_var, denoise_var_device, walk_rays_adaptive_denoised).  Every float of every result is compared with
assert_bits_equal against the NumPy restatement of tests/denoise_var_ref.py applied to the same input images; the expected
values never come from the code under test."""
import numpy as np
import pytest

from conftest import ProductApi, assert_bits_equal, recipe_axis_box, recipe_canonical
import denoise_ref as DR
import denoise_var_ref as DV

pytestmark = pytest.mark.gpu
INF = float("inf")
S, M, P, DEPTH = 32, 8, 8, 5


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


def _adaptive_frame(R, c, sp, w, h, spp, m, p, rel, ab, vp12=None, depth=DEPTH):
    """An adaptive render on device buffers and the features of its first m samples: dict of host arrays accum, sumsq, counts,
    color, albedo, normal and var (rtmi_variance_device on the render's own device buffers)."""
    import torch
    dev = torch.device("cuda", 0)
    vp = R.canonical_viewport(w, h, depth, spp) if vp12 is None else R.Viewport(w, h, vp12, depth, spp)
    acc, sq, col, var = (torch.zeros((h, w, 4), dtype=torch.float32, device=dev) for _ in range(4))
    cnt = torch.zeros((h, w), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ctx = c.walk_adaptive_device(vp, sp, (0, h, h, 0), acc.data_ptr(), sq.data_ptr(), cnt.data_ptr(), col.data_ptr(), st,
                                 min_samples=m, pass_samples=p, rel_tol=rel, abs_tol=ab)
    c.variance_device(acc.data_ptr(), sq.data_ptr(), cnt.data_ptr(), w * h, var.data_ptr(), stream=st, scene=sp)
    torch.cuda.synchronize()
    alb, nrm, _, _ = c.walk_rays_features(vp, sp, sample0=0, nsamples=m, ids=False)
    return dict(accum=acc.cpu().numpy(), sumsq=sq.cpu().numpy(), counts=cnt.cpu().numpy().view(np.uint32), color=col.cpu().numpy(),
                var=var.cpu().numpy(), albedo=alb, normal=nrm, vp=vp, ctx=ctx)


@pytest.fixture(scope="module")
def adaptive_64(R, caster, scene):
    """The canonical view at 64 x 64, S = 32, m = p = 8, with a tolerance picked as tests/test_adaptive.py picks it: the first
    whose replayed count map holds m, S and a value between."""
    from test_adaptive import _sample_colours, pick_tol
    cols = _sample_colours(caster, R, scene, 64, 64, S, depth=DEPTH)
    rel, ab = pick_tol(cols, M, P)
    f = _adaptive_frame(R, caster, scene, 64, 64, S, M, P, rel, ab)
    f["tol"] = (rel, ab)
    return f


def _synthetic(h, w, seed, poison=True):
    """Random colour, variance and guides: coverage in {0, 0.5, 1}, a few flat regions so that every term passes somewhere,
    variances from 0 to the size of the colour differences, and NaN / +-inf injected into every buffer."""
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
    var = np.zeros((h, w, 4), np.float32)
    var[..., 0:3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(0.05) * (rng.random((h, w, 1), dtype=np.float32) < 0.8)
    var[..., 3] = DV.lane_sum(var[..., 0:3])
    if poison and h * w >= 16:
        k = max(1, h * w // 97)
        for buf, vals in ((col, (np.nan, np.inf, -np.inf)), (alb, (np.nan, np.inf)), (nrm, (np.nan, np.inf, -np.inf)),
                          (var, (np.nan, np.inf, -np.inf))):
            for v in vals:
                idx = rng.integers(0, h * w, k)
                buf.reshape(-1, 4)[idx, rng.integers(0, 4, k)] = v
    return col, alb, nrm, var


def _check(c, col, alb, nrm, var, what, with_var_out=True, **kw):
    out = np.full(col.shape, np.nan, np.float32)
    ref_kw = {k: v for k, v in kw.items() if k not in ("demodulate", "scene")}
    want, want_var = DV.denoise_var_ref(col, alb, nrm, var, flags=DR.DEMODULATE if kw.get("demodulate") else 0, **ref_kw)
    if with_var_out:
        vout = np.full(col.shape, np.nan, np.float32)
        got = c.denoise_var(col, alb, nrm, var, out=out, var_out=vout, **kw)
        assert got[0] is out and got[1] is vout
        assert_bits_equal(vout, want_var, what + ": var_out")
    else:
        assert c.denoise_var(col, alb, nrm, var, out=out, **kw) is out
    assert_bits_equal(out, want, what)
    return out


def test_variance_of_an_adaptive_render(adaptive_64):
    f = adaptive_64
    u = set(np.unique(f["counts"]).tolist())
    assert M in u and S in u and len(u) >= 3, u
    assert_bits_equal(f["var"], DV.variance_ref(f["accum"], f["sumsq"], f["counts"]), "k_variance on the render's device buffers")
    assert (f["var"][..., 3] == 0).any() and (f["var"][..., 3] > 0).any()  # sky / Solid pixels, and noisy ones


def test_variance_of_random_moments_with_poison(caster, scene):
    rng = np.random.default_rng(17)
    n = 70001  # more than one block per CU's worth of one launch round, and no multiple of 256
    cnt = rng.integers(2, 40, n).astype(np.uint32)
    smp_mean = rng.random((n, 4), dtype=np.float32)
    s = smp_mean * cnt[:, None].astype(np.float32)
    q = s * smp_mean * (np.float32(1.0) + rng.random((n, 4), dtype=np.float32) * np.float32(0.2) - np.float32(0.02))
    cnt[rng.integers(0, n, 50)] = 0
    cnt[rng.integers(0, n, 50)] = 1
    cnt[rng.integers(0, n, 50)] = 2
    cnt[rng.integers(0, n, 5)] = 0xFFFFFFFF
    for buf in (s, q):
        for v in (np.nan, np.inf, -np.inf):
            buf[rng.integers(0, n, 40), rng.integers(0, 4, 40)] = v
    got = caster.variance(s, q, cnt, scene=scene)
    want = DV.variance_ref(s, q, cnt)
    assert np.isnan(want).any() and np.isposinf(want).any() and (want[..., 0:3] == 0).any()
    assert_bits_equal(got, want, "k_variance on random moments")
    for shape in ((1,), (3, 5), (2, 3, 7)):  # any layout: the call takes npixels
        m = int(np.prod(shape))
        g2 = caster.variance(s[:m].reshape(shape + (4,)).copy(), q[:m].reshape(shape + (4,)).copy(), cnt[:m].reshape(shape).copy(), scene=scene)
        assert_bits_equal(g2, want[:m].reshape(shape + (4,)), f"shape {shape}")


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_adaptive_frame_for_every_iteration_count(caster, adaptive_64, iterations, demodulate):
    """64 x 64; iteration 4 has tap spacing 16, so a pixel's taps reach 32 pixels: most of them leave the image.  With and
    without var_out: the colour must not depend on it."""
    f = adaptive_64
    args = (f["color"], f["albedo"], f["normal"], f["var"])
    assert (f["albedo"][..., 3] == 0).any() and (f["albedo"][..., 3] == 1).any()
    out = _check(caster, *args, f"{iterations} iterations, demodulate={demodulate}", iterations=iterations, demodulate=demodulate)
    _check(caster, *args, f"{iterations} iterations, demodulate={demodulate}, no var_out", with_var_out=False,
           iterations=iterations, demodulate=demodulate)
    assert not np.array_equal(out[..., 0:3], f["color"][..., 0:3]) and not out[..., 3].any()


def test_defaults(caster, adaptive_64):
    f = adaptive_64
    _check(caster, f["color"], f["albedo"], f["normal"], f["var"], "defaults")


@pytest.mark.parametrize("w,h", [(1, 1), (3, 200), (50, 37), (257, 129)])
@pytest.mark.parametrize("demodulate", [False, True])
def test_sizes_that_end_inside_a_tile(caster, w, h, demodulate):
    col, alb, nrm, var = _synthetic(h, w, 100 + w, poison=False)
    _check(caster, col, alb, nrm, var, f"{w}x{h}", iterations=4, demodulate=demodulate)


def test_axis_box_scene_with_non_finite_depth(R):
    """The centred rays of the axis-aligned box's view give t = +-inf / NaN "hits": the depth guide holds them.  The frame is
    an adaptive one with min_samples = S, i.e. the moments of a uniform render."""
    sp = recipe_axis_box()(ProductApi(R))
    c = R.HipRayCaster(seed=1)
    vp12 = R.create_viewport((33, 33), (1.0, 1.0), [0.0, 0.0, 0.0], R.unit([0.0, 0.0, 1.0]), 90.0, 0.0, 1, 1).vp12.copy()
    f = _adaptive_frame(R, c, sp, 33, 33, 4, 4, 4, 0.0, 0.0, vp12=vp12, depth=1)
    one = R.Viewport(33, 33, vp12, 1, 1)  # the guides of the centred rays, whose depth is not finite
    alb, nrm, _, _ = c.walk_rays_features(one, sp, ids=False)
    assert not np.isfinite(nrm[..., 3]).all()
    assert_bits_equal(f["var"], DV.variance_ref(f["accum"], f["sumsq"], f["counts"]), "axis box variance")
    for demodulate in (False, True):
        _check(c, f["color"], alb, nrm, f["var"], "axis box", iterations=4, demodulate=demodulate)


@pytest.mark.parametrize("demodulate", [False, True])
def test_synthetic_images_with_nan_and_inf(caster, demodulate):
    col, alb, nrm, var = _synthetic(83, 131, 7)
    assert np.isnan(col).any() and np.isinf(alb).any() and np.isinf(nrm).any() and np.isnan(var).any() and np.isinf(var).any()
    out = _check(caster, col, alb, nrm, var, "synthetic", iterations=4, demodulate=demodulate, sigma_albedo=0.5)
    assert np.isfinite(out).sum() > out.size // 2


@pytest.mark.parametrize("off", ["sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo", "all"])
def test_each_sigma_switched_off(caster, adaptive_64, off):
    f = adaptive_64
    kw = dict(sigma_albedo=0.3, iterations=3)
    for name in (("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo") if off == "all" else (off,)):
        kw[name] = INF
    _check(caster, f["color"], f["albedo"], f["normal"], f["var"], f"{off} = inf", **kw)
    _check(caster, *_synthetic(40, 70, 3), f"synthetic, {off} = inf", **kw)


def test_1024_square_with_five_iterations(R, caster, scene):
    f = _adaptive_frame(R, caster, scene, 1024, 1024, 4, 2, 2, 0.05, 0.01)
    _check(caster, f["color"], f["albedo"], f["normal"], f["var"], "1024 x 1024", iterations=5)


def test_several_sizes_on_one_handle_regrow_the_scratch(R):
    sp = recipe_canonical(maxdepth=6)(ProductApi(R))
    c = R.HipRayCaster(seed=1)
    for k, (w, h) in enumerate(((40, 24), (200, 160), (40, 24), (300, 90))):
        _check(c, *_synthetic(h, w, 20 + k), f"call {k}: {w}x{h}", scene=sp, iterations=3)


def test_renders_and_the_plain_filter_before_and_after_give_equal_bits(R):
    sp = recipe_canonical(maxdepth=6)(ProductApi(R))
    c = R.HipRayCaster(seed=3)
    vp = R.canonical_viewport(96, 64, 5, 4)
    before = np.zeros((64, 96, 4), np.float32)
    c.walk_rays(vp, sp, before)
    alb0, nrm0, ids0, _ = c.walk_rays_features(vp, sp)
    den0 = c.denoise(before, alb0, nrm0, iterations=3)
    _, _, _, var = _synthetic(64, 96, 31, poison=False)
    _check(c, before, alb0, nrm0, var, "between the renders", iterations=5, demodulate=True)
    data = np.zeros_like(before)
    c.walk_rays_adaptive_denoised(R.canonical_viewport(96, 64, 5, 8), sp, data, min_samples=2, pass_samples=2, iterations=3)
    after = np.zeros_like(before)
    c.walk_rays(vp, sp, after)
    alb1, nrm1, ids1, _ = c.walk_rays_features(vp, sp)
    den1 = c.denoise(after, alb1, nrm1, iterations=3)
    assert_bits_equal(after, before, "render after denoise_var")
    assert_bits_equal(alb1, alb0, "albedo after denoise_var")
    assert_bits_equal(nrm1, nrm0, "normal after denoise_var")
    assert np.array_equal(ids1, ids0)
    assert_bits_equal(den1, den0, "rtmi_denoise after denoise_var")


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_device_variant_on_a_non_default_stream(caster, adaptive_64, iterations):
    import torch
    f = adaptive_64
    imgs = (f["color"], f["albedo"], f["normal"], f["var"])
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        ts = [torch.from_numpy(x).to(dev, non_blocking=False) for x in imgs]
        t_out = torch.full(imgs[0].shape, float("nan"), dtype=torch.float32, device=dev)
        t_var = torch.full(imgs[0].shape, float("nan"), dtype=torch.float32, device=dev)
        keep = [t.clone() for t in ts]
        caster.denoise_var_device(64, 64, *[t.data_ptr() for t in ts], t_out.data_ptr(), var_out_ptr=t_var.data_ptr(),
                                  stream=st.cuda_stream, iterations=iterations, demodulate=True)
        t_twice = t_out * 2.0  # queued behind the filter on the same stream
    st.synchronize()
    want, want_var = DV.denoise_var_ref(*imgs, iterations=iterations, flags=DR.DEMODULATE)
    assert_bits_equal(t_out.cpu().numpy(), want, "device variant")
    assert_bits_equal(t_var.cpu().numpy(), want_var, "device variant: var_out")
    assert_bits_equal(t_twice.cpu().numpy(), want * np.float32(2.0), "work queued behind it")
    for t, k in zip(ts, keep):  # the inputs are read only
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))


@pytest.mark.parametrize("w,h", [(3, 200), (50, 37)])
def test_staged_and_direct_taps_give_equal_bits_at_spacings_1_and_2(R, monkeypatch, w, h):
    """Both filters, 2 iterations (tap spacings 1 and 2), on a handle that stages nothing through LDS (both *_LDS_STEP = 0:
    every tap is global loads) and on one with the defaults (both spacings staged).  The sizes give partial tiles and halo
    slots outside the image on every side.  The two handles must agree bit for bit, and with the restatements."""
    import torch
    handles = []
    for lds in ("0", None):
        for name in ("RTMI_DENOISE_LDS_STEP", "RTMI_DENOISE_VAR_LDS_STEP"):
            if lds is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, lds)
        sp = recipe_axis_box()(ProductApi(R))
        c = R.HipRayCaster(seed=1)
        c.upload(sp)  # the variables are read when the device handle is made
        handles.append((c, sp))
    imgs = _synthetic(h, w, 300 + w, poison=False)
    assert (imgs[1][..., 3] == 0).any() and (imgs[1][..., 3] != 0).any()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    ts = [torch.from_numpy(x).to(dev) for x in imgs]
    names = ("plain filter", "variance-guided filter", "variance-guided filter: var_out")
    for demodulate in (False, True):
        fl = DR.DEMODULATE if demodulate else 0
        want = (DR.denoise_ref(*imgs[:3], iterations=2, flags=fl),) + tuple(DV.denoise_var_ref(*imgs, iterations=2, flags=fl))
        got = []
        for c, sp in handles:
            outs = [torch.full(imgs[0].shape, float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
            c.denoise_device(w, h, *[t.data_ptr() for t in ts[:3]], outs[0].data_ptr(), stream=st, scene=sp, iterations=2,
                             demodulate=demodulate)
            c.denoise_var_device(w, h, *[t.data_ptr() for t in ts], outs[1].data_ptr(), var_out_ptr=outs[2].data_ptr(), stream=st,
                                 scene=sp, iterations=2, demodulate=demodulate)
            torch.cuda.synchronize()
            got.append([t.cpu().numpy() for t in outs])
        for direct, staged, ref, name in zip(got[0], got[1], want, names):
            what = f"{w}x{h}, demodulate={demodulate}, {name}"
            assert_bits_equal(direct, staged, what + ": direct vs staged")
            assert_bits_equal(staged, ref, what + ": staged vs the restatement")
            assert_bits_equal(direct, ref, what + ": direct vs the restatement")


@pytest.mark.parametrize("kw", [dict(), dict(iterations=4, demodulate=True, sigma_color=2.0)])
def test_walk_rays_adaptive_denoised_equals_the_four_calls(R, caster, scene, adaptive_64, kw):
    f = adaptive_64
    rel, ab = f["tol"]
    sep = caster.denoise_var(f["color"], f["albedo"], f["normal"], f["var"], **kw)
    one = np.full((64, 64, 4), np.nan, np.float32)
    ctx = caster.walk_rays_adaptive_denoised(f["vp"], scene, one, min_samples=M, pass_samples=P, rel_tol=rel, abs_tol=ab, **kw)
    assert_bits_equal(one, sep, "walk_rays_adaptive_denoised vs adaptive render + variance + features + denoise_var")
    ref_kw = {k: v for k, v in kw.items() if k != "demodulate"}
    want, _ = DV.denoise_var_ref(f["color"], f["albedo"], f["normal"], f["var"], flags=DR.DEMODULATE if kw.get("demodulate") else 0, **ref_kw)
    assert_bits_equal(one, want, "vs the restatement")
    assert np.array_equal(ctx.counts, f["counts"])
    assert (ctx.passes, ctx.unconverged, ctx.samples) == (f["ctx"].passes, f["ctx"].unconverged, f["ctx"].samples)
    assert ctx.samples == int(f["counts"].sum()) and ctx.total_rays == f["ctx"].total_rays


def test_analytic_spheres_are_refused_by_walk_rays_adaptive_denoised(R):
    from conftest import recipe_circles_analytic
    sp = recipe_circles_analytic()(ProductApi(R))
    with pytest.raises(RuntimeError, match="analytic spheres"):
        R.HipRayCaster(seed=1).walk_rays_adaptive_denoised(R.canonical_viewport(16, 16, 5, 4), sp, np.zeros((16, 16, 4), np.float32),
                                                           min_samples=2, pass_samples=2)
