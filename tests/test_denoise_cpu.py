"""The a-trous denoiser (rtmi_denoise / rtmi_denoise_device / rtmi_render_denoised): the entry points exist and refuse bad
arguments before any HIP call and before the scene is used, the Python methods validate their arguments, and the NumPy
restatement the GPU tests compare with (tests/denoise_ref.py) has the properties the definition promises and lowers the error
of 2- and 4-sample renders against a 256-sample one.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from conftest import OracleApi, assert_bits_equal, recipe_canonical, recipe_circles
import denoise_ref as DR
import features_ref as FR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_denoise_defaults", "rtmi_denoise", "rtmi_denoise_device", "rtmi_render_denoised", "rth_caster_denoise",
         "rth_caster_denoise_device", "rth_caster_walk_denoised")
BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails
CO, AL, NO, OUT = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)  # never touched: every call fails
INF, NAN = float("inf"), float("nan")


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _params(**kw):
    ffi, L = _lib()
    d = ffi.Denoise()
    L.rtmi_denoise_defaults(C.byref(d))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _both(w=8, h=6, bufs=(CO, AL, NO, OUT), scene=BOGUS, params=None, no_params=False):
    """(rc, message) of the device and of the host variant for the same arguments"""
    ffi, L = _lib()
    d = _params() if params is None else params
    pd = None if no_params else C.byref(d)
    res = []
    rc = L.rtmi_denoise_device(scene, w, h, bufs[0], bufs[1], bufs[2], pd, bufs[3], None)
    res.append((rc, L.rtmi_last_error()))
    rc = L.rtmi_denoise(scene, w, h, bufs[0], bufs[1], bufs[2], pd, bufs[3])
    res.append((rc, L.rtmi_last_error()))
    return res


def test_denoise_entry_points_are_exported_and_listed():
    ffi, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name


def test_defaults_are_the_documented_ones():
    d = _params()
    assert (d.iterations, d.flags) == (3, 0)
    assert (d.sigma_color, d.sigma_normal, d.sigma_depth, d.sigma_albedo) == (1.0, 0.5, float(np.float32(0.1)), INF)
    assert C.sizeof(d) == 24
    assert {k: getattr(d, k) for k in DR.DEFAULTS} == {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in DR.DEFAULTS.items()}
    _lib()[1].rtmi_denoise_defaults(None)  # tolerated


def test_null_scene_params_and_buffers_are_refused():
    for rc, msg in _both(scene=None):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and b"scene" in msg, msg
    for rc, msg in _both(no_params=True):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and b"params" in msg, msg
    for k, word in enumerate((b"color", b"albedo", b"normal", b"out")):
        bufs = [CO, AL, NO, OUT]
        bufs[k] = None
        for rc, msg in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"NULL" in msg and word in msg, msg


def test_an_output_that_aliases_an_input_is_refused():
    for bufs, word in (((CO, AL, NO, CO), b"color"), ((CO, AL, NO, AL), b"albedo"), ((CO, AL, NO, NO), b"normal")):
        for rc, msg in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"alias" in msg and word in msg, msg


def test_empty_and_oversized_images_are_refused():
    for w, h in ((0, 6), (8, 0), (0, 0)):
        for rc, msg in _both(w=w, h=h):
            assert rc == RTMI_ERR_INVALID and b"empty image" in msg, msg
    for w, h in ((65536, 65536), (0xFFFFFFFF, 2)):
        for rc, msg in _both(w=w, h=h):
            assert rc == RTMI_ERR_UNSUPPORTED and b"2^32" in msg, msg


@pytest.mark.parametrize("kw,word", [
    (dict(iterations=0), b"iterations"), (dict(iterations=9), b"iterations"), (dict(iterations=0xFFFFFFFF), b"iterations"),
    (dict(flags=2), b"flags"), (dict(flags=3), b"flags"), (dict(flags=0x80000000), b"flags"),
    (dict(sigma_color=0.0), b"sigma_color"), (dict(sigma_color=NAN), b"sigma_color"), (dict(sigma_color=-1.0), b"sigma_color"),
    (dict(sigma_normal=0.0), b"sigma_normal"), (dict(sigma_normal=NAN), b"sigma_normal"), (dict(sigma_normal=-INF), b"sigma_normal"),
    (dict(sigma_depth=-0.0), b"sigma_depth"), (dict(sigma_depth=NAN), b"sigma_depth"),
    (dict(sigma_albedo=0.0), b"sigma_albedo"), (dict(sigma_albedo=NAN), b"sigma_albedo"),
])
def test_bad_parameters_are_refused(kw, word):
    for rc, msg in _both(params=_params(**kw)):
        assert rc == RTMI_ERR_INVALID and word in msg, msg


def test_render_denoised_checks_its_arguments_first():
    from test_features_cpu import Vp, _vp
    ffi, L = _lib()
    vp, d, st = _vp(), _params(), ffi.Stats()
    st.rays = 123
    assert L.rtmi_render_denoised(None, C.byref(vp), 1, C.byref(d), OUT, C.byref(st)) == RTMI_ERR_INVALID
    assert b"scene" in L.rtmi_last_error() and st.rays == 0
    assert L.rtmi_render_denoised(BOGUS, None, 1, C.byref(d), OUT, None) == RTMI_ERR_INVALID
    assert b"viewport" in L.rtmi_last_error()
    assert L.rtmi_render_denoised(BOGUS, C.byref(vp), 1, None, OUT, None) == RTMI_ERR_INVALID
    assert b"params" in L.rtmi_last_error()
    assert L.rtmi_render_denoised(BOGUS, C.byref(vp), 1, C.byref(d), None, None) == RTMI_ERR_INVALID
    assert b"out" in L.rtmi_last_error()
    assert L.rtmi_render_denoised(BOGUS, C.byref(_vp(w=0)), 1, C.byref(d), OUT, None) == RTMI_ERR_INVALID
    assert b"empty image" in L.rtmi_last_error()
    assert L.rtmi_render_denoised(BOGUS, C.byref(vp), 1, C.byref(_params(iterations=9)), OUT, None) == RTMI_ERR_INVALID
    assert b"iterations" in L.rtmi_last_error()
    assert isinstance(vp, Vp)


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    good = np.zeros((6, 8, 4), np.float32)
    with pytest.raises(ValueError):  # no scene yet
        c.denoise(good, good.copy(), good.copy())
    bads = (np.zeros((6, 8, 3), np.float32), np.zeros((8, 6, 4), np.float32), np.zeros((6, 8, 4), np.float64),
            np.zeros((6, 16, 4), np.float32)[:, ::2], np.zeros(192, np.float32), [[0.0]])
    for bad in bads:
        for k in range(4):
            args = [good.copy(), good.copy(), good.copy(), good.copy()]
            args[k] = bad
            with pytest.raises(ValueError):
                c.denoise(*args, scene=sp)
    with pytest.raises(ValueError):
        c.denoise(good, good.copy(), good.copy(), out=good, scene=sp)
    a = good.copy()
    with pytest.raises(ValueError):
        c.denoise(good, a, good.copy(), out=a, scene=sp)
    for kw in (dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_normal=NAN), dict(sigma_depth=-1.0),
               dict(sigma_albedo=0.0)):
        with pytest.raises(ValueError):
            c.denoise(good, good.copy(), good.copy(), scene=sp, **kw)
        with pytest.raises(ValueError):
            c.denoise_device(8, 6, 4096, 8192, 12288, 16384, scene=sp, **kw)
        with pytest.raises(ValueError):
            c.walk_rays_denoised(R.canonical_viewport(8, 6, 5, 4), sp, good.copy(), **kw)
    with pytest.raises(TypeError):
        c.denoise(good, good.copy(), good.copy(), scene=sp, sigma=1.0)
    for ptrs in ((0, 8192, 12288, 16384), (4096, None, 12288, 16384), (4096, 8192, 12288, 0), (4096, 8192, 12288, 4096),
                 (4096, 8192, 12288, 12288)):
        with pytest.raises(ValueError):
            c.denoise_device(8, 6, *ptrs, scene=sp)
    for w, h in ((0, 6), (8, 0)):
        with pytest.raises(ValueError):
            c.denoise_device(w, h, 4096, 8192, 12288, 16384, scene=sp)
    with pytest.raises(ValueError):
        c.denoise_device(8, 6, 4096, 8192, 12288, 16384)  # no scene
    for bad in (np.zeros((6, 8, 3), np.float32), np.zeros((6, 8, 4), np.float64), np.zeros((6, 16, 4), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            c.walk_rays_denoised(R.canonical_viewport(8, 6, 5, 4), sp, bad)
    p = R.HipRayCaster.denoise_params(iterations=5, demodulate=True, sigma_albedo=0.25)
    assert (p.iterations, p.flags, p.sigma_albedo, p.sigma_color) == (5, 1, 0.25, 1.0)


# ---------------------------------------------------------------- properties of the restatement
def _guides(h, w, rng, full=True):
    alb = rng.random((h, w, 4), dtype=np.float32)
    alb[..., 3] = 1.0 if full else rng.integers(0, 3, (h, w)).astype(np.float32) * 0.5
    nrm = rng.standard_normal((h, w, 4)).astype(np.float32)
    nrm[..., 3] = 1.0 + rng.random((h, w), dtype=np.float32) * 9.0
    return alb, nrm


@pytest.mark.parametrize("flags", [0, DR.DEMODULATE])
def test_a_constant_image_is_a_fixed_point(flags):
    """Bit for bit: the colours, the k products (multiples of 1/256) and every g (exactly 1 at distance 0) are short dyadic
    numbers, so every product and sum is exact and num / den returns the colour; albedo + 1/256 is a power of two, so
    demodulation and remodulation are exact too."""
    h, w = 19, 37
    col = np.zeros((h, w, 4), np.float32)
    col[..., 0:3] = np.array([0.25, 0.5, 0.75], np.float32)
    col[..., 3] = 7.0  # ignored
    alb = np.zeros((h, w, 4), np.float32)
    alb[...] = np.array([0.5 - 1.0 / 256.0, 0.25 - 1.0 / 256.0, 1.0 - 1.0 / 256.0, 1.0], np.float32)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[...] = np.array([0.0, 0.0, -1.0, 4.0], np.float32)
    out = DR.denoise_ref(col, alb, nrm, iterations=5, flags=flags)
    want = col.copy()
    want[..., 3] = 0.0
    assert_bits_equal(out, want, "constant image")


def test_a_nan_pixel_stays_nan_and_poisons_nobody():
    rng = np.random.default_rng(5)
    h, w = 24, 31
    col = rng.random((h, w, 4), dtype=np.float32)
    alb, nrm = _guides(h, w, rng)
    col[7, 9, 1] = np.nan
    col[15, 20, 0:3] = np.inf
    col[0, 0, 2] = np.nan
    nrm[3, 3, 3] = np.inf   # depth of a degenerate hit
    nrm[4, 25, 0] = np.nan
    alb[20, 5, 3] = np.nan
    for kw in (dict(), dict(sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)):
        out = DR.denoise_ref(col, alb, nrm, iterations=4, **kw)
        bad = ~np.isfinite(out[..., 0:3]).all(axis=2)
        want = np.zeros((h, w), bool)
        want[7, 9] = want[15, 20] = want[0, 0] = True
        assert np.array_equal(bad, want), np.argwhere(bad != want)
        assert np.isnan(out[7, 9, 1]) and np.isnan(out[0, 0, 2])
        assert not out[..., 3].any()


def test_all_sigmas_inf_on_full_coverage_is_the_plain_b3_spline():
    rng = np.random.default_rng(11)
    h, w = 21, 26
    col = rng.random((h, w, 4), dtype=np.float32)
    alb, nrm = _guides(h, w, rng)
    out = DR.denoise_ref(col, alb, nrm, iterations=3, sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    u = col[..., 0:3].copy()
    for i in range(3):  # the same taps in the same order, weights k*k alone
        num, den = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                kk = np.float32(DR.K[dy + 2] * DR.K[dx + 2])
                for y in range(h):
                    for x in range(w):
                        qy, qx = y + (dy << i), x + (dx << i)
                        if 0 <= qy < h and 0 <= qx < w:
                            num[y, x] = num[y, x] + kk * u[qy, qx]
                            den[y, x] = den[y, x] + kk
        u = num / den[..., None]
    assert_bits_equal(out[..., 0:3], u, "B3 spline")


def test_a_1x1_image_is_returned_unchanged():
    """Only the centre tap exists: u' = (w * u) / w with w = k[2] * k[2] = 9/64, per iteration.  That is u itself, bit for
    bit, wherever 9 u is representable (asserted on such colours for 8 iterations); for any other u the stated operations
    leave a rounding of at most one ulp per iteration, and the restatement must return exactly that value."""
    alb = np.array([[[0.2, 0.4, 0.6, 1.0]]], np.float32)
    nrm = np.array([[[0.0, 1.0, 0.0, 3.0]]], np.float32)
    col = np.array([[[0.25, 0.5, 0.8125, 5.0]]], np.float32)
    out = DR.denoise_ref(col, alb, nrm, iterations=8)
    assert_bits_equal(out, np.array([[[0.25, 0.5, 0.8125, 0.0]]], np.float32), "1x1")
    col = np.array([[[0.3, 0.6, 0.9, 5.0]]], np.float32)
    out = DR.denoise_ref(col, alb, nrm, iterations=1)
    w = np.float32(0.140625)
    assert_bits_equal(out[0, 0, 0:3], (w * col[0, 0, 0:3]) / w, "1x1, the definition's value")
    assert (np.abs(out[0, 0, 0:3] - col[0, 0, 0:3]) <= np.spacing(col[0, 0, 0:3])).all() and out[0, 0, 3] == 0.0


def test_sky_beside_sky_uses_the_colour_term_alone():
    """Two sky pixels with different (meaningless) guides still blend; a sky pixel and a hit never do (coverage term)."""
    col = np.zeros((1, 2, 4), np.float32)
    col[0, 0, 0:3], col[0, 1, 0:3] = 0.2, 0.4
    alb = np.zeros((1, 2, 4), np.float32)
    nrm = np.zeros((1, 2, 4), np.float32)
    nrm[0, 1] = (0.0, 0.0, 1.0, 0.0)
    out = DR.denoise_ref(col, alb, nrm, iterations=1)
    assert 0.2 < out[0, 0, 0] < 0.4 and 0.2 < out[0, 1, 0] < 0.4
    alb[0, 1, 3] = 1.0
    nrm[0, 1, 3] = 5.0
    out = DR.denoise_ref(col, alb, nrm, iterations=1)
    assert_bits_equal(out[..., 0:3], col[..., 0:3], "sky beside a hit")


# ---------------------------------------------------------------- quality, with the oracle only
def _rmse(a, b):
    d = a[..., 0:3].astype(np.float64) - b[..., 0:3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


@pytest.fixture(scope="module")
def quality_scenes():
    from oracle import orc
    w = h = 96
    vp = orc.canonical_viewport(w, h)
    res = {}
    for name, recipe in (("canonical", recipe_canonical(maxdepth=8)), ("circles", recipe_circles())):
        so = recipe(OracleApi(orc))
        truth, _ = so.render(w, h, vp, 5, 256, seed=7, threads=8)
        res[name] = (so, truth)
    return orc, w, h, vp, res


@pytest.mark.parametrize("scene", ["canonical", "circles"])
@pytest.mark.parametrize("spp", [2, 4])
def test_the_default_filter_lowers_the_error_of_a_low_sample_render(quality_scenes, scene, spp):
    """RMSE over rgb against a 256-spp render (seed 7) of the input at `spp` samples (seed 1) and of its filtered image at
    the defaults.  Measured, input -> filtered: canonical 2 spp 0.0570 -> 0.0402, 4 spp 0.0420 -> 0.0285; circles 2 spp
    0.0345 -> 0.0299, 4 spp 0.0256 -> 0.0225.  Asserted: strictly lower, nothing more -- a filter that
    fails that is not a denoiser."""
    orc, w, h, vp, res = quality_scenes
    so, truth = res[scene]
    noisy, _ = so.render(w, h, vp, 5, spp, seed=1, threads=8)
    alb, nrm, _, _ = FR.features_ref(orc, so, w, h, vp, spp, 1)
    out = DR.denoise_ref(noisy, alb, nrm, **DR.DEFAULTS)
    before, after = _rmse(noisy, truth), _rmse(out, truth)
    print(f"{scene} {spp} spp: RMSE {before:.4f} -> {after:.4f}")
    assert after < before
