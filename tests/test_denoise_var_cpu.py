"""Variance-guided denoising (rtmi_variance* / rtmi_denoise_var* / rtmi_render_adaptive_denoised): the entry points exist and
refuse bad arguments before any HIP call and before the scene is used, the Python methods validate their arguments, and the
NumPy restatement the GPU tests compare with (tests/denoise_var_ref.py) has the properties the definition promises and, at the
defaults, lowers the error of frames of 4, 8 and 16 samples against a 256-spp render.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from conftest import OracleApi, assert_bits_equal, recipe_canonical, recipe_circles
import denoise_ref as DR
import denoise_var_ref as DV
import features_ref as FR

RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_denoise_var_defaults", "rtmi_variance", "rtmi_variance_device", "rtmi_denoise_var", "rtmi_denoise_var_device",
         "rtmi_render_adaptive_denoised", "rth_caster_variance", "rth_caster_variance_device", "rth_caster_denoise_var",
         "rth_caster_denoise_var_device", "rth_caster_walk_adaptive_denoised")
BOGUS = C.c_void_p(0x10)  # a dangling scene handle: never dereferenced when a check fails
CO, AL, NO, VA, OUT, VO = (C.c_void_p(0x1000 * k) for k in range(1, 7))  # never touched: every call fails
INF, NAN = float("inf"), float("nan")
F32 = np.float32


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _params(**kw):
    ffi, L = _lib()
    d = ffi.Denoise()
    L.rtmi_denoise_var_defaults(C.byref(d))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _both(w=8, h=6, bufs=(CO, AL, NO, VA, OUT, VO), scene=BOGUS, params=None, no_params=False):
    """(rc, message) of the device and of the host variant for the same arguments; bufs: colour, albedo, normal, variance,
    out, var_out"""
    ffi, L = _lib()
    d = _params() if params is None else params
    pd = None if no_params else C.byref(d)
    res = []
    rc = L.rtmi_denoise_var_device(scene, w, h, bufs[0], bufs[1], bufs[2], bufs[3], pd, bufs[4], bufs[5], None)
    res.append((rc, L.rtmi_last_error()))
    rc = L.rtmi_denoise_var(scene, w, h, bufs[0], bufs[1], bufs[2], bufs[3], pd, bufs[4], bufs[5])
    res.append((rc, L.rtmi_last_error()))
    return res


def test_entry_points_are_exported_and_listed():
    ffi, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name


def test_defaults_are_the_documented_ones():
    d = _params()
    assert (d.iterations, d.flags) == (1, 0)
    assert (d.sigma_color, d.sigma_normal, d.sigma_depth, d.sigma_albedo) == (3.0, 0.5, float(F32(0.1)), INF)
    assert {k: getattr(d, k) for k in DV.DEFAULTS} == {k: (float(F32(v)) if isinstance(v, float) else v) for k, v in DV.DEFAULTS.items()}
    _lib()[1].rtmi_denoise_var_defaults(None)  # tolerated
    from rust_raytrace_amd import raytrace as R
    p = R.HipRayCaster.denoise_var_params()
    assert (p.iterations, p.flags, p.sigma_color, p.sigma_normal) == (1, 0, 3.0, 0.5)
    p = R.HipRayCaster.denoise_var_params(iterations=4, demodulate=True, sigma_color=2.0, sigma_albedo=0.25)
    assert (p.iterations, p.flags, p.sigma_color, p.sigma_albedo) == (4, 1, 2.0, 0.25)


def test_null_scene_params_and_buffers_are_refused():
    for rc, msg in _both(scene=None):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and b"scene" in msg, msg
    for rc, msg in _both(no_params=True):
        assert rc == RTMI_ERR_INVALID and b"NULL" in msg and b"params" in msg, msg
    for k, word in enumerate((b"color", b"albedo", b"normal", b"variance", b"out")):
        bufs = [CO, AL, NO, VA, OUT, VO]
        bufs[k] = None
        for rc, msg in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"NULL" in msg and word in msg, msg
    # var_out is optional: without it the next check that fails is reached
    for rc, msg in _both(bufs=(CO, AL, NO, VA, OUT, None), w=0):
        assert rc == RTMI_ERR_INVALID and b"empty image" in msg, msg


def test_outputs_that_alias_are_refused():
    for k, word in enumerate((b"color", b"albedo", b"normal", b"variance")):
        bufs = [CO, AL, NO, VA, OUT, VO]
        bufs[4] = bufs[k]
        for rc, msg in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"out must not alias" in msg and word in msg, msg
        bufs = [CO, AL, NO, VA, OUT, VO]
        bufs[5] = bufs[k]
        for rc, msg in _both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"var_out must not alias" in msg and word in msg, msg
    for rc, msg in _both(bufs=(CO, AL, NO, VA, OUT, OUT)):
        assert rc == RTMI_ERR_INVALID and b"var_out must not alias out" in msg, msg


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


def _variance_both(bufs=(CO, AL, NO, OUT), n=48, scene=BOGUS):
    ffi, L = _lib()
    res = []
    rc = L.rtmi_variance_device(scene, bufs[0], bufs[1], bufs[2], n, bufs[3], None)
    res.append((rc, L.rtmi_last_error()))
    rc = L.rtmi_variance(scene, bufs[0], bufs[1], bufs[2], n, bufs[3])
    res.append((rc, L.rtmi_last_error()))
    return res


def test_variance_checks_its_arguments_first():
    for rc, msg in _variance_both(scene=None):
        assert rc == RTMI_ERR_INVALID and b"scene" in msg, msg
    for rc, msg in _variance_both(scene=None, n=0):  # the scene comes before the empty set
        assert rc == RTMI_ERR_INVALID and b"scene" in msg, msg
    for k in range(4):
        bufs = [CO, AL, NO, OUT]
        bufs[k] = None
        for rc, msg in _variance_both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"NULL" in msg, msg
        for rc, _ in _variance_both(bufs=bufs, n=0):  # npixels == 0: RTMI_OK, nothing is looked at or touched
            assert rc == RTMI_OK
    for rc, _ in _variance_both(n=0):
        assert rc == RTMI_OK
    for k in range(3):
        bufs = [CO, AL, NO, OUT]
        bufs[3] = bufs[k]
        for rc, msg in _variance_both(bufs=bufs):
            assert rc == RTMI_ERR_INVALID and b"alias" in msg, msg
    ffi, L = _lib()
    assert L.rtmi_variance(BOGUS, CO, AL, NO, 1 << 32, OUT) == RTMI_ERR_UNSUPPORTED and b"2^32" in L.rtmi_last_error()


def test_render_adaptive_denoised_checks_its_arguments_first():
    from test_features_cpu import _vp
    ffi, L = _lib()
    f = L.rtmi_render_adaptive_denoised

    def ad(m=4, p=4):
        return ffi.Adaptive(m, p, 0.01, 0.002)
    vp, d, st = _vp(spp=16), _params(), ffi.Stats()
    st.rays = 123
    assert f(None, C.byref(vp), 1, C.byref(ad()), C.byref(d), OUT, CO, C.byref(st)) == RTMI_ERR_INVALID
    assert b"scene" in L.rtmi_last_error() and st.rays == 0
    assert f(BOGUS, None, 1, C.byref(ad()), C.byref(d), OUT, CO, None) == RTMI_ERR_INVALID and b"viewport" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, None, C.byref(d), OUT, CO, None) == RTMI_ERR_INVALID and b"rtmi_adaptive_t" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, C.byref(ad()), None, OUT, CO, None) == RTMI_ERR_INVALID and b"params" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, C.byref(ad()), C.byref(d), None, CO, None) == RTMI_ERR_INVALID and b"out" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, C.byref(ad()), C.byref(d), OUT, OUT, None) == RTMI_ERR_INVALID and b"alias" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(_vp(w=0, spp=16)), 1, C.byref(ad()), C.byref(d), OUT, None, None) == RTMI_ERR_INVALID
    assert b"empty image" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, C.byref(ad()), C.byref(_params(iterations=9)), OUT, None, None) == RTMI_ERR_INVALID
    assert b"iterations" in L.rtmi_last_error()
    assert f(BOGUS, C.byref(vp), 1, C.byref(ad()), C.byref(_params(sigma_color=NAN)), OUT, None, None) == RTMI_ERR_INVALID
    assert b"sigma_color" in L.rtmi_last_error()
    # the adaptive schedule's errors
    for a, v, word in ((ad(m=1), vp, b"min_samples"), (ad(m=17), vp, b"min_samples"), (ad(p=0), vp, b"pass_samples"),
                       (ad(m=2), _vp(spp=1), b"samples_per_pixel")):
        assert f(BOGUS, C.byref(v), 1, C.byref(a), C.byref(d), OUT, None, None) == RTMI_ERR_INVALID
        assert word in L.rtmi_last_error(), L.rtmi_last_error()
    assert f(BOGUS, C.byref(_vp(spp=16, depth=33)), 1, C.byref(ad()), C.byref(d), OUT, None, None) == RTMI_ERR_UNSUPPORTED
    assert b"maxdepth" in L.rtmi_last_error()


def test_python_api_validates_its_arguments(canonical_pair):
    from rust_raytrace_amd import raytrace as R
    _, sp = canonical_pair
    c = R.HipRayCaster()
    good = np.zeros((6, 8, 4), np.float32)
    cnt = np.full((6, 8), 4, np.uint32)
    with pytest.raises(ValueError):  # no scene yet
        c.denoise_var(good, good.copy(), good.copy(), good.copy())
    with pytest.raises(ValueError):
        c.variance(good, good.copy(), cnt)
    bads = (np.zeros((6, 8, 3), np.float32), np.zeros((8, 6, 4), np.float32), np.zeros((6, 8, 4), np.float64),
            np.zeros((6, 16, 4), np.float32)[:, ::2], np.zeros(192, np.float32), [[0.0]])
    for bad in bads:
        for k in range(6):
            args = [good.copy() for _ in range(6)]
            args[k] = bad
            with pytest.raises(ValueError):
                c.denoise_var(*args, scene=sp)
    for k in range(4):  # out / var_out sharing memory with an input, and with each other
        args = [good.copy() for _ in range(4)]
        with pytest.raises(ValueError):
            c.denoise_var(*args, out=args[k], scene=sp)
        with pytest.raises(ValueError):
            c.denoise_var(*args, var_out=args[k], scene=sp)
    o = good.copy()
    with pytest.raises(ValueError):
        c.denoise_var(good, good.copy(), good.copy(), good.copy(), out=o, var_out=o, scene=sp)
    vp = R.canonical_viewport(8, 6, 5, 16)
    for kw in (dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_normal=NAN), dict(sigma_depth=-1.0),
               dict(sigma_albedo=0.0)):
        with pytest.raises(ValueError):
            c.denoise_var(good, good.copy(), good.copy(), good.copy(), scene=sp, **kw)
        with pytest.raises(ValueError):
            c.denoise_var_device(8, 6, 4096, 8192, 12288, 16384, 20480, scene=sp, **kw)
        with pytest.raises(ValueError):
            c.walk_rays_adaptive_denoised(vp, sp, good.copy(), **kw)
    with pytest.raises(TypeError):
        c.denoise_var(good, good.copy(), good.copy(), good.copy(), scene=sp, sigma=1.0)
    for ptrs in ((0, 8192, 12288, 16384, 20480), (4096, None, 12288, 16384, 20480), (4096, 8192, 12288, 0, 20480),
                 (4096, 8192, 12288, 16384, 0), (4096, 8192, 12288, 16384, 4096), (4096, 8192, 12288, 16384, 16384)):
        with pytest.raises(ValueError):
            c.denoise_var_device(8, 6, *ptrs, scene=sp)
    for vo in (4096, 16384, 20480):
        with pytest.raises(ValueError):
            c.denoise_var_device(8, 6, 4096, 8192, 12288, 16384, 20480, var_out_ptr=vo, scene=sp)
    for w, h in ((0, 6), (8, 0)):
        with pytest.raises(ValueError):
            c.denoise_var_device(w, h, 4096, 8192, 12288, 16384, 20480, scene=sp)
    with pytest.raises(ValueError):
        c.denoise_var_device(8, 6, 4096, 8192, 12288, 16384, 20480)  # no scene
    # variance
    for args in ((bads[0], good.copy(), cnt), (good, bads[2], cnt), (good, good.copy(), cnt.astype(np.int32)),
                 (good, good.copy(), np.zeros((8, 6), np.uint32)), (good, good.copy(), cnt[:, ::2])):
        with pytest.raises(ValueError):
            c.variance(*args, scene=sp)
    with pytest.raises(ValueError):
        c.variance(good, good.copy(), cnt, out=good, scene=sp)
    with pytest.raises(ValueError):
        c.variance(good, good.copy(), cnt, out=np.zeros((6, 8, 3), np.float32), scene=sp)
    for ptrs in ((0, 8192, 12288, 16384), (4096, 8192, 0, 16384), (4096, 8192, 12288, None), (4096, 8192, 12288, 8192)):
        with pytest.raises(ValueError):
            c.variance_device(ptrs[0], ptrs[1], ptrs[2], 48, ptrs[3], scene=sp)
    # the one-call method: data, counts and the adaptive schedule
    for bad in (np.zeros((6, 8, 3), np.float32), np.zeros((6, 8, 4), np.float64), np.zeros((6, 16, 4), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            c.walk_rays_adaptive_denoised(vp, sp, bad)
    with pytest.raises(ValueError):
        c.walk_rays_adaptive_denoised(vp, sp, good.copy(), counts=np.zeros((6, 8), np.int32))
    for kw in (dict(min_samples=1), dict(min_samples=17), dict(pass_samples=0)):
        with pytest.raises(ValueError):
            c.walk_rays_adaptive_denoised(vp, sp, good.copy(), **kw)
    with pytest.raises(ValueError):
        c.walk_rays_adaptive_denoised(R.canonical_viewport(8, 6, 5, 1), sp, good.copy())


# ---------------------------------------------------------------- properties of the restatement
def _guides(h, w, rng, full=True):
    alb = rng.random((h, w, 4), dtype=np.float32)
    alb[..., 3] = 1.0 if full else rng.integers(0, 3, (h, w)).astype(np.float32) * 0.5
    nrm = rng.standard_normal((h, w, 4)).astype(np.float32)
    nrm[..., 3] = 1.0 + rng.random((h, w), dtype=np.float32) * 9.0
    return alb, nrm


def _var(h, w, rng, scale=1e-3):
    v = np.zeros((h, w, 4), np.float32)
    v[..., 0:3] = rng.random((h, w, 3), dtype=np.float32) * F32(scale)
    v[..., 3] = DV.lane_sum(v[..., 0:3])
    return v


@pytest.mark.parametrize("flags", [0, DR.DEMODULATE])
def test_a_constant_image_with_any_finite_variance_is_a_fixed_point(flags):
    """Bit for bit, as for the plain filter: every colour distance is 0 < s2c (>= 2^-40 whatever the variance), so every g is
    exactly 1 and the sums are sums of short dyadic numbers."""
    h, w = 19, 37
    rng = np.random.default_rng(2)
    col = np.zeros((h, w, 4), np.float32)
    col[..., 0:3] = np.array([0.25, 0.5, 0.75], np.float32)
    col[..., 3] = 7.0  # ignored
    alb = np.zeros((h, w, 4), np.float32)
    alb[...] = np.array([0.5 - 1.0 / 256.0, 0.25 - 1.0 / 256.0, 1.0 - 1.0 / 256.0, 1.0], np.float32)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[...] = np.array([0.0, 0.0, -1.0, 4.0], np.float32)
    var = _var(h, w, rng, 10.0)
    var[3, 4] = 0.0
    var[10, 20, 0:3] = 1e30
    var[10, 20, 3] = 3e30
    out, _ = DV.denoise_var_ref(col, alb, nrm, var, iterations=5, flags=flags)
    want = col.copy()
    want[..., 3] = 0.0
    assert_bits_equal(out, want, "constant image")


def test_infinite_variance_is_the_plain_filter_without_its_colour_term():
    """+inf variance makes every colour term exactly 1: the output is denoise_ref's with sigma_color = +inf (whose 4^-i factor
    then changes nothing), and the propagated variance stays +inf."""
    rng = np.random.default_rng(11)
    h, w = 21, 26
    col = rng.random((h, w, 4), dtype=np.float32)
    alb, nrm = _guides(h, w, rng, full=False)
    var = np.full((h, w, 4), np.inf, np.float32)
    for flags in (0, DR.DEMODULATE):
        out, vout = DV.denoise_var_ref(col, alb, nrm, var, iterations=3, flags=flags, sigma_color=2.0, sigma_albedo=0.7)
        want = DR.denoise_ref(col, alb, nrm, iterations=3, flags=flags, sigma_color=INF, sigma_albedo=0.7)
        assert_bits_equal(out, want, "colour with variance +inf")
        assert np.isposinf(vout).all()


def test_zero_variance_leaves_distinct_colours_unchanged():
    """s2c = 2^-40: only the centre tap is added, (w * u) / w with w = 9/64, which is u where 9 u is representable: the
    colours are distinct multiples of 2^-16 below 1."""
    rng = np.random.default_rng(4)
    h, w = 17, 23
    k = rng.permutation(65536)[:h * w * 3].astype(np.float32).reshape(h, w, 3)
    col = np.zeros((h, w, 4), np.float32)
    col[..., 0:3] = k / F32(65536.0)
    alb, nrm = _guides(h, w, rng)
    var = np.zeros((h, w, 4), np.float32)
    out, vout = DV.denoise_var_ref(col, alb, nrm, var, iterations=4, sigma_color=6.0)
    assert_bits_equal(out[..., 0:3], col[..., 0:3], "zero variance")
    assert not vout.any()


def test_a_nan_variance_freezes_its_3x3_neighbourhood_and_poisons_no_colour():
    rng = np.random.default_rng(5)
    h, w = 24, 31
    col = rng.random((h, w, 4), dtype=np.float32)
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., 0:3] = 0.5
    alb[..., 3] = 1.0
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[...] = np.array([0.0, 0.0, -1.0, 4.0], np.float32)
    var = np.zeros((h, w, 4), np.float32)
    var[..., 0:3] = 1.0  # wide enough for every pair of colours to mix
    var[..., 3] = 3.0
    var[7, 9] = np.nan
    var[0, 30, 3] = np.nan  # lane 3 alone, in a corner
    out, vout = DV.denoise_var_ref(col, alb, nrm, var, iterations=1)
    frozen = np.zeros((h, w), bool)
    frozen[6:9, 8:11] = True
    frozen[0:2, 29:31] = True
    wgt = F32(0.140625)
    centre_only = (wgt * col[..., 0:3]) / wgt
    same = (out[..., 0:3].view(np.uint32) == centre_only.view(np.uint32)).all(axis=2)
    assert np.array_equal(same, frozen), np.argwhere(same != frozen)
    assert np.isfinite(out).all()
    assert np.isnan(vout[7, 9, 0:3]).all() and np.isnan(vout[5, 9, 0]) and not np.isnan(vout[0, 29]).any()
    for it in (2, 4):  # the NaN spreads through the variance, never into a colour
        out, _ = DV.denoise_var_ref(col, alb, nrm, var, iterations=it)
        assert np.isfinite(out).all()


def test_propagated_variance_is_sum_w2_v_over_sum_w_squared():
    """Full coverage, constant guides, all sigmas +inf and a finite positive variance: every weight is k[dy] * k[dx], so one
    iteration's variance is sum(w^2 v) / sum(w)^2 over the taps inside the image.  Computed independently in float64; the f32
    result differs by the roundings of 25 products and additions of positive terms, the square and one division: each
    result within (25 + 3) * 2^-24 relative, asserted with 32 * 2^-24."""
    rng = np.random.default_rng(9)
    h, w = 13, 18
    col = rng.random((h, w, 4), dtype=np.float32)
    alb = np.ones((h, w, 4), np.float32)
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[...] = np.array([0.0, 1.0, 0.0, 2.0], np.float32)
    var = _var(h, w, rng) + F32(1e-6)
    var[..., 3] = DV.lane_sum(var[..., 0:3])
    _, vout = DV.denoise_var_ref(col, alb, nrm, var, iterations=1, sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    k = DR.K.astype(np.float64)
    v64 = var[..., 0:3].astype(np.float64)
    want = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            sw, swv = 0.0, np.zeros(3)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        wt = k[dy + 2] * k[dx + 2]
                        sw += wt
                        swv += wt * wt * v64[y + dy, x + dx]
            want[y, x] = swv / (sw * sw)
    rel = np.abs(vout[..., 0:3].astype(np.float64) - want) / want
    assert rel.max() <= 32 * 2.0 ** -24, rel.max()
    assert_bits_equal(vout[..., 3], DV.lane_sum(vout[..., 0:3]), "lane 3")
    assert (vout[2:-2, 2:-2, 0:3] < var[2:-2, 2:-2, 0:3].max()).all()  # and it shrinks


def test_variance_agrees_with_the_stop_rule():
    """max(vm_r, vm_g, vm_b) is the stop rule's e (the division by n is monotonic, and the clamp at 0 cannot change a
    comparison with t * t >= 0): with rel_tol = 0 the rule of tests/test_adaptive.py stops exactly where it is <= abs_tol^2."""
    from test_adaptive import stop_rule
    rng = np.random.default_rng(21)
    n = 9
    smp = rng.random((n, 4000, 4), dtype=np.float32) * rng.random((1, 4000, 1), dtype=np.float32)
    smp[:, :500] = smp[0:1, :500]  # constant pixels: v is 0 or a rounding error of either sign
    s = np.zeros((4000, 4), np.float32)
    q = np.zeros((4000, 4), np.float32)
    for k in range(n):
        s = s + smp[k]
        q = q + smp[k] * smp[k]
    var = DV.variance_ref(s, q, np.full(4000, n, np.uint32))
    assert (var[..., 0:3] >= 0).all()
    e = var[..., 0:3].max(axis=1)
    # the same e, written as the stop rule writes it
    f = np.float32
    inv = f(1) / f(n)
    m = s[..., :3] * inv
    v = (q[..., :3] - s[..., :3] * m) / f(n - 1)
    e_rule = v.max(axis=1) / f(n)
    assert_bits_equal(e, np.where(e_rule < 0, f(0), e_rule), "e")
    for ab in [0.0] + [float(np.sqrt(x)) for x in np.quantile(e, [0.1, 0.5, 0.9])] + [float(np.sqrt(e[1234]))]:
        t = f(ab)
        assert np.array_equal(stop_rule(s, q, n, 0.0, ab), e <= t * t), ab
    assert_bits_equal(var[..., 3], DV.lane_sum(var[..., 0:3]), "lane 3")


def test_variance_of_fewer_than_two_samples_is_infinite_and_nan_stays():
    s = np.array([[1.0, 2.0, 3.0, 0.0]] * 5, np.float32)
    q = np.array([[1.0, 4.0, 9.0, 0.0]] * 5, np.float32)
    s[4, 1] = np.nan
    var = DV.variance_ref(s, q, np.array([0, 1, 2, 3, 2], np.uint32))
    assert np.isposinf(var[0:2]).all()
    assert np.isfinite(var[2:4]).all() and (var[2:4] >= 0).all()
    assert np.isnan(var[4, 1]) and np.isnan(var[4, 3]) and np.isfinite(var[4, 0]) and np.isfinite(var[4, 2])


# ---------------------------------------------------------------- quality, with the oracle only
def _rmse(a, b):
    d = a[..., 0:3].astype(np.float64) - b[..., 0:3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


@pytest.fixture(scope="module")
def quality_scenes():
    """Per scene: the truth (256 spp, seed 7), the guides of seed 100 and sixteen 2-spp renders of seeds 100 .. 115, the
    "samples" of the frames below (the oracle has no per-sample output)."""
    from oracle import orc
    w = h = 96
    vp = orc.canonical_viewport(w, h)
    res = {}
    for name, recipe in (("canonical", recipe_canonical(maxdepth=8)), ("circles", recipe_circles())):
        so = recipe(OracleApi(orc))
        truth, _ = so.render(w, h, vp, 5, 256, seed=7, threads=8)
        alb, nrm, _, _ = FR.features_ref(orc, so, w, h, vp, 2, 100)
        smp = [so.render(w, h, vp, 5, 2, seed=100 + k, threads=8)[0] for k in range(16)]
        res[name] = (truth, alb, nrm, smp)
    return w, h, res


@pytest.mark.parametrize("scene", ["canonical", "circles"])
@pytest.mark.parametrize("K", [4, 8, 16])
def test_the_default_filter_lowers_the_error_where_the_plain_filter_raises_it(quality_scenes, scene, K):
    """RMSE over rgb against the truth of a frame of K samples per pixel, of the plain filter at its defaults and of the
    variance-guided filter at its defaults (sigma_color 3, 1 iteration).  Measured, input / plain / guided:
    canonical K = 4 0.0279 / 0.0249 / 0.0236, 8 0.0208 / 0.0239 / 0.0183, 16 0.0154 / 0.0220 / 0.0139; circles K = 4 0.0188 /
    0.0222 / 0.0185, 8 0.0135 / 0.0201 / 0.0131, 16 0.0093 / 0.0181 / 0.0089.  Asserted: guided < input in all six, and guided
    < plain for K >= 8; the K = 4 comparison with the plain filter is printed only."""
    w, h, res = quality_scenes
    truth, alb, nrm, smp = res[scene]
    acc = np.zeros((h, w, 4), np.float32)
    sq = np.zeros((h, w, 4), np.float32)
    for k in range(K):
        acc = acc + smp[k]
        sq = sq + smp[k] * smp[k]
    col = acc * (F32(1.0) / F32(K))
    var = DV.variance_ref(acc, sq, np.full((h, w), K, np.uint32))
    out, _ = DV.denoise_var_ref(col, alb, nrm, var, **DV.DEFAULTS)
    plain = DR.denoise_ref(col, alb, nrm, **DR.DEFAULTS)
    before, after, shipped = _rmse(col, truth), _rmse(out, truth), _rmse(plain, truth)
    print(f"{scene} K = {K}: RMSE input {before:.4f}, plain filter {shipped:.4f}, variance-guided {after:.4f}")
    assert after < before
    if K >= 8:
        assert after < shipped
