"""-m gpu: the environment of a scene (rtmi_scene_set_environment / rtmi_scene_set_sky, include/rtmi.h) through every call that gains
it, every float bit for bit against tests/env_ref.py, the float32 NumPy restatement of the header on the oracle's closest hits,
records and RNG (tests/test_env_cpu.py pins it), so no expected value comes from the code under test.  RTMI_OPT_BVH, RTMI_OPT_FAST and
analytic spheres are held against the restatement fed by the product's own rtmi_trace, as in tests/test_glass.py, whose cases these
are.  Scenes: tests/glass_cases.py and the canonical scene.  The references are computed once per case and shared."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import camera_ref as CR
import env_ref as ER
import features_ref as FR
import glass_cases as GC
import rays_ref as RR

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = GC.VIEW["w"], GC.VIEW["h"]
SPP, SEED, MAXDEPTH = 4, 5, 6
# a sun 37 degrees wide, low on the -x side of the canonical camera (which looks down +z): one half of every image is the lit one
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _rotation():
    a, b = 0.7, -0.4
    ra = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rb = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (ra @ rb).astype(F32)


def _hdr(n):
    """A random HDR table, values up to 1e4"""
    return (np.random.default_rng(100 + n).random((n, n, 3)) ** 4 * 1e4).astype(F32)


def _sky_env(n=8, sky=SUN):
    return SimpleNamespace(table=ER.sky_table(n, sky), frame=None)


@pytest.fixture(scope="module")
def slab():
    """The glass slab under a random HDR table of 3 x 3 texels in a rotated frame"""
    so, sp = GC.build_pair(GC.recipe_slab())
    env = SimpleNamespace(table=_hdr(3), frame=_rotation())
    sp.set_environment(env.table, env.frame)
    return so, sp, env


@pytest.fixture(scope="module")
def teapot():
    """The canonical Matte / Reflective scene under the generated sky with the sun on one side"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_sky(8, **SUN)
    return so, sp, _sky_env()


def _ref(so, env, spp=SPP, maxdepth=MAXDEPTH, vp12=None, w=W, h=H, seed=SEED, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    vo = _orc().canonical_viewport(w, h) if vp12 is None else vp12
    key = (id(so), id(env), spp, maxdepth, tuple(np.asarray(vo, F32).tolist()), w, h, seed,
           tuple(sorted((k, str(v)) for k, v in kw.items() if k != "trace")), id(kw.get("trace")))
    if key not in _REFS:
        _REFS[key] = ER.render(_orc(), so, vo, w, h, spp, seed, maxdepth, env=env, **kw)
    return _REFS[key]


def _vp(spp=SPP, maxdepth=MAXDEPTH, w=W, h=H):
    return _R().canonical_viewport(w, h, maxdepth, spp)


def _render(sp, vp, seed=SEED, **caster):
    img = np.full((vp.height, vp.width, 4), -7.0, F32)
    ctx = _R().HipRayCaster(seed=seed, **caster).walk_rays(vp, sp, img)
    return img, ctx


def _assert_env_stats(ctx, ref):
    assert ctx.stats["rays"] == ref.rays, (ctx.stats["rays"], ref.rays)
    assert ctx.stats["pipeline"] == 1 and ctx.stats["slow_paths"] == 0


# ---------------------------------------------------------------- the lookup alone
def _lookup_dirs():
    """Unit directions: the axes, zero-component and near-axis ones, both sides of m.z = 0 and of every fold edge, the
    neighbourhood of the -z pole, 256 random ones"""
    e = 1e-4
    rows = []
    for k in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[k] = s
            rows.append(v)
            for j in range(3):
                if j != k:
                    for t in (e, -e, 1e-30):
                        u = list(v)
                        u[j] = t
                        rows.append(u)
    rows += [[1, 1, 0], [1, -1, 0], [0, 1, 1], [0, 1, -1], [1, 0, -1], [-1, 0, -1], [0, -1, -1], [-1, 1, 0]]
    for a in np.linspace(0, 2 * np.pi, 24, endpoint=False):
        rows += [[np.cos(a), np.sin(a), e], [np.cos(a), np.sin(a), -e]]                      # m.z = 0
        rows += [[e * np.cos(a), e * np.sin(a), -1.0], [0.3 * np.cos(a), 0.3 * np.sin(a), -1.0]]  # around the -z pole
    for u in np.linspace(0.1, 0.9, 9):
        z = -np.sqrt(1 - u * u)
        for s in (1.0, -1.0):
            rows += [[s * u, e, z], [s * u, -e, z], [e, s * u, z], [-e, s * u, z], [s * u, 0.0, z], [0.0, s * u, z]]  # the fold edges
    d = np.zeros((len(rows) + 256, 4), F32)
    d[:len(rows), :3] = np.array(rows, np.float64)
    d[len(rows):, :3] = np.random.default_rng(7).normal(size=(256, 3))
    return RR.vunit(d)


def _recipe_tilted(accel):
    """Two tilted triangles around the origin.  No plane of the scene is parallel to an axis: the reference calls a ray that is
    parallel to a triangle's plane a hit at t = inf, and the rays of the lookup test must be misses."""
    def r(api):
        s = api.scene()
        api.add_triangle(s, np.array([[-1.0, -0.7, 0.3], [1.1, -0.2, -0.6], [0.2, 0.9, 0.8]], F32), api.matte((200, 100, 50), 0.5), 0.0)
        api.add_triangle(s, np.array([[-0.9, 0.6, -0.5], [0.4, -1.0, 0.7], [0.8, 0.7, -0.9]], F32), api.solid((20, 100, 250)), 0.02)
        s.populate_triangle_numbers()
        if accel == "octree":
            s.build_bounding_box([0.0, 0.0, 0.0], 2.0, 2, 1)
        else:
            s.build_trivial_bounding_box([0.0, 0.0, 0.0], 4.0)
        return s
    return r


@pytest.mark.parametrize("frame", ["identity", "rotated"])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_a_ray_that_leaves_the_scene_returns_the_lookup(n, frame):
    so, sp = CT.build_pair(_recipe_tilted("trivial" if n == 2 else "octree"))
    table, fr = _hdr(n), (None if frame == "identity" else _rotation())
    sp.set_environment(table, fr)
    d = _lookup_dirs()
    o = (d * F32(100.0)).astype(F32)  # far outside the scene, pointing away from it
    tri = _orc_trace(so, o, d)
    assert not tri.any()
    want = ER.lookup(table, fr, d)
    assert np.isfinite(want).all() and want.max() > 100.0 and (want[:, 3] == 0).all()
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o, d, 1)
    assert_bits_equal(got["color"], want, f"lookup, n = {n}, {frame} frame")
    assert ctx.stats["rays"] == len(d) and ctx.stats["pipeline"] == 1


def _orc_trace(so, o, d):
    return np.asarray(so.trace(o, d)[0])


# ---------------------------------------------------------------- the generated sky
def test_generated_sky_set_replace_clear():
    R = _R()
    so, sp = GC.build_pair(GC.recipe_slab())
    c = R.HipRayCaster(seed=SEED)
    assert c.environment(sp) is None
    for n, sky in ((3, SUN), (8, dict(SUN, up=(0.0, 0.0, 2.0), ground=(0.5, 0.25, 0.125))), (1, {})):
        sp.set_sky(n, **sky)
        got = c.environment(sp)
        assert got.shape == (n, n, 3)
        assert_bits_equal(got, ER.sky_table(n, sky), f"k_env_sky, n = {n}")
    assert (ER.sky_table(8, SUN) > 10).any()  # the sun is on the table
    table = _hdr(2)
    sp.set_environment(table)  # a generated table replaced by a given one
    assert_bits_equal(c.environment(sp), table, "the table read back")
    sp.clear_environment()
    assert c.environment(sp) is None
    ref = ER.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 1, SEED, 3)
    img, ctx = _render(sp, _vp(1, 3))
    assert_bits_equal(img, ref.image, "after clear_environment: the sky constant")


# ---------------------------------------------------------------- frames
def test_slab_host_variant(slab):
    so, sp, env = slab
    ref = _ref(so, env)
    assert ref.pt.total["refract_in"] >= 1 and ref.pt.total["refract_out"] >= 1 and (ref.pt.hits0[0] == 0).any()
    assert ref.image.max() > 2.0  # HDR texels reach the image
    img, ctx = _render(sp, _vp())
    assert_bits_equal(img, ref.image, "slab, rtmi_render")
    _assert_env_stats(ctx, ref)
    assert ctx.stats["trace_launches"] == MAXDEPTH


def test_canonical_scene_lit_from_one_side(teapot):
    so, sp, env = teapot
    ref = _ref(so, env, spp=2, maxdepth=5)
    # the restatement, on the CPU: the half of the image whose rays point to the sun's side is the brighter one
    dx = ref.d4[:, 0].reshape(H, W, 2).mean(axis=(0, 2))
    left_is_sunny = dx[:W // 2].mean() < dx[W // 2:].mean()  # the sun is at -x
    lum = ref.image[..., :3].astype(np.float64).sum(axis=-1)
    sunny, other = (lum[:, :W // 2], lum[:, W // 2:]) if left_is_sunny else (lum[:, W // 2:], lum[:, :W // 2])
    assert sunny.mean() > 1.25 * other.mean(), (sunny.mean(), other.mean())
    plain = ER.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5)
    assert (plain.image != ref.image).mean() > 0.5 and plain.rays == ref.rays  # the environment moves colours, not rays
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, ref.image, "canonical scene under the sky")
    _assert_env_stats(ctx, ref)


def test_device_variant_on_a_striped_tile(slab):
    import torch
    so, sp, env = slab
    tile = (1, 12, 3, 8)  # rows 1-3, 9-11, 17-19, 25-27
    ref = _ref(so, env, tile=tile)
    buf = torch.full((12 * W * 4 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _R().HipRayCaster(seed=SEED).walk_tile_device(_vp(), sp, tile, buf[64:].data_ptr())
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:64] == 7.5).all() and (g[64 + 12 * W * 4:] == 7.5).all()
    assert_bits_equal(g[64:64 + 12 * W * 4].reshape(12, W, 4), ref.image, "slab, striped tile")
    _assert_env_stats(ctx, ref)


# ---------------------------------------------------------------- one path loop under every sampling mode
def test_progressive_passes_end_in_the_bits_of_one_call(slab):
    so, sp, env = slab
    ref = _ref(so, env)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_progressive(_vp(), sp, img, pass_samples=1)
    assert_bits_equal(img, ref.image, "four passes of one sample")
    assert ctx.samples_done == SPP and ctx.total_rays == ref.rays and ctx.stats["pipeline"] == 1


def test_adaptive_without_a_tolerance_is_the_uniform_render(slab):
    so, sp, env = slab
    ref = _ref(so, env)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_adaptive(_vp(), sp, img, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(img, ref.image, "adaptive, abs_tol = NaN")
    assert (ctx.counts == SPP).all() and ctx.total_rays == ref.rays


def test_views_of_two_cameras_with_two_seeds(slab):
    R = _R()
    so, sp, env = slab
    vs = GC.side_viewport(_orc(), W, H)
    views = [_vp(), R.Viewport(W, H, vs, MAXDEPTH, SPP)]
    ctx = R.HipRayCaster(seed=SEED).walk_rays_views(views, sp, seeds=[SEED, SEED + 1])
    assert_bits_equal(ctx.data[0], _ref(so, env).image, "view 0")
    assert_bits_equal(ctx.data[1], _ref(so, env, vp12=vs, seed=SEED + 1).image, "view 1")
    assert ctx.stats["pipeline"] == 1


def test_explicit_rays_of_the_camera_with_their_keys_equal_the_render(slab):
    import torch
    so, sp, env = slab
    ref = _ref(so, env)
    n = len(ref.o4)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to("cuda:0").contiguous()
    o4, d4 = dev(ref.o4, torch.float32), dev(ref.d4, torch.float32)
    keys = dev(np.stack([ref.pixel, ref.sample], axis=1).astype(np.int32), torch.int32)
    color = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    mean = torch.zeros(n // SPP * 4, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit_device(sp, o4, d4, MAXDEPTH, group=SPP, keys=keys, color=color, mean=mean)
    torch.cuda.synchronize()
    assert_bits_equal(color.cpu().numpy().reshape(n, 4), ref.color, "sample colours")
    assert_bits_equal(mean.cpu().numpy().reshape(H, W, 4), ref.image, "group means")
    _assert_env_stats(ctx, ref)


def test_bake_light_is_the_restatements_fold_and_open_is_unchanged(slab):
    orc = _orc()
    so, sp, env = slab
    c = _R().HipRayCaster(seed=SEED)
    # on the slab's front face, on the floor below it, and inside the glass looking out through the back face
    pos = np.array([[0.0, 0.3, 4.0, 0], [-1.0, -2.6, 3.0, 0], [0.2, -0.5, 4.1, 0]], F32)
    nrm = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
    K, depth, pixel0 = 32, 5, 7
    params = c.bake_params("points", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = c.bake(sp, pos, nrm, params, light=True, open=True, orig=True, dir=True)
    pt = ER.path_trace(orc, so, got["orig"], got["dir"], pixel0 + np.repeat(np.arange(3), K), np.tile(np.arange(K), 3), depth, SEED, env=env)
    assert_bits_equal(got["light"], RR.fold(pt.color, K), "bake against the restatement")
    assert ctx.total_rays == pt.rays and ctx.stats["pipeline"] == 1 and (pt.hits0[0] == 0).any()
    try:
        sp.clear_environment()
        plain, _ = c.bake(sp, pos, nrm, params, light=True, open=True)
    finally:
        sp.set_environment(env.table, env.frame)
    assert_bits_equal(got["open"], plain["open"], "open does not look at the environment")
    assert (got["light"] != plain["light"]).any()


def test_thin_lens_camera(slab):
    from rust_raytrace_amd import _ffi
    orc = _orc()
    so, sp, env = slab
    cr = CR.camera_rays(orc, orc.canonical_viewport(W, H), W, H, 2, SEED, CR.cam(CR.THIN_LENS, 0.05, 4.0))
    pt = ER.path_trace(orc, so, cr.o4, cr.d4, cr.keys[:, 0], cr.keys[:, 1], 5, SEED, env=env)
    acc, want = CR.fold(pt.color, cr.npix, cr.n)
    accum, img = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_samples_camera(_vp(2, 5), sp, 0, H, _ffi.Camera(CR.THIN_LENS, 0, 0.05, 4.0), 0, 2, accum, img)
    assert_bits_equal(img, want.reshape(H, W, 4), "thin lens: out")
    assert_bits_equal(accum, acc.reshape(H, W, 4), "thin lens: accum")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- scene kinds
def test_linear_list_scene():
    so, sp = GC.build_pair(GC.recipe_slab(accel="trivial"))
    env = _sky_env(3)
    sp.set_sky(3, **SUN)
    ref = _ref(so, env, spp=2, maxdepth=5)
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, ref.image, "linear list")
    _assert_env_stats(ctx, ref)


def test_generic_tree(slab):
    so, sp, env = slab
    ref = _ref(so, env, spp=2, maxdepth=5)
    img, ctx = _render(sp, _vp(2, 5), options=_R().OPT_GENERIC)
    assert_bits_equal(img, ref.image, "RTMI_OPT_GENERIC")
    _assert_env_stats(ctx, ref)


@pytest.mark.parametrize("option", ["OPT_BVH", "OPT_FAST"])
def test_bvh_and_fast_against_their_own_trace(slab, option):
    R = _R()
    so, sp, env = slab
    caster = R.HipRayCaster(seed=SEED, options=getattr(R, option))
    ref = ER.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3], env=env)
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, option)
    _assert_env_stats(ctx, ref)
    assert (ref.pt.hits0[0] == 0).any()


def test_analytic_sphere():
    R, orc = _R(), _orc()
    so, sp = GC.build_pair(GC.recipe_sphere())
    env = SimpleNamespace(table=_hdr(8), frame=None)
    sp.set_environment(env.table)
    caster = R.HipRayCaster(seed=SEED)
    ref = ER.render(orc, so, orc.canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3],
                    spheres=GC.sphere_table(orc), env=env)
    assert ref.pt.total["refract_in"] >= 1 and (ref.pt.hits0[0] == 0).any()
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, "analytic glass sphere under an environment")
    _assert_env_stats(ctx, ref)


# ---------------------------------------------------------------- tuning, depth
@pytest.mark.parametrize("tuning", [dict(streams=3, batch_paths=600, subtile_min_paths=1), dict(streams=1, batch_paths=500)])
def test_tuning_changes_no_bit(slab, tuning):
    so, sp, env = slab
    ref = _ref(so, env)
    img, ctx = _render(sp, _vp(), tuning=tuning)
    assert_bits_equal(img, ref.image, f"tuning {tuning}")
    _assert_env_stats(ctx, ref)


@pytest.mark.parametrize("maxdepth", [0, 1, 2])
def test_shallow_depths(teapot, maxdepth):
    so, sp, env = teapot
    ref = _ref(so, env, spp=2, maxdepth=maxdepth)
    img, ctx = _render(sp, _vp(2, maxdepth))
    assert_bits_equal(img, ref.image, f"maxdepth {maxdepth}")
    assert ctx.stats["rays"] == ref.rays
    if maxdepth == 0:
        assert not img.any()


# ---------------------------------------------------------------- refusals, and the way back to the old path
def test_shadowed_refuses_an_environment_and_the_handle_stays_usable(teapot):
    so, sp, env = teapot
    c = _R().HipRayCaster(seed=SEED)
    ref = _ref(so, env, spp=2, maxdepth=5)
    img, _ = _render(sp, _vp(2, 5))  # the scene is on the device
    with pytest.raises(RuntimeError, match="environment"):
        c.walk_rays_shadowed(_vp(2, 5), sp, orig=(2.0, 3.0, 0.0))
    again, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(again, ref.image, "after the refusal")
    _assert_env_stats(ctx, ref)


def test_bad_arguments_are_refused_by_the_abi():
    import test_gpu_abi_raw as RAW
    from rust_raytrace_amd import _ffi
    L, ffi = RAW._lib()
    so = CT.recipe_axis_box()(CT.OracleApi(_orc()))
    tris, geo, topo, refs = RAW._abi_arrays(so)
    rc, h = RAW._create(L, tris, RAW._boxes(geo, topo), refs)
    assert rc == RAW.RTMI_OK
    try:
        rgb = _hdr(2)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        n = C.c_uint32(9)
        assert L.rtmi_scene_set_environment(h, p(rgb), 4097, None) == RAW.RTMI_ERR_INVALID
        e = _ffi.Environment()
        L.rtmi_environment_defaults(C.byref(e))
        e.frame[4] = float("nan")
        assert L.rtmi_scene_set_environment(h, p(rgb), 2, C.byref(e)) == RAW.RTMI_ERR_INVALID and b"frame" in L.rtmi_last_error()
        e.frame[4] = float("inf")
        assert L.rtmi_scene_set_environment(h, p(rgb), 2, C.byref(e)) == RAW.RTMI_ERR_INVALID
        k = _ffi.Sky()
        L.rtmi_sky_defaults(C.byref(k))
        assert L.rtmi_scene_set_sky(h, 0, C.byref(k)) == RAW.RTMI_ERR_INVALID and L.rtmi_scene_set_sky(h, 4097, C.byref(k)) == RAW.RTMI_ERR_INVALID
        k.sun_dir[:] = [0.0, 0.0, 0.0]
        assert L.rtmi_scene_set_sky(h, 4, C.byref(k)) == RAW.RTMI_ERR_INVALID and b"sun_dir" in L.rtmi_last_error()
        L.rtmi_sky_defaults(C.byref(k))
        k.up[:] = [0.0, float("nan"), 0.0]
        assert L.rtmi_scene_set_sky(h, 4, C.byref(k)) == RAW.RTMI_ERR_INVALID
        assert L.rtmi_scene_get_environment(h, None, C.byref(n)) == RAW.RTMI_OK and n.value == 0  # none of them left anything behind
        # set, read back, remove through the raw ABI
        assert L.rtmi_scene_set_environment(h, p(rgb), 2, None) == RAW.RTMI_OK, L.rtmi_last_error()
        back = np.zeros((2, 2, 3), F32)
        assert L.rtmi_scene_get_environment(h, p(back), C.byref(n)) == RAW.RTMI_OK and n.value == 2
        assert_bits_equal(back, rgb, "rtmi_scene_get_environment")
        w = 8
        vo = _orc().canonical_viewport(w, w)
        lit, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        assert_bits_equal(lit, ER.render(_orc(), so, vo, w, w, 1, SEED, 3, env=SimpleNamespace(table=rgb, frame=None)).image, "raw ABI, lit")
        assert st.pipeline == 1
        assert L.rtmi_scene_set_environment(h, None, 2, None) == RAW.RTMI_OK
        assert L.rtmi_scene_get_environment(h, None, C.byref(n)) == RAW.RTMI_OK and n.value == 0
        plain, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        want, _ = so.render(w, w, vo, 3, 1, seed=SEED, threads=2)
        assert_bits_equal(plain, want, "raw ABI, the environment removed")
    finally:
        L.rtmi_scene_destroy(h)


def test_after_clear_environment_the_canonical_scene_is_the_oracles_again(teapot):
    orc = _orc()
    so, sp, env = teapot
    want, cn = so.render(W, H, orc.canonical_viewport(W, H), 5, 2, seed=SEED, threads=4)
    try:
        sp.clear_environment()
        img, ctx = _render(sp, _vp(2, 5))
    finally:
        sp.set_sky(8, **SUN)
    assert_bits_equal(img, want, "canonical scene, environment cleared")
    assert ctx.stats["pipeline"] == 3 and ctx.stats["rays"] == cn["rays"]
    again, ctx = _render(sp, _vp(2, 5))  # and back
    assert_bits_equal(again, _ref(so, env, spp=2, maxdepth=5).image, "the sky set again")
    assert ctx.stats["pipeline"] == 1


def test_first_hit_calls_are_unchanged(teapot):
    so, sp, env = teapot
    alb, nrm, ids, _ = FR.features_ref(_orc(), so, W, H, _orc().canonical_viewport(W, H), 2, SEED)
    a, n, i, ctx = _R().HipRayCaster(seed=SEED).walk_rays_features(_vp(2, 5), sp)
    assert_bits_equal(a, alb, "albedo")
    assert_bits_equal(n, nrm, "normal")
    assert np.array_equal(i, ids)
    clear = a[..., 3] == 0  # pixels all of whose samples miss: the documented sky constant, not the environment
    assert clear.any() and (ids[clear] == 0).all() and (a[clear][:, :3] == FR.SKY).all()
