"""-m gpu: the vertex normals of a scene (rtmi_scene_set_normals / rtmi_smooth_normals, include/rtmi.h) through every call that
gains them, every float bit for bit against tests/smooth_ref.py, the float32 NumPy restatement of the header on the oracle's
closest hits, records and RNG (tests/test_smooth_cpu.py pins it), so no expected value comes from the code under test: the
generated normals of a case are smooth_ref.generate's on the oracle's records, and the device's table is held against them.
RTMI_OPT_BVH, RTMI_OPT_FAST and analytic spheres are held against the restatement fed by the product's own rtmi_trace, as in
tests/test_glass.py and tests/test_env.py, whose matrix this is.  Scenes: tests/smooth_cases.py's patch, tests/glass_cases.py's
slab and the canonical scene, 32 x 32, spp 4, depth <= 6.  The references are computed once per case and shared."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import camera_ref as CR
import env_ref as ER
import glass_cases as GC
import rays_ref as RR
import smooth_cases as SC
import smooth_ref as SR

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = GC.VIEW["w"], GC.VIEW["h"]
SPP, SEED, MAXDEPTH = 4, 5, 6
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _generated(so, first, count, crease_cos):
    """The normals Scene.smooth_normals(first, count, crease_cos) must produce, from the oracle's records: (ntris, 3, 3)"""
    rec = so.triangles()[0]
    out = np.zeros((len(rec), 3, 3), F32)
    out[first:first + count] = SR.generate(rec[first:first + count, 20:29], rec[first:first + count, 3:6], crease_cos)
    return out


@pytest.fixture(scope="module")
def teapot():
    """The canonical Matte / Reflective scene, the teapot with generated normals"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.smooth_normals(1, NTEAPOT)
    return so, sp, _generated(so, 1, NTEAPOT, 0.5)


@pytest.fixture(scope="module")
def slab():
    """The glass slab, its box with the normals of crease_cos = -1: every corner's is the mean of its three faces', 55 degrees
    off each of them"""
    so, sp = GC.build_pair(GC.recipe_slab())
    sp.smooth_normals(1, 12, crease_cos=-1.0)
    return so, sp, _generated(so, 1, 12, -1.0)


@pytest.fixture(scope="module")
def patch():
    so, sp = GC.build_pair(SC.recipe_patch())
    nrm = SC.patch_normals(so.triangles()[0])
    sp.set_vertex_normals(nrm[1:])
    o4, d4 = SC.patch_rays()
    return so, sp, nrm, o4, d4


def _ref(so, normals, spp=SPP, maxdepth=MAXDEPTH, vp12=None, w=W, h=H, seed=SEED, env=None, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    vo = _orc().canonical_viewport(w, h) if vp12 is None else vp12
    key = (id(so), id(normals), id(env), spp, maxdepth, tuple(np.asarray(vo, F32).tolist()), w, h, seed,
           tuple(sorted((k, str(v)) for k, v in kw.items() if k != "trace")), id(kw.get("trace")))
    if key not in _REFS:
        _REFS[key] = SR.render(_orc(), so, vo, w, h, spp, seed, maxdepth, env=env, normals=normals, **kw)
    return _REFS[key]


def _vp(spp=SPP, maxdepth=MAXDEPTH, w=W, h=H):
    return _R().canonical_viewport(w, h, maxdepth, spp)


def _render(sp, vp, seed=SEED, **caster):
    img = np.full((vp.height, vp.width, 4), -7.0, F32)
    ctx = _R().HipRayCaster(seed=seed, **caster).walk_rays(vp, sp, img)
    return img, ctx


def _assert_stats(ctx, ref):
    assert ctx.stats["rays"] == ref.rays, (ctx.stats["rays"], ref.rays)
    assert ctx.stats["pipeline"] == 1 and ctx.stats["slow_paths"] == 0


# ---------------------------------------------------------------- the normal alone
def test_the_normal_alone_on_explicit_rays_with_guides(patch):
    so, sp, nrm, o4, d4 = patch
    hn = SR.hit_normals(so, nrm, o4, d4)
    # a condition on the inputs (tests/test_smooth_cpu.py verifies it without a GPU): every branch of `use` runs in this set
    assert hn.use.sum() >= 100 and hn.flat.sum() >= 50 and hn.away_from_ng.sum() >= 20 and hn.away_from_ray.sum() >= 50
    assert ((hn.face & 1) != 0).sum() >= 100 and (hn.tri == 0).any()
    alb, want, ids = SR.features(_orc(), so, nrm, 0, 0, None, 1, SEED, rays=(o4, d4, len(o4), 1))
    assert (want[hn.use][:, :3] != hn.ng[hn.use][:, :3]).any(axis=1).all()  # where `use` holds the guide is not the flat one
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o4, d4, 1, color=True, albedo=True, normal=True, ids=True)
    assert_bits_equal(got["normal"], want, "the normal guide of the patch")
    assert_bits_equal(got["albedo"], alb, "albedo")
    assert np.array_equal(got["ids"], ids)
    pt = SR.path_trace(_orc(), so, o4, d4, np.arange(len(o4)), np.zeros(len(o4), np.int64), 1, SEED, normals=nrm)
    assert_bits_equal(got["color"], pt.color, "depth 1: nothing bounces, the colours are the flat ones")
    assert ctx.stats["rays"] == len(o4) and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- the bounce
def test_the_bounce_and_its_fallback_per_kind(patch):
    so, sp, nrm, o4, d4 = patch
    n = len(o4)
    pt = SR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, SEED, normals=nrm)
    c = pt.smooth
    assert c["smooth"] >= 100 and c["flat"] >= 100 and c["away_from_ng"] >= 20 and c["away_from_ray"] >= 50, c
    assert min(c["fallback_matte"], c["fallback_reflective"], c["fallback_glass_reflect"], c["fallback_glass_refract"]) >= 1, c
    flat = SR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, SEED)
    assert (flat.color != pt.color).any(axis=1).sum() >= 100  # the normals move the paths
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o4, d4, 3)
    assert_bits_equal(got["color"], pt.color, "the patch at depth 3")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- the teapot, generated normals
def test_teapot_host_variant_and_the_table_read_back(teapot):
    so, sp, nrm = teapot
    c = _R().HipRayCaster(seed=SEED)
    assert_bits_equal(c.vertex_normals(sp), nrm, "the device's table against generate() on the oracle's records")
    ref = _ref(so, nrm)
    assert ref.pt.smooth["smooth"] >= 1000 and ref.pt.smooth["flat"] >= 100  # the teapot smooth, the mirrors flat
    plain = ER.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, SPP, SEED, MAXDEPTH)
    assert (plain.image != ref.image).any(axis=2).mean() > 0.05  # smooth shading shows
    img = np.full((H, W, 4), -7.0, F32)
    ctx = c.walk_rays(_vp(), sp, img)
    assert_bits_equal(img, ref.image, "teapot, rtmi_render")
    _assert_stats(ctx, ref)
    assert ctx.stats["trace_launches"] == MAXDEPTH


def test_device_variant_on_a_striped_tile(teapot):
    import torch
    so, sp, nrm = teapot
    tile = (1, 12, 3, 8)  # rows 1-3, 9-11, 17-19, 25-27
    ref = _ref(so, nrm, tile=tile)
    buf = torch.full((12 * W * 4 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _R().HipRayCaster(seed=SEED).walk_tile_device(_vp(), sp, tile, buf[64:].data_ptr())
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:64] == 7.5).all() and (g[64 + 12 * W * 4:] == 7.5).all()
    assert_bits_equal(g[64:64 + 12 * W * 4].reshape(12, W, 4), ref.image, "teapot, striped tile")
    _assert_stats(ctx, ref)


def test_progressive_passes_end_in_the_bits_of_one_call(teapot):
    so, sp, nrm = teapot
    ref = _ref(so, nrm)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_progressive(_vp(), sp, img, pass_samples=1)
    assert_bits_equal(img, ref.image, "four passes of one sample")
    assert ctx.samples_done == SPP and ctx.total_rays == ref.rays and ctx.stats["pipeline"] == 1


def test_adaptive_without_a_tolerance_is_the_uniform_render(teapot):
    so, sp, nrm = teapot
    ref = _ref(so, nrm)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_adaptive(_vp(), sp, img, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(img, ref.image, "adaptive, abs_tol = NaN")
    assert (ctx.counts == SPP).all() and ctx.total_rays == ref.rays


def test_views_of_two_cameras_with_two_seeds(teapot):
    R = _R()
    so, sp, nrm = teapot
    c = dict(GC.SIDE_VIEW, pos=(0.5, 1.0, 1.5), aim=(0.1, -0.1, 1.0))
    vs = _orc().create_viewport(W, H, c["size"], np.array(c["pos"], F32), _orc().unit(list(c["aim"])), 70.0, _orc().to_radians(0.0))
    views = [_vp(), R.Viewport(W, H, vs, MAXDEPTH, SPP)]
    ctx = R.HipRayCaster(seed=SEED).walk_rays_views(views, sp, seeds=[SEED, SEED + 1])
    assert_bits_equal(ctx.data[0], _ref(so, nrm).image, "view 0")
    assert_bits_equal(ctx.data[1], _ref(so, nrm, vp12=vs, seed=SEED + 1).image, "view 1")
    assert ctx.stats["pipeline"] == 1


def test_explicit_rays_of_the_camera_with_their_keys_equal_the_render(teapot):
    import torch
    so, sp, nrm = teapot
    ref = _ref(so, nrm)
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
    _assert_stats(ctx, ref)


def test_bake_light_bounces_smoothly(teapot):
    orc = _orc()
    so, sp, nrm = teapot
    c = _R().HipRayCaster(seed=SEED)
    # above the teapot looking down at it, beside it, and under the large mirror
    pos = np.array([[0.0, 2.5, 5.0, 0], [-2.0, 0.5, 4.0, 0], [3.0, 2.0, 6.0, 0]], F32)
    nrm4 = RR.vunit(np.array([[0.05, -1, 0.1, 0], [1, 0.1, 0.3, 0], [-0.4, -0.5, -0.2, 0]], F32))
    K, depth, pixel0 = 32, 5, 7
    params = c.bake_params("points", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = c.bake(sp, pos, nrm4, params, light=True, orig=True, dir=True)
    pt = SR.path_trace(orc, so, got["orig"], got["dir"], pixel0 + np.repeat(np.arange(3), K), np.tile(np.arange(K), 3), depth, SEED, normals=nrm)
    assert_bits_equal(got["light"], RR.fold(pt.color, K), "bake against the restatement")
    assert ctx.total_rays == pt.rays and ctx.stats["pipeline"] == 1 and pt.smooth["smooth"] >= 10


def test_thin_lens_camera_with_guides(teapot):
    from rust_raytrace_amd import _ffi
    orc = _orc()
    so, sp, nrm = teapot
    cr = CR.camera_rays(orc, orc.canonical_viewport(W, H), W, H, 2, SEED, CR.cam(CR.THIN_LENS, 0.05, 4.0))
    pt = SR.path_trace(orc, so, cr.o4, cr.d4, cr.keys[:, 0], cr.keys[:, 1], 5, SEED, normals=nrm)
    acc, want = CR.fold(pt.color, cr.npix, cr.n)
    alb, gn, ids = SR.features(orc, so, nrm, W, H, None, 2, SEED, rays=(cr.o4, cr.d4, cr.npix, cr.n))
    accum, img = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_samples_camera(_vp(2, 5), sp, 0, H, _ffi.Camera(CR.THIN_LENS, 0, 0.05, 4.0), 0, 2, accum, img,
                                                           albedo=True, normal=True, ids=True)
    assert_bits_equal(img, want.reshape(H, W, 4), "thin lens: out")
    assert_bits_equal(accum, acc.reshape(H, W, 4), "thin lens: accum")
    assert_bits_equal(ctx.normal.reshape(H, W, 4), gn.reshape(H, W, 4), "thin lens: the normal guide")
    assert_bits_equal(ctx.albedo.reshape(H, W, 4), alb.reshape(H, W, 4), "thin lens: albedo")
    assert np.array_equal(ctx.ids.reshape(H, W), ids.reshape(H, W))
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- scene kinds
def test_linear_list_scene():
    so, sp = CT.build_pair(CT.recipe_canonical(accel="trivial"))
    sp.smooth_normals(1, NTEAPOT)
    nrm = _generated(so, 1, NTEAPOT, 0.5)
    ref = _ref(so, nrm, spp=1, maxdepth=4, w=16, h=16)
    img, ctx = _render(sp, _vp(1, 4, 16, 16))
    assert_bits_equal(img, ref.image, "linear list")
    _assert_stats(ctx, ref)


def test_generic_tree(teapot):
    so, sp, nrm = teapot
    ref = _ref(so, nrm, spp=2, maxdepth=5)
    img, ctx = _render(sp, _vp(2, 5), options=_R().OPT_GENERIC)
    assert_bits_equal(img, ref.image, "RTMI_OPT_GENERIC")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("option", ["OPT_BVH", "OPT_FAST"])
def test_bvh_and_fast_against_their_own_trace(teapot, option):
    R = _R()
    so, sp, nrm = teapot
    caster = R.HipRayCaster(seed=SEED, options=getattr(R, option))
    ref = SR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3], normals=nrm)
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, option)
    _assert_stats(ctx, ref)
    assert ref.pt.smooth["smooth"] >= 100


def test_analytic_sphere_beside_smooth_triangles():
    R, orc = _R(), _orc()
    so, sp = GC.build_pair(GC.recipe_sphere())
    rec = so.triangles()[0]
    nrm = np.zeros((len(rec), 3, 3), F32)
    tilt = rec[:, 3:6].astype(np.float64) + np.array([0.3, -0.4, 0.2])
    nrm[1:] = (tilt / np.linalg.norm(tilt, axis=1, keepdims=True)).astype(F32)[1:, None, :]  # every triangle: one tilted normal
    sp.set_vertex_normals(nrm[1:])
    caster = R.HipRayCaster(seed=SEED)
    ref = SR.render(orc, so, orc.canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3],
                    spheres=GC.sphere_table(orc), normals=nrm)
    assert ref.pt.total["refract_in"] >= 1 and ref.pt.smooth["smooth"] >= 10
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, "an analytic glass sphere over smooth triangles")
    _assert_stats(ctx, ref)


# ---------------------------------------------------------------- tuning, depth
@pytest.mark.parametrize("tuning", [dict(streams=3, batch_paths=600, subtile_min_paths=1), dict(streams=1, batch_paths=500)])
def test_tuning_changes_no_bit(teapot, tuning):
    so, sp, nrm = teapot
    ref = _ref(so, nrm)
    img, ctx = _render(sp, _vp(), tuning=tuning)
    assert_bits_equal(img, ref.image, f"tuning {tuning}")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("maxdepth", [0, 1, 2])
def test_shallow_depths(teapot, maxdepth):
    so, sp, nrm = teapot
    ref = _ref(so, nrm, spp=2, maxdepth=maxdepth)
    img, ctx = _render(sp, _vp(2, maxdepth))
    assert_bits_equal(img, ref.image, f"maxdepth {maxdepth}")
    assert ctx.stats["rays"] == ref.rays
    if maxdepth == 0:
        assert not img.any()


# ---------------------------------------------------------------- {glass} x {environment}
@pytest.mark.parametrize("with_env", [False, True])
@pytest.mark.parametrize("scene", ["slab", "teapot"])
def test_glass_and_environment_combinations(slab, teapot, scene, with_env):
    so, sp, nrm = slab if scene == "slab" else teapot
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None) if with_env else None
    ref = SR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, env=env, normals=nrm)
    assert (ref.pt.hits0[0] == 0).any() and ref.pt.smooth["smooth"] >= 10
    assert (ref.pt.total["refract_in"] >= 1) == (scene == "slab")
    try:
        if with_env:
            sp.set_sky(8, **SUN)
        img, ctx = _render(sp, _vp(2, 5))
    finally:
        sp.clear_environment()
    assert_bits_equal(img, ref.image, f"{scene}, environment {with_env}")
    _assert_stats(ctx, ref)
    if not with_env:  # a miss starts at the sky constant, bit for bit
        first_miss = (ref.pt.hits0[0].reshape(H, W, 2) == 0).all(axis=2)
        assert first_miss.any() and (img[first_miss][:, :3] == ER.FR.SKY).all()


# ---------------------------------------------------------------- features
def test_features_normal_plane(teapot):
    so, sp, nrm = teapot
    alb, want, ids = SR.features(_orc(), so, nrm, W, H, _orc().canonical_viewport(W, H), 2, SEED)
    import features_ref as FR
    flat = FR.features_ref(_orc(), so, W, H, _orc().canonical_viewport(W, H), 2, SEED)[1]
    assert (flat != want).any(axis=2).mean() > 0.05 and (flat[..., 3] == want[..., 3]).all()  # depth does not move
    a, n, i, ctx = _R().HipRayCaster(seed=SEED).walk_rays_features(_vp(2, 5), sp)
    assert_bits_equal(n, want, "the normal plane")
    assert_bits_equal(a, alb, "albedo")
    assert np.array_equal(i, ids)


def test_denoised_wrapper_end_to_end(teapot):
    so, sp, nrm = teapot
    c = _R().HipRayCaster(seed=SEED)
    vp = _vp(2, 5)
    img = np.zeros((H, W, 4), F32)
    c.walk_rays(vp, sp, img)
    a, n, _, _ = c.walk_rays_features(vp, sp, ids=False)
    assert_bits_equal(img, _ref(so, nrm, spp=2, maxdepth=5).image, "the noisy image")
    want = c.denoise(img, a, n)
    got = np.zeros((H, W, 4), F32)
    ctx = c.walk_rays_denoised(vp, sp, got)
    assert_bits_equal(got, want, "rtmi_render_denoised = denoise(render, features) with the smooth guide")
    assert ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- setting and clearing
def test_set_replace_read_back_and_clear(teapot):
    orc, R = _orc(), _R()
    so, sp = CT.build_pair(CT.recipe_canonical())
    c = R.HipRayCaster(seed=SEED)
    assert sp.vertex_normals() is None and c.vertex_normals(sp) is None
    want, cn = so.render(W, H, orc.canonical_viewport(W, H), 5, 2, seed=SEED, threads=4)
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, want, "before any normals")
    assert ctx.stats["pipeline"] == 3
    nrm = teapot[2]
    sp.smooth_normals(1, NTEAPOT, crease_cos=1.0)  # every corner its own face's normal
    sharp = c.vertex_normals(sp)
    assert_bits_equal(sharp, _generated(so, 1, NTEAPOT, 1.0), "crease_cos = 1")
    sp.smooth_normals(1, NTEAPOT)  # replaced
    assert_bits_equal(c.vertex_normals(sp), nrm, "replaced by crease_cos = 0.5")
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, _ref(so, nrm, spp=2, maxdepth=5).image, "with normals")
    assert ctx.stats["pipeline"] == 1
    sp.set_vertex_normals(np.zeros((NTEAPOT, 3, 3), F32))  # all-zero normals: flat, on the smooth kernels
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, want, "all-zero normals render the flat image")
    assert ctx.stats["pipeline"] == 1 and ctx.stats["rays"] == cn["rays"]
    sp.clear_vertex_normals()
    assert c.vertex_normals(sp) is None
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, want, "normals cleared: the oracle's bits")
    assert ctx.stats["pipeline"] == 3 and ctx.stats["rays"] == cn["rays"]


# ---------------------------------------------------------------- refusals
def test_shadowed_refuses_vertex_normals_and_the_handle_stays_usable(teapot):
    so, sp, nrm = teapot
    c = _R().HipRayCaster(seed=SEED)
    ref = _ref(so, nrm, spp=2, maxdepth=5)
    _render(sp, _vp(2, 5))  # the scene is on the device
    with pytest.raises(RuntimeError, match="vertex normals"):
        c.walk_rays_shadowed(_vp(2, 5), sp, orig=(2.0, 3.0, 0.0))
    again, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(again, ref.image, "after the refusal")
    _assert_stats(ctx, ref)


def test_bad_arguments_are_refused_by_the_abi():
    import test_gpu_abi_raw as RAW
    L, ffi = RAW._lib()
    so = CT.recipe_axis_box()(CT.OracleApi(_orc()))
    tris, geo, topo, refs = RAW._abi_arrays(so)
    rc, h = RAW._create(L, tris, RAW._boxes(geo, topo), refs)
    assert rc == RAW.RTMI_OK
    try:
        rec = so.triangles()[0]
        n = len(rec)
        corners = np.ascontiguousarray(rec[:, 20:29])
        tilt = rec[:, 3:6].astype(np.float64) + np.array([0.2, 0.3, -0.25])
        nrm = np.zeros((n, 3, 3), F32)
        nrm[1:] = (tilt / np.linalg.norm(tilt, axis=1, keepdims=True)).astype(F32)[1:, None, :]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        cnt = C.c_uint64(9)
        assert L.rtmi_scene_set_normals(h, p(corners), p(nrm), n - 1) == RAW.RTMI_ERR_INVALID and b"ntris" in L.rtmi_last_error()
        assert L.rtmi_scene_set_normals(h, None, p(nrm), n) == RAW.RTMI_ERR_INVALID
        for bad in (float("nan"), float("inf")):
            x = nrm.copy()
            x[n - 1, 2, 1] = bad
            assert L.rtmi_scene_set_normals(h, p(corners), p(x), n) == RAW.RTMI_ERR_INVALID and b"normal" in L.rtmi_last_error()
            y = corners.copy()
            y[1, 4] = bad
            assert L.rtmi_scene_set_normals(h, p(y), p(nrm), n) == RAW.RTMI_ERR_INVALID and b"corner" in L.rtmi_last_error()
        assert L.rtmi_scene_get_normals(h, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0  # none of them left anything behind
        out = np.zeros((4, 3, 3), F32)
        for cc in (1.5, -1.01, float("nan")):
            assert L.rtmi_smooth_normals(p(corners), p(np.ascontiguousarray(rec[:, 3:6])), 4, C.c_float(cc), p(out)) == RAW.RTMI_ERR_INVALID
        # set, read back, render, remove through the raw ABI; entry 0 may hold anything
        x, y = nrm.copy(), corners.copy()
        x[0], y[0] = float("nan"), float("inf")
        assert L.rtmi_scene_set_normals(h, p(y), p(x), n) == RAW.RTMI_OK, L.rtmi_last_error()
        back = np.full((n, 3, 3), 7.0, F32)
        assert L.rtmi_scene_get_normals(h, p(back), C.byref(cnt)) == RAW.RTMI_OK and cnt.value == n
        assert_bits_equal(back, nrm, "rtmi_scene_get_normals")
        w = 8
        vo = _orc().canonical_viewport(w, w)
        got, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        assert_bits_equal(got, SR.render(_orc(), so, vo, w, w, 1, SEED, 3, normals=nrm).image, "raw ABI, smooth")
        assert st.pipeline == 1
        assert L.rtmi_scene_set_normals(h, p(corners), None, n) == RAW.RTMI_OK
        assert L.rtmi_scene_get_normals(h, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0
        plain, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        want, _ = so.render(w, w, vo, 3, 1, seed=SEED, threads=2)
        assert_bits_equal(plain, want, "raw ABI, the normals removed")
    finally:
        L.rtmi_scene_destroy(h)
