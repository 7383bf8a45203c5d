"""-m gpu: the textures of a scene (rtmi_scene_set_textures / rtmi_project_uvs, include/rtmi.h) through every call that gains
them, every float bit for bit against tests/tex_ref.py, the float32 NumPy restatement of the header on the oracle's closest hits,
records and RNG (tests/test_tex_cpu.py pins it), so no expected value comes from the code under test: the projected uvs of a case
are tex_ref.project's on the oracle's records, and the device's tables are held against them.  RTMI_OPT_BVH, RTMI_OPT_FAST and
analytic spheres are held against the restatement fed by the product's own rtmi_trace, as in tests/test_smooth.py, whose matrix
this is.  Scenes: tests/tex_cases.py's patch and the canonical scene with the teapot box-projected, 32 x 32, spp 4, depth <= 6.
The references are computed once per case and shared."""
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
import tex_cases as TC
import tex_ref as TR

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = GC.VIEW["w"], GC.VIEW["h"]
SPP, SEED, MAXDEPTH = 4, 5, 6
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
LO, SCALE = (-1.7, -0.4, 3.1), 0.9  # the box projection of the teapot: about three repeats across it
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _projected(so, first, count, texture):
    """The textures namespace Scene.project_uvs(first, count, LO, SCALE, texture) with the 8 x 8 image must produce, from the
    oracle's records"""
    rec = so.triangles()[0]
    uvs, tot = np.zeros((len(rec), 3, 2), F32), np.zeros(len(rec), np.uint32)
    uvs[first:first + count] = TR.project(rec[first:first + count, 20:29], rec[first:first + count, 3:6], LO, SCALE)
    tot[first:first + count] = texture
    return TR.textures([TC.images()[3]], uvs, tot)


@pytest.fixture(scope="module")
def teapot():
    """The canonical Matte / Reflective scene, the teapot box-projected with the 8 x 8 texture"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_textures([TC.images()[3]], None, None)
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    return so, sp, _projected(so, 1, NTEAPOT, 1)


@pytest.fixture(scope="module")
def patch():
    so, sp = GC.build_pair(TC.recipe_patch())
    uvs, tot = TC.patch_uvs(len(so.triangles()[0]))
    sp.set_textures(TC.images(), uvs[1:], tot[1:])
    o4, d4 = TC.rays()
    return so, sp, TR.textures(TC.images(), uvs, tot), o4, d4


def _ref(so, tex, spp=SPP, maxdepth=MAXDEPTH, vp12=None, w=W, h=H, seed=SEED, env=None, normals=None, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    vo = _orc().canonical_viewport(w, h) if vp12 is None else vp12
    key = (id(so), id(tex), id(env), id(normals), spp, maxdepth, tuple(np.asarray(vo, F32).tolist()), w, h, seed,
           tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = TR.render(_orc(), so, vo, w, h, spp, seed, maxdepth, env=env, normals=normals, tex=tex, **kw)
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


def _patch_conditions(so, tex, o4, d4):
    """The conditions on the inputs that tests/test_tex_cpu.py verifies as counts, as plain asserts"""
    recs, kinds, surf = so.triangles()
    tri, t, face, _ = so.trace(o4, d4)
    tri, face, t = np.asarray(tri, np.int64), np.asarray(face, np.uint32), np.asarray(t, F32)
    ok = (tri != 0) & ((face & 2) == 0)
    point = ((d4[ok] * t[ok, None]).astype(F32) + o4[ok]).astype(F32)
    _, d = TR.colour(TR.records(recs[:, 20:29], tex.uvs, tex.tex_of_tri), tex.images, tri[ok], point, surf[tri[ok], :3], detail=True)
    T = d.textured
    for m in (d.u < 0, d.v < 0, d.u > 1, d.v > 1, d.ix == -1, d.ix + 1 == d.w, d.iy == -1, d.iy + 1 == d.h):
        assert (T & m).sum() >= 20
    assert (~T).sum() >= 20 and (T & (tri[ok] == TC.SOLID_TRI)).sum() >= 20


# ---------------------------------------------------------------- the patch
def test_patch_depth_1_on_explicit_rays_with_guides(patch):
    so, sp, tex, o4, d4 = patch
    _patch_conditions(so, tex, o4, d4)
    n = len(o4)
    alb, nrm, ids = TR.features(_orc(), so, None, tex, 0, 0, None, 1, SEED, rays=(o4, d4, n, 1))
    flat = SR.features(_orc(), so, np.zeros((len(tex.uvs), 3, 3), F32), 0, 0, None, 1, SEED, rays=(o4, d4, n, 1))
    assert (alb != flat[0]).any(axis=1).sum() >= 500 and (alb[:, 3] == flat[0][:, 3]).all()  # the textures show; coverage stays
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o4, d4, 1, color=True, albedo=True, normal=True, ids=True)
    assert_bits_equal(got["albedo"], alb, "the albedo guide of the patch")
    assert_bits_equal(got["normal"], nrm, "the normal guide: unchanged")
    assert_bits_equal(got["normal"], flat[1], "the normal guide is the untextured scene's")
    assert np.array_equal(got["ids"], ids) and np.array_equal(ids, flat[2])
    pt = TR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 1, SEED, tex=tex)
    assert pt.tex["solid"] >= 20
    assert_bits_equal(got["color"], pt.color, "depth 1: the textured Solid shows its colour, everything that would bounce is black")
    assert ctx.stats["rays"] == n and ctx.stats["pipeline"] == 1


def test_patch_depth_3_folds_through_the_colour_stack(patch):
    so, sp, tex, o4, d4 = patch
    n = len(o4)
    pt = TR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, SEED, tex=tex)
    c = pt.tex
    assert min(c["matte"], c["reflective"], c["glass"]) >= 100 and c["solid"] >= 20 and c["untextured"] >= 100, c
    plain = SR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 3, SEED)
    assert (plain.color != pt.color).any(axis=1).sum() >= 500 and plain.rays == pt.rays  # colours move, paths do not
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o4, d4, 3)
    assert_bits_equal(got["color"], pt.color, "the patch at depth 3")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1 and ctx.stats["slow_paths"] == 0


def test_patch_with_normals_and_a_sky_all_four_flags_live(patch):
    so, sp, tex, o4, d4 = patch
    n = len(o4)
    nrm = np.zeros((len(tex.uvs), 3, 3), F32)
    nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(so.triangles()[0])[:SC.NTRI_PATCH + 1]
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)
    pt = TR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 4, SEED, env=env, normals=nrm, tex=tex)
    flat = TR.path_trace(_orc(), so, o4, d4, np.arange(n), np.zeros(n, np.int64), 4, SEED, env=env, tex=tex)
    assert (flat.color != pt.color).any(axis=1).sum() >= 100 and pt.total["refract_in"] >= 10 and (pt.hits0[0] == 0).any()
    try:
        sp.set_vertex_normals(nrm[1:])
        sp.set_sky(8, **SUN)
        got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, o4, d4, 4)
    finally:
        sp.clear_environment()
        sp.clear_vertex_normals()
    assert_bits_equal(got["color"], pt.color, "textures, vertex normals, glass and an environment at once")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


def test_all_ones_textures_render_the_untextured_image_of_the_existing_kernels(patch):
    so, sp, tex, o4, d4 = patch
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    ref = _ref(so, tex, spp=2, maxdepth=5)  # textures and nothing else: SmoothTab and EnvTab are empty
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, ref.image, "the patch through the camera")
    _assert_stats(ctx, ref)
    _, plain = GC.build_pair(TC.recipe_patch())
    want, pctx = _render(plain, _vp(2, 5))
    assert pctx.stats["pipeline"] == 1  # (glass: the existing k_shade_glass)
    assert_bits_equal(want, SR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5).image, "untextured")
    assert (want != img).any(axis=2).mean() > 0.02
    plain.set_textures(TC.images(ones=True), tex.uvs[1:], tex.tex_of_tri[1:])
    ones, octx = _render(plain, _vp(2, 5))
    assert_bits_equal(ones, want, "all-ones textures on the _tex kernels against the existing kernels")
    assert octx.stats["pipeline"] == 1 and octx.stats["rays"] == pctx.stats["rays"]
    a1 = c.walk_rays_features(_vp(2, 5), plain)[0]
    plain.clear_textures()
    a0 = c.walk_rays_features(_vp(2, 5), plain)[0]
    assert_bits_equal(a1, a0, "all-ones albedo")


def test_table_read_back(patch, teapot):
    so, sp, tex, _, _ = patch
    images, uvs, tot = _R().HipRayCaster(seed=SEED).textures(sp)
    rec = TR.records(so.triangles()[0][:, 20:29], tex.uvs, tex.tex_of_tri)
    assert rec.den[TC.SLIVER_TRI] == 0 and tex.tex_of_tri[TC.SLIVER_TRI] != 0 and rec.tex[TC.SLIVER_TRI] == 0
    assert_bits_equal(uvs, tex.uvs, "the device's uvs")
    assert np.array_equal(tot, rec.tex)  # (the sliver reads as texture 0)
    assert len(images) == 4
    for a, b in zip(images, TC.images()):
        assert a.shape == b.shape
        assert_bits_equal(a, b, "the device's texels")
    so, sp, tex = teapot
    images, uvs, tot = _R().HipRayCaster(seed=SEED).textures(sp)
    assert_bits_equal(uvs, tex.uvs, "project_uvs against tex_ref.project on the oracle's records")
    assert np.array_equal(tot, tex.tex_of_tri) and len(images) == 1
    assert_bits_equal(images[0], tex.images[0], "the 8 x 8 image")


# ---------------------------------------------------------------- the teapot through every call
def test_teapot_host_variant(teapot):
    so, sp, tex = teapot
    ref = _ref(so, tex)
    assert ref.pt.tex["matte"] >= 1000 and ref.pt.tex["untextured"] >= 100
    plain = SR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, SPP, SEED, MAXDEPTH)
    assert (plain.image != ref.image).any(axis=2).mean() > 0.05 and plain.rays == ref.rays
    img, ctx = _render(sp, _vp())
    assert_bits_equal(img, ref.image, "teapot, rtmi_render")
    _assert_stats(ctx, ref)
    assert ctx.stats["trace_launches"] == MAXDEPTH


def test_device_variant_on_a_striped_tile(teapot):
    import torch
    so, sp, tex = teapot
    tile = (1, 12, 3, 8)  # rows 1-3, 9-11, 17-19, 25-27
    ref = _ref(so, tex, tile=tile)
    buf = torch.full((12 * W * 4 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _R().HipRayCaster(seed=SEED).walk_tile_device(_vp(), sp, tile, buf[64:].data_ptr())
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:64] == 7.5).all() and (g[64 + 12 * W * 4:] == 7.5).all()
    assert_bits_equal(g[64:64 + 12 * W * 4].reshape(12, W, 4), ref.image, "teapot, striped tile")
    _assert_stats(ctx, ref)


def test_progressive_passes_end_in_the_bits_of_one_call(teapot):
    so, sp, tex = teapot
    ref = _ref(so, tex)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_progressive(_vp(), sp, img, pass_samples=1)
    assert_bits_equal(img, ref.image, "four passes of one sample")
    assert ctx.samples_done == SPP and ctx.total_rays == ref.rays and ctx.stats["pipeline"] == 1


def test_adaptive_without_a_tolerance_is_the_uniform_render(teapot):
    so, sp, tex = teapot
    ref = _ref(so, tex)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_adaptive(_vp(), sp, img, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(img, ref.image, "adaptive, abs_tol = NaN")
    assert (ctx.counts == SPP).all() and ctx.total_rays == ref.rays


def test_views_of_two_cameras_with_two_seeds(teapot):
    R = _R()
    so, sp, tex = teapot
    c = dict(GC.SIDE_VIEW, pos=(0.5, 1.0, 1.5), aim=(0.1, -0.1, 1.0))
    vs = _orc().create_viewport(W, H, c["size"], np.array(c["pos"], F32), _orc().unit(list(c["aim"])), 70.0, _orc().to_radians(0.0))
    views = [_vp(), R.Viewport(W, H, vs, MAXDEPTH, SPP)]
    ctx = R.HipRayCaster(seed=SEED).walk_rays_views(views, sp, seeds=[SEED, SEED + 1])
    assert_bits_equal(ctx.data[0], _ref(so, tex).image, "view 0")
    assert_bits_equal(ctx.data[1], _ref(so, tex, vp12=vs, seed=SEED + 1).image, "view 1")
    assert ctx.stats["pipeline"] == 1


def test_frame_multi_on_two_handles_of_one_device(teapot):
    so, sp, tex = teapot
    ref = _ref(so, tex)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED, devices=[0, 0]).walk_frame_multi(_vp(), sp, img, stripe_rows=4)
    assert_bits_equal(img, ref.image, "rtmi_render_frame_multi: both handles carry the textures")
    assert ctx.total_rays == ref.rays and all(d["pipeline"] == 1 for d in ctx.per_device)


def test_explicit_rays_of_the_camera_with_their_keys_equal_the_render(teapot):
    import torch
    so, sp, tex = teapot
    ref = _ref(so, tex)
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


def test_bake_gathers_textured_light(teapot):
    orc = _orc()
    so, sp, tex = teapot
    c = _R().HipRayCaster(seed=SEED)
    # above the teapot looking down at it, beside it, and under the large mirror
    pos = np.array([[0.0, 2.5, 5.0, 0], [-2.0, 0.5, 4.0, 0], [3.0, 2.0, 6.0, 0]], F32)
    nrm4 = RR.vunit(np.array([[0.05, -1, 0.1, 0], [1, 0.1, 0.3, 0], [-0.4, -0.5, -0.2, 0]], F32))
    K, depth, pixel0 = 32, 5, 7
    params = c.bake_params("points", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = c.bake(sp, pos, nrm4, params, light=True, orig=True, dir=True)
    pt = TR.path_trace(orc, so, got["orig"], got["dir"], pixel0 + np.repeat(np.arange(3), K), np.tile(np.arange(K), 3), depth, SEED, tex=tex)
    assert_bits_equal(got["light"], RR.fold(pt.color, K), "bake against the restatement")
    assert ctx.total_rays == pt.rays and ctx.stats["pipeline"] == 1 and pt.tex["matte"] >= 10


def test_thin_lens_camera_with_guides(teapot):
    from rust_raytrace_amd import _ffi
    orc = _orc()
    so, sp, tex = teapot
    cr = CR.camera_rays(orc, orc.canonical_viewport(W, H), W, H, 2, SEED, CR.cam(CR.THIN_LENS, 0.05, 4.0))
    pt = TR.path_trace(orc, so, cr.o4, cr.d4, cr.keys[:, 0], cr.keys[:, 1], 5, SEED, tex=tex)
    acc, want = CR.fold(pt.color, cr.npix, cr.n)
    alb, gn, ids = TR.features(orc, so, None, tex, W, H, None, 2, SEED, rays=(cr.o4, cr.d4, cr.npix, cr.n))
    accum, img = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_samples_camera(_vp(2, 5), sp, 0, H, _ffi.Camera(CR.THIN_LENS, 0, 0.05, 4.0), 0, 2, accum, img,
                                                           albedo=True, normal=True, ids=True)
    assert_bits_equal(img, want.reshape(H, W, 4), "thin lens: out")
    assert_bits_equal(accum, acc.reshape(H, W, 4), "thin lens: accum")
    assert_bits_equal(ctx.albedo.reshape(H, W, 4), alb.reshape(H, W, 4), "thin lens: the albedo guide")
    assert_bits_equal(ctx.normal.reshape(H, W, 4), gn.reshape(H, W, 4), "thin lens: the normal guide")
    assert np.array_equal(ctx.ids.reshape(H, W), ids.reshape(H, W))
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


def test_features_albedo_plane(teapot):
    so, sp, tex = teapot
    alb, nrm, ids = TR.features(_orc(), so, None, tex, W, H, _orc().canonical_viewport(W, H), 2, SEED)
    import features_ref as FR
    flat = FR.features_ref(_orc(), so, W, H, _orc().canonical_viewport(W, H), 2, SEED)
    assert (flat[0] != alb).any(axis=2).mean() > 0.05 and (flat[0][..., 3] == alb[..., 3]).all()  # coverage does not move
    a, n, i, ctx = _R().HipRayCaster(seed=SEED).walk_rays_features(_vp(2, 5), sp)
    assert_bits_equal(a, alb, "the albedo plane")
    assert_bits_equal(n, nrm, "the normal plane")
    assert_bits_equal(n, flat[1], "the normal plane is the untextured scene's")
    assert np.array_equal(i, ids)


def test_denoised_wrapper_end_to_end(teapot):
    so, sp, tex = teapot
    c = _R().HipRayCaster(seed=SEED)
    vp = _vp(2, 5)
    img = np.zeros((H, W, 4), F32)
    c.walk_rays(vp, sp, img)
    a, n, _, _ = c.walk_rays_features(vp, sp, ids=False)
    assert_bits_equal(img, _ref(so, tex, spp=2, maxdepth=5).image, "the noisy image")
    assert_bits_equal(a, TR.features(_orc(), so, None, tex, W, H, _orc().canonical_viewport(W, H), 2, SEED)[0], "the textured guide")
    want = c.denoise(img, a, n)
    got = np.zeros((H, W, 4), F32)
    ctx = c.walk_rays_denoised(vp, sp, got)
    assert_bits_equal(got, want, "rtmi_render_denoised = denoise(render, features) with the textured albedo guide")
    assert ctx.stats["pipeline"] == 1


def test_adaptive_denoised_wrapper_end_to_end(teapot):
    from test_denoise_var import _adaptive_frame
    so, sp, tex = teapot
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    f = _adaptive_frame(R, c, sp, W, H, SPP, 2, 1, None, float("nan"), depth=MAXDEPTH)
    assert_bits_equal(f["color"], _ref(so, tex).image, "the adaptive render")
    assert_bits_equal(f["albedo"], TR.features(_orc(), so, None, tex, W, H, _orc().canonical_viewport(W, H), SPP, SEED, nsamples=2)[0],
                      "the guide of the first two samples")
    want = c.denoise_var(f["color"], f["albedo"], f["normal"], f["var"])
    got = np.full((H, W, 4), np.nan, F32)
    ctx = c.walk_rays_adaptive_denoised(f["vp"], sp, got, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(got, want, "rtmi_render_adaptive_denoised = its four calls")
    assert ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- scene kinds and options
def test_linear_list_scene():
    so, sp = CT.build_pair(CT.recipe_canonical(accel="trivial"))
    sp.set_textures([TC.images()[3]], None, None)
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    ref = _ref(so, _projected(so, 1, NTEAPOT, 1), spp=1, maxdepth=4, w=16, h=16)
    img, ctx = _render(sp, _vp(1, 4, 16, 16))
    assert_bits_equal(img, ref.image, "linear list")
    _assert_stats(ctx, ref)


def test_generic_tree(teapot):
    so, sp, tex = teapot
    ref = _ref(so, tex, spp=2, maxdepth=5)
    img, ctx = _render(sp, _vp(2, 5), options=_R().OPT_GENERIC)
    assert_bits_equal(img, ref.image, "RTMI_OPT_GENERIC")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("option", ["OPT_BVH", "OPT_FAST"])
def test_bvh_and_fast_against_their_own_trace(teapot, option):
    R = _R()
    so, sp, tex = teapot
    caster = R.HipRayCaster(seed=SEED, options=getattr(R, option))
    ref = TR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3], tex=tex)
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, option)
    _assert_stats(ctx, ref)
    assert ref.pt.tex["matte"] >= 100


def test_analytic_sphere_beside_textured_triangles():
    R, orc = _R(), _orc()
    so, sp = GC.build_pair(GC.recipe_sphere())
    rec = so.triangles()[0]
    n = len(rec)
    uvs = TR.project(rec[:, 20:29], rec[:, 3:6], (0.1, 0.2, 0.3), 0.7)
    tot = np.full(n, 1, np.uint32)
    tot[0] = 0
    sp.set_textures([TC.images()[2]], uvs[1:], tot[1:])
    tex = TR.textures([TC.images()[2]], uvs, tot)
    caster = R.HipRayCaster(seed=SEED)
    ref = TR.render(orc, so, orc.canonical_viewport(W, H), W, H, 2, SEED, 5, trace=lambda o, d: caster.trace(sp, o, d)[:3],
                    spheres=GC.sphere_table(orc), tex=tex)
    assert ref.pt.total["refract_in"] >= 1 and sum(ref.pt.tex[k] for k in ("solid", "matte", "reflective", "glass")) >= 100
    img = np.zeros((H, W, 4), F32)
    ctx = caster.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, ref.image, "an analytic glass sphere (untextured) over textured triangles")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("tuning", [dict(streams=3, batch_paths=600, subtile_min_paths=1), dict(streams=1, batch_paths=500)])
def test_tuning_changes_no_bit(teapot, tuning):
    so, sp, tex = teapot
    ref = _ref(so, tex)
    img, ctx = _render(sp, _vp(), tuning=tuning)
    assert_bits_equal(img, ref.image, f"tuning {tuning}")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("maxdepth", [0, 1, 2])
def test_shallow_depths(teapot, maxdepth):
    so, sp, tex = teapot
    ref = _ref(so, tex, spp=2, maxdepth=maxdepth)
    img, ctx = _render(sp, _vp(2, maxdepth))
    assert_bits_equal(img, ref.image, f"maxdepth {maxdepth}")
    assert ctx.stats["rays"] == ref.rays
    if maxdepth == 0:
        assert not img.any()


# ---------------------------------------------------------------- setting and clearing
def test_set_replace_and_clear_returns_the_exact_earlier_image_and_pipeline(teapot):
    orc, R = _orc(), _R()
    so, sp = CT.build_pair(CT.recipe_canonical())
    c = R.HipRayCaster(seed=SEED)
    assert sp.textures() is None and c.textures(sp) is None
    want, cn = so.render(W, H, orc.canonical_viewport(W, H), 5, 2, seed=SEED, threads=4)
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, want, "before any textures")
    assert ctx.stats["pipeline"] == 3
    sp.set_textures([TC.images()[1]], None, None)
    sp.project_uvs(1, NTEAPOT, (0, 0, 0), 2.0, 1)
    first, fctx = _render(sp, _vp(2, 5))
    assert fctx.stats["pipeline"] == 1 and (first != want).any()
    sp.set_textures([TC.images()[3]], None, None)  # replaced: the image, then the uvs
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, _ref(so, teapot[2], spp=2, maxdepth=5).image, "replaced")
    assert ctx.stats["pipeline"] == 1
    sp.clear_textures()
    assert sp.textures() is None and c.textures(sp) is None
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, want, "textures cleared: the oracle's bits")
    assert ctx.stats["pipeline"] == 3 and ctx.stats["rays"] == cn["rays"]


# ---------------------------------------------------------------- refusals
def test_shadowed_and_preview_refuse_textures_and_the_handle_stays_usable(teapot):
    so, sp, tex = teapot
    c = _R().HipRayCaster(seed=SEED)
    ref = _ref(so, tex, spp=2, maxdepth=5)
    _render(sp, _vp(2, 5))  # the scene is on the device
    with pytest.raises(RuntimeError, match="textures"):
        c.walk_rays_shadowed(_vp(2, 5), sp, orig=(2.0, 3.0, 0.0))
    with pytest.raises(RuntimeError, match="textures"):
        c.walk_rays_preview(_vp(2, 5), sp)
    again, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(again, ref.image, "after the refusals")
    _assert_stats(ctx, ref)


def test_bad_arguments_are_refused_by_the_abi():
    import test_gpu_abi_raw as RAW
    from rust_raytrace_amd import _ffi
    L, ffi = RAW._lib()
    so = CT.recipe_axis_box()(CT.OracleApi(_orc()))
    tris, geo, topo, refs = RAW._abi_arrays(so)
    rc, h = RAW._create(L, tris, RAW._boxes(geo, topo), refs)
    assert rc == RAW.RTMI_OK
    try:
        rec = so.triangles()[0]
        n = len(rec)
        corners = np.ascontiguousarray(rec[:, 20:29])
        uvs = TR.project(corners, rec[:, 3:6], (0, 0, 0), 0.5)
        tot = np.full(n, 2, np.uint32)
        imgs = [TC.images()[2], TC.images()[0]]
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def texs(images, flags=0, wh=None):
            arr = (_ffi.Texture * len(images))()
            for k, a in enumerate(images):
                w, hh = (a.shape[1], a.shape[0]) if wh is None else wh
                arr[k] = _ffi.Texture(a.ctypes.data, w, hh, flags)
            return arr

        cnt = C.c_uint64(9)
        bad = lambda *a: L.rtmi_scene_set_textures(h, *a) == RAW.RTMI_ERR_INVALID
        assert bad(texs(imgs), 2, p(corners), p(uvs), p(tot), n - 1) and b"ntris" in L.rtmi_last_error()
        assert bad(texs(imgs), 2, None, p(uvs), p(tot), n)
        assert bad(texs(imgs, flags=1), 2, p(corners), p(uvs), p(tot), n) and b"flags" in L.rtmi_last_error()
        assert bad(texs(imgs, wh=(8193, 1)), 2, p(corners), p(uvs), p(tot), n) and b"8192" in L.rtmi_last_error()
        assert bad(texs(imgs, wh=(0, 1)), 2, p(corners), p(uvs), p(tot), n)
        assert bad(texs(imgs * 129), 258, p(corners), p(uvs), p(tot), n) and b"256" in L.rtmi_last_error()
        assert bad(texs(imgs * 5, wh=(8192, 2048)), 10, p(corners), p(uvs), p(tot), n) and b"2^26" in L.rtmi_last_error()
        x = tot.copy()
        x[n - 1] = 3
        assert bad(texs(imgs), 2, p(corners), p(uvs), p(x), n) and b"above ntex" in L.rtmi_last_error()
        for v in (float("nan"), float("inf")):
            y = uvs.copy()
            y[n - 1, 2, 1] = v
            assert bad(texs(imgs), 2, p(corners), p(y), p(tot), n) and b"uv" in L.rtmi_last_error()
            z = corners.copy()
            z[1, 4] = v
            assert bad(texs(imgs), 2, p(z), p(uvs), p(tot), n) and b"corner" in L.rtmi_last_error()
        assert L.rtmi_scene_get_uvs(h, None, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0  # none of them left anything behind
        # set, read back, render, remove through the raw ABI; entry 0 and untextured triangles may hold anything
        y, z, x = uvs.copy(), corners.copy(), tot.copy()
        y[0], z[0], x[0] = float("nan"), float("inf"), 77
        x[2] = 0
        y[2], z[2] = float("nan"), float("inf")
        x[3] = 1
        assert L.rtmi_scene_set_textures(h, texs(imgs), 2, p(z), p(y), p(x), n) == RAW.RTMI_OK, L.rtmi_last_error()
        back, tback = np.full((n, 3, 2), 7.0, F32), np.full(n, 9, np.uint32)
        assert L.rtmi_scene_get_uvs(h, p(back), p(tback), C.byref(cnt)) == RAW.RTMI_OK and cnt.value == n
        assert_bits_equal(back[1:], y[1:], "rtmi_scene_get_uvs")
        assert np.array_equal(tback[1:], x[1:]) and tback[0] == 0
        ww, hh = C.c_uint32(0), C.c_uint32(0)
        im = np.zeros_like(imgs[0])
        assert L.rtmi_scene_get_texture(h, 1, p(im), C.byref(ww), C.byref(hh)) == RAW.RTMI_OK and (ww.value, hh.value) == (5, 3)
        assert_bits_equal(im, imgs[0], "rtmi_scene_get_texture")
        assert L.rtmi_scene_get_texture(h, 3, None, C.byref(ww), C.byref(hh)) == RAW.RTMI_ERR_INVALID
        w = 8
        vo = _orc().canonical_viewport(w, w)
        got, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        x[0] = 0
        assert_bits_equal(got, TR.render(_orc(), so, vo, w, w, 1, SEED, 3, tex=TR.textures(imgs, y, x)).image, "raw ABI, textured")
        assert st.pipeline == 1
        assert L.rtmi_scene_set_textures(h, None, 0, None, None, None, 0) == RAW.RTMI_OK
        assert L.rtmi_scene_get_uvs(h, None, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0
        plain, st = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        want, _ = so.render(w, w, vo, 3, 1, seed=SEED, threads=2)
        assert_bits_equal(plain, want, "raw ABI, the textures removed")
    finally:
        L.rtmi_scene_destroy(h)
