"""-m gpu: the normal maps of a scene (rtmi_scene_set_normal_maps, include/rtmi.h) through every call that gains them, every float
bit for bit against tests/nmap_ref.py, the float32 NumPy restatement of the header on the oracle's closest hits, records and RNG
(tests/test_nmap_cpu.py pins it), so no expected value comes from the code under test: the map of the teapot is
nmap_ref.from_height's, its uvs are tex_ref.project's on the oracle's records.  Scenes: tests/nmap_cases.py's patch and the canonical
scene with the teapot box-projected, tests/test_tex.py's view, spp 4, depth <= 6.  The references are computed once per case and
shared."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import camera_ref as CR
import env_ref as ER
import glass_cases as GC
import nmap_cases as NC
import nmap_ref as NR
import rays_ref as RR
import smooth_cases as SC
import tex_cases as TC
import tex_ref as TR

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = GC.VIEW["w"], GC.VIEW["h"]
SPP, SEED, MAXDEPTH = 4, 5, 6
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
LO, SCALE = (-1.7, -0.4, 3.1), 0.9  # tests/test_tex.py's box projection of the teapot
HEIGHT_SCALE = 2.0
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _teapot_inputs(so):
    """(tex, nm) of the restatement for the teapot: the 8 x 8 texture and an 8 x 8 map from seeded heights, box-projected uvs"""
    rec = so.triangles()[0]
    uvs, tot, nm = np.zeros((len(rec), 3, 2), F32), np.zeros(len(rec), np.uint32), np.zeros(len(rec), np.uint32)
    uvs[1:1 + NTEAPOT] = TR.project(rec[1:1 + NTEAPOT, 20:29], rec[1:1 + NTEAPOT, 3:6], LO, SCALE)
    tot[1:1 + NTEAPOT] = 1
    nm[1:1 + NTEAPOT] = 2
    return TR.textures([TC.images()[3], NR.from_height(NC.heights(), HEIGHT_SCALE)], uvs, tot), NR.maps(nm)


def _map_the_teapot(sp):
    R = _R()
    sp.set_textures([TC.images()[3], R.normal_map_from_height(NC.heights(), HEIGHT_SCALE)], None, None)
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))


@pytest.fixture(scope="module")
def teapot():
    """The canonical Matte / Reflective scene, the teapot box-projected with the 8 x 8 texture and an 8 x 8 normal map"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    _map_the_teapot(sp)
    tex, nm = _teapot_inputs(so)
    return so, sp, tex, nm


@pytest.fixture(scope="module")
def patch():
    so, sp = GC.build_pair(NC.recipe_patch())
    n = len(so.triangles()[0])
    uvs, tot = NC.patch_uvs(n)
    nm = NC.patch_nmaps(n)
    sp.set_textures(NC.images(), uvs[1:], tot[1:])
    sp.set_normal_maps(nm[1:])
    o4, d4 = NC.rays()
    nrm = np.zeros((n, 3, 3), F32)
    nrm[:SC.NTRI_PATCH + 1] = SC.patch_normals(so.triangles()[0])[:SC.NTRI_PATCH + 1]
    return SimpleNamespace(so=so, sp=sp, uvs=uvs, tot=tot, nmaps=nm, tex=TR.textures(NC.images(), uvs, tot), nm=NR.maps(nm), o4=o4, d4=d4,
                           normals=nrm, n=n)


def _ref(so, tex, nm, spp=SPP, maxdepth=MAXDEPTH, vp12=None, w=W, h=H, seed=SEED, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    vo = _orc().canonical_viewport(w, h) if vp12 is None else vp12
    key = (id(so), id(tex), id(nm), spp, maxdepth, tuple(np.asarray(vo, F32).tolist()), w, h, seed, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = NR.render(_orc(), so, vo, w, h, spp, seed, maxdepth, tex=tex, nm=nm, **kw)
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


def _paths(p, depth, tex=None, nm=None, **kw):
    n = len(p.o4)
    return NR.path_trace(_orc(), p.so, p.o4, p.d4, np.arange(n), np.zeros(n, np.int64), depth, SEED, tex=p.tex if tex is None else tex,
                         nm=p.nm if nm is None else nm, **kw)


# ---------------------------------------------------------------- the patch
def test_patch_depth_1_on_explicit_rays_with_guides(patch):
    p = patch
    n = len(p.o4)
    alb, nrm, ids = NR.features(_orc(), p.so, None, p.tex, p.nm, 0, 0, None, 1, SEED, rays=(p.o4, p.d4, n, 1))
    plain = TR.features(_orc(), p.so, None, p.tex, 0, 0, None, 1, SEED, rays=(p.o4, p.d4, n, 1))
    assert (nrm[:, :3] != plain[1][:, :3]).any(axis=1).sum() >= 500 and (nrm[:, 3] == plain[1][:, 3]).all()  # the relief shows; depth stays
    hn = NR.hit_normals(p.so, None, p.tex, p.nm, p.o4, p.d4)
    assert (hn.usem & (hn.tri == TC.SOLID_TRI)).sum() >= 20  # the guide sees the mapped Solid triangle
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(p.sp, p.o4, p.d4, 1, color=True, albedo=True, normal=True, ids=True)
    assert_bits_equal(got["normal"], nrm, "the normal guide of the patch")
    assert_bits_equal(got["albedo"], alb, "the albedo guide")
    assert_bits_equal(got["albedo"], plain[0], "the albedo guide is the unmapped scene's")
    assert np.array_equal(got["ids"], ids) and np.array_equal(ids, plain[2])
    pt = _paths(p, 1)
    assert_bits_equal(got["color"], pt.color, "depth 1: nothing bounces, no map is looked at")
    assert ctx.stats["rays"] == n and ctx.stats["pipeline"] == 1


def test_patch_depth_3_all_kinds_with_the_conditions_counted(patch):
    p = patch
    tex = TR.textures(NC.images(wild=True), p.uvs, p.tot)
    pt = _paths(p, 3, tex=tex, normals=p.normals)
    c = pt.nmap
    for k in ("usem", "away_from_ray", "away_from_ng", "nan", "retry_usem", "back_usem", "flat_usem", "mapped_matte", "mapped_reflective",
              "mapped_glass"):
        assert c[k] >= 20, (k, c)
    try:
        p.sp.set_textures(NC.images(wild=True), p.uvs[1:], p.tot[1:])
        p.sp.set_normal_maps(p.nmaps[1:])
        p.sp.set_vertex_normals(p.normals[1:])
        got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(p.sp, p.o4, p.d4, 3)
    finally:
        p.sp.clear_vertex_normals()
        p.sp.set_textures(NC.images(), p.uvs[1:], p.tot[1:])
        p.sp.set_normal_maps(p.nmaps[1:])
    assert_bits_equal(got["color"], pt.color, "the patch at depth 3, wild map, vertex normals")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1 and ctx.stats["slow_paths"] == 0


def test_patch_depth_3_tame_maps(patch):
    p = patch
    pt = _paths(p, 3)
    plain = TR.path_trace(_orc(), p.so, p.o4, p.d4, np.arange(len(p.o4)), np.zeros(len(p.o4), np.int64), 3, SEED, tex=p.tex)
    assert (plain.color != pt.color).any(axis=1).sum() >= 200 and pt.nmap["usem"] >= 500
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(p.sp, p.o4, p.d4, 3)
    assert_bits_equal(got["color"], pt.color, "the patch at depth 3")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1 and ctx.stats["slow_paths"] == 0


def test_patch_with_normals_and_a_sky_all_five_flags_live(patch):
    p = patch
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)
    pt = _paths(p, 4, env=env, normals=p.normals)
    unmapped = TR.path_trace(_orc(), p.so, p.o4, p.d4, np.arange(len(p.o4)), np.zeros(len(p.o4), np.int64), 4, SEED, env=env, normals=p.normals,
                             tex=p.tex)
    assert (unmapped.color != pt.color).any(axis=1).sum() >= 100 and pt.total["refract_in"] >= 10 and (pt.hits0[0] == 0).any()
    try:
        p.sp.set_vertex_normals(p.normals[1:])
        p.sp.set_sky(8, **SUN)
        got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(p.sp, p.o4, p.d4, 4)
    finally:
        p.sp.clear_environment()
        p.sp.clear_vertex_normals()
    assert_bits_equal(got["color"], pt.color, "normal maps, textures, vertex normals, glass and an environment at once")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


def test_patch_with_a_strength_and_through_the_camera(patch):
    p = patch
    nm = NR.maps(p.nmaps, 0.5)
    ref = NR.render(_orc(), p.so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, tex=p.tex, nm=nm)
    try:
        p.sp.set_normal_maps(p.nmaps[1:], strength=0.5)
        img, ctx = _render(p.sp, _vp(2, 5))
    finally:
        p.sp.set_normal_maps(p.nmaps[1:])
    assert_bits_equal(img, ref.image, "the patch through the camera, strength 0.5")
    _assert_stats(ctx, ref)


def test_maps_alone_on_untextured_triangles(patch):
    p = patch
    so, sp = GC.build_pair(NC.recipe_patch())
    tot = np.zeros_like(p.tot)
    sp.set_textures(NC.images(), p.uvs[1:], tot[1:])
    sp.set_normal_maps(p.nmaps[1:])
    tex = TR.textures(NC.images(), p.uvs, tot)
    pt = _paths(p, 3, tex=tex)
    assert pt.tex["untextured"] >= 1000 and pt.tex["matte"] == 0 and pt.nmap["usem"] >= 500
    got, ctx = _R().HipRayCaster(seed=SEED).walk_rays_explicit(sp, p.o4, p.d4, 3, color=True, albedo=True)
    assert_bits_equal(got["color"], pt.color, "maps and no colour texture")
    flat = TR.features(_orc(), so, None, tex, 0, 0, None, 1, SEED, rays=(p.o4, p.d4, len(p.o4), 1))
    assert_bits_equal(got["albedo"], flat[0], "the colour is the material's, bit for bit")
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


def test_table_read_back(patch, teapot):
    p = patch
    c = _R().HipRayCaster(seed=SEED)
    recs = p.so.triangles()[0]
    fr = NR.frames(recs[:, 20:29], p.uvs, recs[:, 3:6], p.nmaps)
    nm, strength = c.normal_maps(p.sp)
    assert p.nmaps[NC.COLLINEAR_TRI] and p.nmaps[TC.SLIVER_TRI] and nm[NC.COLLINEAR_TRI] == 0 and nm[TC.SLIVER_TRI] == 0
    assert np.array_equal(nm, fr.nmap) and strength == 1.0
    so, sp, tex, m = teapot
    nm, strength = c.normal_maps(sp)
    rec = so.triangles()[0]
    assert np.array_equal(nm, NR.frames(rec[:, 20:29], tex.uvs, rec[:, 3:6], m.nmap_of_tri).nmap) and (nm[1:1 + NTEAPOT] == 2).all()
    images, uvs, tot = c.textures(sp)
    assert_bits_equal(images[1], tex.images[1], "the map's texels: normal_map_from_height against the restatement")
    assert_bits_equal(uvs, tex.uvs, "the uvs")


# ---------------------------------------------------------------- the teapot through every call
def test_teapot_host_variant(teapot):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
    assert ref.pt.nmap["usem"] >= 1000 and ref.pt.nmap["unmapped"] >= 100 and ref.pt.nmap["away_from_ray"] >= 1
    plain = TR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, SPP, SEED, MAXDEPTH, tex=tex)
    assert (plain.image != ref.image).any(axis=2).mean() > 0.05
    img, ctx = _render(sp, _vp())
    assert_bits_equal(img, ref.image, "teapot, rtmi_render")
    _assert_stats(ctx, ref)
    assert ctx.stats["trace_launches"] == MAXDEPTH


def test_device_variant_on_a_striped_tile(teapot):
    import torch
    so, sp, tex, nm = teapot
    tile = (1, 12, 3, 8)  # rows 1-3, 9-11, 17-19, 25-27
    ref = _ref(so, tex, nm, tile=tile)
    buf = torch.full((12 * W * 4 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx = _R().HipRayCaster(seed=SEED).walk_tile_device(_vp(), sp, tile, buf[64:].data_ptr())
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[:64] == 7.5).all() and (g[64 + 12 * W * 4:] == 7.5).all()
    assert_bits_equal(g[64:64 + 12 * W * 4].reshape(12, W, 4), ref.image, "teapot, striped tile")
    _assert_stats(ctx, ref)


def test_progressive_passes_end_in_the_bits_of_one_call(teapot):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_progressive(_vp(), sp, img, pass_samples=1)
    assert_bits_equal(img, ref.image, "four passes of one sample")
    assert ctx.samples_done == SPP and ctx.total_rays == ref.rays and ctx.stats["pipeline"] == 1


def test_adaptive_without_a_tolerance_is_the_uniform_render(teapot):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_rays_adaptive(_vp(), sp, img, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(img, ref.image, "adaptive, abs_tol = NaN")
    assert (ctx.counts == SPP).all() and ctx.total_rays == ref.rays


def test_views_of_two_cameras_with_two_seeds(teapot):
    R = _R()
    so, sp, tex, nm = teapot
    c = dict(GC.SIDE_VIEW, pos=(0.5, 1.0, 1.5), aim=(0.1, -0.1, 1.0))
    vs = _orc().create_viewport(W, H, c["size"], np.array(c["pos"], F32), _orc().unit(list(c["aim"])), 70.0, _orc().to_radians(0.0))
    views = [_vp(), R.Viewport(W, H, vs, MAXDEPTH, SPP)]
    ctx = R.HipRayCaster(seed=SEED).walk_rays_views(views, sp, seeds=[SEED, SEED + 1])
    assert_bits_equal(ctx.data[0], _ref(so, tex, nm).image, "view 0")
    assert_bits_equal(ctx.data[1], _ref(so, tex, nm, vp12=vs, seed=SEED + 1).image, "view 1")
    assert ctx.stats["pipeline"] == 1


def test_frame_multi_on_two_handles_of_one_device(teapot):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
    img = np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED, devices=[0, 0]).walk_frame_multi(_vp(), sp, img, stripe_rows=4)
    assert_bits_equal(img, ref.image, "rtmi_render_frame_multi: both handles carry the maps")
    assert ctx.total_rays == ref.rays and all(d["pipeline"] == 1 for d in ctx.per_device)


def test_explicit_rays_of_the_camera_with_their_keys_equal_the_render(teapot):
    import torch
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
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


def test_bake_gathers_light_over_mapped_surfaces(teapot):
    orc = _orc()
    so, sp, tex, nm = teapot
    c = _R().HipRayCaster(seed=SEED)
    pos = np.array([[0.0, 2.5, 5.0, 0], [-2.0, 0.5, 4.0, 0], [3.0, 2.0, 6.0, 0]], F32)
    nrm4 = RR.vunit(np.array([[0.05, -1, 0.1, 0], [1, 0.1, 0.3, 0], [-0.4, -0.5, -0.2, 0]], F32))
    K, depth, pixel0 = 32, 5, 7
    params = c.bake_params("points", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = c.bake(sp, pos, nrm4, params, light=True, orig=True, dir=True)
    pt = NR.path_trace(orc, so, got["orig"], got["dir"], pixel0 + np.repeat(np.arange(3), K), np.tile(np.arange(K), 3), depth, SEED, tex=tex, nm=nm)
    assert_bits_equal(got["light"], RR.fold(pt.color, K), "bake against the restatement")
    assert ctx.total_rays == pt.rays and ctx.stats["pipeline"] == 1 and pt.nmap["usem"] >= 10


def test_thin_lens_camera_with_guides(teapot):
    from rust_raytrace_amd import _ffi
    orc = _orc()
    so, sp, tex, nm = teapot
    cr = CR.camera_rays(orc, orc.canonical_viewport(W, H), W, H, 2, SEED, CR.cam(CR.THIN_LENS, 0.05, 4.0))
    pt = NR.path_trace(orc, so, cr.o4, cr.d4, cr.keys[:, 0], cr.keys[:, 1], 5, SEED, tex=tex, nm=nm)
    acc, want = CR.fold(pt.color, cr.npix, cr.n)
    alb, gn, ids = NR.features(orc, so, None, tex, nm, W, H, None, 2, SEED, rays=(cr.o4, cr.d4, cr.npix, cr.n))
    accum, img = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    ctx = _R().HipRayCaster(seed=SEED).walk_samples_camera(_vp(2, 5), sp, 0, H, _ffi.Camera(CR.THIN_LENS, 0, 0.05, 4.0), 0, 2, accum, img,
                                                           albedo=True, normal=True, ids=True)
    assert_bits_equal(img, want.reshape(H, W, 4), "thin lens: out")
    assert_bits_equal(accum, acc.reshape(H, W, 4), "thin lens: accum")
    assert_bits_equal(ctx.albedo.reshape(H, W, 4), alb.reshape(H, W, 4), "thin lens: the albedo guide")
    assert_bits_equal(ctx.normal.reshape(H, W, 4), gn.reshape(H, W, 4), "thin lens: the normal guide")
    assert np.array_equal(ctx.ids.reshape(H, W), ids.reshape(H, W))
    assert ctx.stats["rays"] == pt.rays and ctx.stats["pipeline"] == 1


def test_features_normal_plane(teapot):
    so, sp, tex, nm = teapot
    vo = _orc().canonical_viewport(W, H)
    alb, nrm, ids = NR.features(_orc(), so, None, tex, nm, W, H, vo, 2, SEED)
    plain = TR.features(_orc(), so, None, tex, W, H, vo, 2, SEED)
    assert (plain[1] != nrm).any(axis=2).mean() > 0.05 and (plain[1][..., 3] == nrm[..., 3]).all()  # depth does not move
    a, n, i, ctx = _R().HipRayCaster(seed=SEED).walk_rays_features(_vp(2, 5), sp)
    assert_bits_equal(n, nrm, "the normal plane")
    assert_bits_equal(a, alb, "the albedo plane")
    assert_bits_equal(a, plain[0], "the albedo plane is the unmapped scene's")
    assert np.array_equal(i, ids)


def test_denoised_wrapper_end_to_end(teapot):
    so, sp, tex, nm = teapot
    c = _R().HipRayCaster(seed=SEED)
    vp = _vp(2, 5)
    img = np.zeros((H, W, 4), F32)
    c.walk_rays(vp, sp, img)
    a, n, _, _ = c.walk_rays_features(vp, sp, ids=False)
    assert_bits_equal(img, _ref(so, tex, nm, spp=2, maxdepth=5).image, "the noisy image")
    assert_bits_equal(n, NR.features(_orc(), so, None, tex, nm, W, H, _orc().canonical_viewport(W, H), 2, SEED)[1], "the mapped guide")
    want = c.denoise(img, a, n)
    got = np.zeros((H, W, 4), F32)
    ctx = c.walk_rays_denoised(vp, sp, got)
    assert_bits_equal(got, want, "rtmi_render_denoised = denoise(render, features) with the mapped normal guide")
    assert ctx.stats["pipeline"] == 1


def test_adaptive_denoised_wrapper_end_to_end(teapot):
    from test_denoise_var import _adaptive_frame
    so, sp, tex, nm = teapot
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    f = _adaptive_frame(R, c, sp, W, H, SPP, 2, 1, None, float("nan"), depth=MAXDEPTH)
    assert_bits_equal(f["color"], _ref(so, tex, nm).image, "the adaptive render")
    assert_bits_equal(f["normal"], NR.features(_orc(), so, None, tex, nm, W, H, _orc().canonical_viewport(W, H), SPP, SEED, nsamples=2)[1],
                      "the guide of the first two samples")
    want = c.denoise_var(f["color"], f["albedo"], f["normal"], f["var"])
    got = np.full((H, W, 4), np.nan, F32)
    ctx = c.walk_rays_adaptive_denoised(f["vp"], sp, got, min_samples=2, pass_samples=1, abs_tol=float("nan"))
    assert_bits_equal(got, want, "rtmi_render_adaptive_denoised = its four calls")
    assert ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- scene kinds and options
def test_linear_list_scene():
    so, sp = CT.build_pair(CT.recipe_canonical(accel="trivial"))
    _map_the_teapot(sp)
    tex, nm = _teapot_inputs(so)
    ref = NR.render(_orc(), so, _orc().canonical_viewport(16, 16), 16, 16, 1, SEED, 4, tex=tex, nm=nm)
    img, ctx = _render(sp, _vp(1, 4, 16, 16))
    assert_bits_equal(img, ref.image, "linear list")
    _assert_stats(ctx, ref)


def test_generic_tree(teapot):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm, spp=2, maxdepth=5)
    img, ctx = _render(sp, _vp(2, 5), options=_R().OPT_GENERIC)
    assert_bits_equal(img, ref.image, "RTMI_OPT_GENERIC")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("tuning", [dict(streams=3, batch_paths=600, subtile_min_paths=1), dict(streams=1, batch_paths=500)])
def test_tuning_changes_no_bit(teapot, tuning):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm)
    img, ctx = _render(sp, _vp(), tuning=tuning)
    assert_bits_equal(img, ref.image, f"tuning {tuning}")
    _assert_stats(ctx, ref)


@pytest.mark.parametrize("maxdepth", [0, 1, 2])
def test_shallow_depths(teapot, maxdepth):
    so, sp, tex, nm = teapot
    ref = _ref(so, tex, nm, spp=2, maxdepth=maxdepth)
    img, ctx = _render(sp, _vp(2, maxdepth))
    assert_bits_equal(img, ref.image, f"maxdepth {maxdepth}")
    assert ctx.stats["rays"] == ref.rays
    if maxdepth == 0:
        assert not img.any()


# ---------------------------------------------------------------- setting and clearing
def test_set_replace_and_clear_returns_the_exact_earlier_images_and_pipeline(teapot):
    orc, R = _orc(), _R()
    so, tsp, tex, nm = teapot
    _, sp = CT.build_pair(CT.recipe_canonical())
    c = R.HipRayCaster(seed=SEED)
    assert sp.normal_maps() is None and c.normal_maps(sp) is None
    _map_the_teapot(sp)
    sp.set_normal_maps(np.full(NTEAPOT, 1, np.uint32), strength=3.0)  # the colour texture as a map
    first, fctx = _render(sp, _vp(2, 5))
    assert fctx.stats["pipeline"] == 1
    sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))  # replaced
    img, ctx = _render(sp, _vp(2, 5))
    assert_bits_equal(img, _ref(so, tex, nm, spp=2, maxdepth=5).image, "replaced")
    assert (first != img).any() and c.normal_maps(sp)[1] == 1.0
    sp.clear_normal_maps()
    assert sp.normal_maps() is None and c.normal_maps(sp) is None
    img, ctx = _render(sp, _vp(2, 5))
    want = TR.render(orc, so, orc.canonical_viewport(W, H), W, H, 2, SEED, 5, tex=tex)
    assert_bits_equal(img, want.image, "maps cleared: the textured image of the _tex kernels")
    assert ctx.stats["pipeline"] == 1 and ctx.stats["rays"] == want.rays
    sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))
    sp.clear_textures()
    assert sp.normal_maps() is None and c.normal_maps(sp) is None and c.textures(sp) is None
    img, ctx = _render(sp, _vp(2, 5))
    plain, cn = so.render(W, H, orc.canonical_viewport(W, H), 5, 2, seed=SEED, threads=4)
    assert_bits_equal(img, plain, "textures cleared as well: the oracle's bits")
    assert ctx.stats["pipeline"] == 3 and ctx.stats["rays"] == cn["rays"]


# ---------------------------------------------------------------- refusals
def test_set_textures_drops_the_maps_on_the_device(teapot):
    so, _, tex, nm = teapot
    _, sp = CT.build_pair(CT.recipe_canonical())
    c = _R().HipRayCaster(seed=SEED)
    _map_the_teapot(sp)
    assert c.normal_maps(sp) is not None
    sp.set_textures(tex.images, None, None)  # the same images again: the uvs stay, the maps go
    assert sp.normal_maps() is None and c.normal_maps(sp) is None
    img = np.zeros((H, W, 4), F32)
    ctx = c.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, TR.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, 2, SEED, 5, tex=tex).image, "textured, unmapped")
    assert ctx.stats["pipeline"] == 1
    # new uvs keep the maps, and the device's frames follow them
    sp.set_normal_maps(np.full(NTEAPOT, 2, np.uint32))
    sp.project_uvs(1, NTEAPOT, LO, SCALE, 1)
    ctx = c.walk_rays(_vp(2, 5), sp, img)
    assert_bits_equal(img, _ref(so, tex, nm, spp=2, maxdepth=5).image, "the uvs set again: the maps are applied again")


def test_bad_arguments_are_refused_by_the_abi_and_the_handle_stays_usable():
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
        tot = np.full(n, 1, np.uint32)
        imgs = [TC.images()[2], NC.tame_maps()[3]]
        nm = np.full(n, 2, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        arr = (_ffi.Texture * 2)()
        for k, a in enumerate(imgs):
            arr[k] = _ffi.Texture(a.ctypes.data, a.shape[1], a.shape[0], 0)
        cnt, st = C.c_uint64(9), C.c_float(9)
        bad = lambda *a: L.rtmi_scene_set_normal_maps(h, *a) == RAW.RTMI_ERR_INVALID
        assert bad(p(corners), p(nm), n, None) and b"no textures" in L.rtmi_last_error()
        assert L.rtmi_scene_set_textures(h, arr, 2, p(corners), p(uvs), p(tot), n) == RAW.RTMI_OK, L.rtmi_last_error()
        assert bad(p(corners), p(nm), n - 1, None) and b"ntris" in L.rtmi_last_error()
        assert bad(None, p(nm), n, None)
        assert bad(p(corners), p(nm), n, C.byref(_ffi.NormalMaps(1.0, 1))) and b"flags" in L.rtmi_last_error()
        for v in (float("nan"), float("inf")):
            assert bad(p(corners), p(nm), n, C.byref(_ffi.NormalMaps(v, 0))) and b"strength" in L.rtmi_last_error()
            z = corners.copy()
            z[1, 4] = v
            assert bad(p(z), p(nm), n, None) and b"corner" in L.rtmi_last_error()
        x = nm.copy()
        x[n - 1] = 3
        assert bad(p(corners), p(x), n, None) and b"above ntex" in L.rtmi_last_error()
        assert L.rtmi_scene_get_normal_maps(h, None, C.byref(st), C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0  # nothing left behind
        assert L.rtmi_scene_get_normal_maps(h, None, None, None) == RAW.RTMI_ERR_INVALID
        # set, read back, render, remove through the raw ABI; entry 0 and unmapped triangles may hold anything
        z, x = corners.copy(), nm.copy()
        z[0], x[0] = float("inf"), 77
        x[2] = 0
        z[2] = float("nan")
        assert L.rtmi_scene_set_normal_maps(h, p(z), p(x), n, C.byref(_ffi.NormalMaps(0.8, 0))) == RAW.RTMI_OK, L.rtmi_last_error()
        back = np.full(n, 9, np.uint32)
        assert L.rtmi_scene_get_normal_maps(h, p(back), C.byref(st), C.byref(cnt)) == RAW.RTMI_OK and cnt.value == n
        x[0] = 0
        assert np.array_equal(back, NR.frames(corners, uvs, rec[:, 3:6], x).nmap) and abs(st.value - 0.8) < 1e-7
        w = 8
        vo = _orc().canonical_viewport(w, w)
        got, stats = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        tex = TR.textures(imgs, uvs, tot)
        assert_bits_equal(got, NR.render(_orc(), so, vo, w, w, 1, SEED, 3, tex=tex, nm=NR.maps(x, F32(0.8))).image, "raw ABI, mapped")
        assert stats.pipeline == 1
        assert L.rtmi_scene_set_normal_maps(h, None, None, 0, None) == RAW.RTMI_OK
        assert L.rtmi_scene_get_normal_maps(h, None, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0
        got, stats = RAW._render(L, ffi, h, vo, w, w, 3, 1, SEED)
        assert_bits_equal(got, TR.render(_orc(), so, vo, w, w, 1, SEED, 3, tex=tex).image, "raw ABI, the maps removed")
        assert L.rtmi_scene_set_normal_maps(h, p(corners), p(nm), n, None) == RAW.RTMI_OK
        assert L.rtmi_scene_set_textures(h, arr, 2, p(corners), p(uvs), p(tot), n) == RAW.RTMI_OK  # replaced: the maps are gone
        assert L.rtmi_scene_get_normal_maps(h, None, None, C.byref(cnt)) == RAW.RTMI_OK and cnt.value == 0
    finally:
        L.rtmi_scene_destroy(h)
