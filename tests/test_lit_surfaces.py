"""-m gpu: box lights on shaded surfaces (RTMI_LIT_SURFACES: rtmi_render_lit*, rtmi_render_rays_lit*, rtmi_bake_lit* on scenes with
a dielectric, vertex normals, textures and normal maps), every float bit for bit against tests/lit_surfaces_ref.py, the float32 NumPy
restatement of include/rtmi.h on the oracle's closest hits, records and RNG (tests/test_lit_surfaces_cpu.py pins it, holds it against
a float64 referee and confirms the case mix of these recipes), so no expected value comes from the code under test.  Three groups
need no restatement: degenerate tables against the old kernels on the bare scene, the flag on unfeatured scenes, and the refusals.
The recipes are tests/lit_surfaces_cases.py's.  The references are computed once per case and shared."""
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import bake_lit_ref as BL
import env_ref as ER
import glass_cases as GC
import lit_ref as LT
import lit_surfaces_cases as LC
import lit_surfaces_ref as LS
import nmap_cases as NC
import tex_cases as TC

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED = LC.SEED
AB, FOUR = LC.AB, LC.FOUR
FULL = None  # tile: the whole frame through the host variant
TILE = (1, 12, 3, 8)
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.8, sun_color=(30.0, 24.0, 16.0))
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _sky():
    return SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)


@pytest.fixture(scope="module")
def teapot():
    """The canonical scene in its octree with the featured teapot"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    LC.feature_teapot(_R(), sp)
    return so, sp, LC.teapot_inputs(so)


@pytest.fixture(scope="module")
def patch():
    so, sp = GC.build_pair(NC.recipe_patch())
    p = LC.patch_inputs(so)
    LC.feature_patch(sp, p)
    return so, sp, p


def _ref(so, f, lights, vo, w, h, spp, depth, inverse_square=False, env=None, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it).  f: the scene's normals, tex, nm"""
    key = (id(so), id(f), str(lights), np.asarray(vo, F32).tobytes(), w, h, spp, depth, inverse_square, bool(env),
           tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = LS.render(_orc(), so, vo, w, h, spp, SEED, depth, lights, inverse_square, _sky() if env else None,
                               getattr(f, "normals", None), getattr(f, "tex", None), getattr(f, "nm", None), **kw)
    return _REFS[key]


def _render(c, sp, vo, w, h, spp, depth, lights, inverse_square=False, surfaces=True, tile=FULL, sample0=0, nsamples=None, accum=None):
    """(image (rows, w, 4), accum, stats) of one call: the host variant for the whole frame, the device variant on torch tensors
    with guard floats for a tile"""
    vp = _R().Viewport(w, h, vo, depth, spp)
    lit = c.lit_params(lights, inverse_square, surfaces=surfaces)
    if tile is FULL:
        img, ctx = c.walk_rays_lit(vp, sp, lit, accum=accum, sample0=sample0, nsamples=nsamples)
        return img, ctx.accum, ctx.stats
    import torch
    n = tile[1] * w * 4
    bufs = [torch.full((n + 128,), 7.5, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    if accum is not None:
        bufs[0][64:64 + n] = torch.from_numpy(np.ascontiguousarray(accum, F32).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_lit_device(vp, sp, lit, bufs[0][64:64 + n], bufs[1][64:64 + n], tile=tile, sample0=sample0, nsamples=nsamples)
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        g = b.cpu().numpy()
        assert (g[:64] == 7.5).all() and (g[64 + n:] == 7.5).all(), "guard floats"
        out.append(g[64:64 + n].reshape(tile[1], w, 4))
    return out[1], out[0], ctx.stats


def _check(c, ref, sp, vo, w, h, spp, depth, lights, what, **kw):
    """One call against the restatement: the image, the sums, stats.rays and the launch bookkeeping"""
    img, acc, st = _render(c, sp, vo, w, h, spp, depth, lights, **kw)
    assert_bits_equal(img, ref.image, f"{what}: image")
    assert_bits_equal(acc, ref.accum, f"{what}: accum")
    assert st["rays"] == ref.rays + ref.nlive, f"{what}: rays {st['rays']} vs {ref.rays} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0
    assert st["trace_launches"] >= 2 * depth and st["trace_launches"] % (2 * depth) == 0
    return st


def _both_variants(c, so, sp, f, vo, w, h, spp, depth, lights, what, **kw):
    """The host variant and the device variant (the whole frame as a tile), without and with an environment"""
    for env in (False, True):
        ref = _ref(so, f, lights, vo, w, h, spp, depth, env=env, **{k: v for k, v in kw.items() if k == "inverse_square"})
        try:
            if env:
                sp.set_sky(8, **SUN)
            _check(c, ref, sp, vo, w, h, spp, depth, lights, f"{what}, env={env}, host", **kw)
            _check(c, ref, sp, vo, w, h, spp, depth, lights, f"{what}, env={env}, device", tile=(0, h, h, 0), **kw)
        finally:
            if env:
                sp.clear_environment()
    return ref


# ---------------------------------------------------------------- the frame pass against the restatement
@pytest.mark.parametrize("depth", LC.PATCH["depths"])
def test_patch(patch, depth):
    so, sp, p = patch
    c = LC.PATCH
    ref = _both_variants(_R().HipRayCaster(seed=SEED), so, sp, p, LC.patch_view(_orc()), c["w"], c["h"], c["spp"], depth, AB, f"patch, depth {depth}")
    assert (ref.nlive > 100) == (depth > 1)


def test_teapot_on_the_octree(teapot):
    so, sp, t = teapot
    c = LC.TEAPOT
    vo = _orc().canonical_viewport(c["w"], c["h"])
    ref = _both_variants(_R().HipRayCaster(seed=SEED), so, sp, t, vo, c["w"], c["h"], c["spp"], c["depth"], AB, "teapot, octree")
    bare = LT.render(_orc(), so, vo, c["w"], c["h"], c["spp"], SEED, c["depth"], AB)
    assert ref.nlive > 500 and not np.array_equal(bare.image, ref.image)


def test_teapot_as_a_linear_list():
    so, sp = CT.build_pair(CT.recipe_canonical(accel="trivial", obj=CT.TEAPOT))
    n = len(so.triangles()[0]) - 1
    # (this teapot file has its own triangle count: every triangle gets the teapot's treatment)
    rec = so.triangles()[0]
    import nmap_ref as NR
    import smooth_ref as SR
    import tex_ref as TR
    uvs, tot, nm = np.zeros((n + 1, 3, 2), F32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    uvs[1:] = TR.project(rec[1:, 20:29], rec[1:, 3:6], LC.LO, LC.SCALE)
    tot[1:], nm[1:] = 1, 2
    nrm = np.zeros((n + 1, 3, 3), F32)
    nrm[1:] = SR.generate(rec[1:, 20:29], rec[1:, 3:6], LC.CREASE)
    f = SimpleNamespace(normals=nrm, tex=TR.textures([TC.images()[3], NR.from_height(NC.heights(), LC.HEIGHT_SCALE)], uvs, tot), nm=NR.maps(nm))
    sp.smooth_normals(1, n, LC.CREASE)
    sp.set_textures([TC.images()[3], _R().normal_map_from_height(NC.heights(), LC.HEIGHT_SCALE)], None, None)
    sp.project_uvs(1, n, LC.LO, LC.SCALE, 1)
    sp.set_normal_maps(np.full(n, 2, np.uint32))
    ref = _both_variants(_R().HipRayCaster(seed=SEED), so, sp, f, _orc().canonical_viewport(16, 16), 16, 16, 2, 3, AB, "teapot, linear list")
    assert ref.nlive > 50 and LS.total(ref.pt, "differs") > 50


def test_striped_tile(teapot):
    so, sp, t = teapot
    c = LC.TEAPOT
    vo = _orc().canonical_viewport(c["w"], c["h"])
    ref = _ref(so, t, AB, vo, c["w"], c["h"], c["spp"], c["depth"], tile=TILE)
    assert ref.nlive > 100
    _check(_R().HipRayCaster(seed=SEED), ref, sp, vo, c["w"], c["h"], c["spp"], c["depth"], AB, f"tile {TILE}", tile=TILE)


@pytest.mark.parametrize("tile", [FULL, (0, 32, 32, 0)], ids=["host", "device"])
def test_two_calls_of_half_the_samples_each(teapot, tile):
    so, sp, t = teapot
    c = LC.TEAPOT
    vo = _orc().canonical_viewport(c["w"], c["h"])
    ref = _ref(so, t, AB, vo, c["w"], c["h"], c["spp"], c["depth"])
    caster = _R().HipRayCaster(seed=SEED)
    acc, img = None, None
    for s0, n in ((0, 2), (2, 2)):
        img, acc, _ = _render(caster, sp, vo, c["w"], c["h"], c["spp"], c["depth"], AB, sample0=s0, nsamples=n, tile=tile, accum=acc)
    assert_bits_equal(img, ref.image, "passes [0,2) [2,4): out")
    assert_bits_equal(acc, ref.accum, "passes [0,2) [2,4): accum")


def test_three_streams_and_batches_of_600_paths(teapot):
    so, sp, t = teapot
    c = LC.TEAPOT
    R = _R()
    vo = _orc().canonical_viewport(c["w"], c["h"])
    try:
        st = _check(R.HipRayCaster(seed=SEED, tuning=dict(streams=3, batch_paths=600, subtile_min_paths=1)),
                    _ref(so, t, AB, vo, c["w"], c["h"], c["spp"], c["depth"]), sp, vo, c["w"], c["h"], c["spp"], c["depth"], AB,
                    "3 streams, batches of 600")
        assert st["streams"] == 3 and st["trace_launches"] >= 2 * c["depth"] * 3 * 2
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


def test_a_frame_whose_count_is_no_multiple_of_256(teapot):
    so, sp, t = teapot
    vo = _orc().canonical_viewport(19, 13)
    ref = _ref(so, t, AB, vo, 19, 13, 3, 4)
    assert (19 * 13 * 3) % 256 != 0 and all(p % 256 != 0 for p in ref.passes if p) and ref.nlive > 50
    _check(_R().HipRayCaster(seed=SEED), ref, sp, vo, 19, 13, 3, 4, AB, "19 x 13, spp 3")


def test_four_lights_one_unbounded_inverse_square(teapot):
    so, sp, t = teapot
    c = LC.TEAPOT
    vo = _orc().canonical_viewport(c["w"], c["h"])
    ref = _ref(so, t, FOUR, vo, c["w"], c["h"], c["spp"], c["depth"], inverse_square=True)
    assert all(ref.pt.live[0][l] > 0 for l in range(4)) and ref.nlive > 1500
    _check(_R().HipRayCaster(seed=SEED), ref, sp, vo, c["w"], c["h"], c["spp"], c["depth"], FOUR, "four lights, inverse square", inverse_square=True)


# ---------------------------------------------------------------- against the old kernels
def test_degenerate_tables_give_the_old_kernels_bits():
    """Nine-zero normals, all-ones textures and no maps on the canonical scene: with the flag the new kernels run, and the image
    is the old kernels' on the bare scene without the flag"""
    R = _R()
    _, bare = CT.build_pair(CT.recipe_canonical())
    so, sp = CT.build_pair(CT.recipe_canonical())
    n = len(so.triangles()[0]) - 1
    sp.set_vertex_normals(np.zeros((n, 3, 3), F32))
    sp.set_textures([np.ones((8, 8, 3), F32)], None, None)
    sp.project_uvs(1, LC.NTEAPOT, LC.LO, LC.SCALE, 1)
    c = R.HipRayCaster(seed=SEED)
    vo = _orc().canonical_viewport(32, 32)
    for lights, inv in ((AB, False), (FOUR, True)):
        want, wacc, wst = _render(c, bare, vo, 32, 32, 4, 4, lights, inv, surfaces=False, tile=(0, 32, 32, 0))
        got, gacc, gst = _render(c, sp, vo, 32, 32, 4, 4, lights, inv, tile=(0, 32, 32, 0))
        assert_bits_equal(got, want, "degenerate tables: image")
        assert_bits_equal(gacc, wacc, "degenerate tables: accum")
        assert gst["rays"] == wst["rays"]
    with pytest.raises(RuntimeError, match="vertex normals"):  # (the featured scene did run the new path: without the flag it is refused)
        _render(c, sp, vo, 32, 32, 4, 4, AB, surfaces=False)


def test_the_flag_on_an_unfeatured_scene_changes_no_bit_and_no_stat():
    so, sp = CT.build_pair(CT.recipe_canonical())
    c = _R().HipRayCaster(seed=SEED)
    vo = _orc().canonical_viewport(32, 32)
    for env in (False, True):
        if env:
            sp.set_sky(8, **SUN)
        ref = LT.render(_orc(), so, vo, 32, 32, 4, SEED, 4, AB, env=_sky() if env else None)
        for tile in (FULL, TILE):
            r = ref if tile is FULL else LT.render(_orc(), so, vo, 32, 32, 4, SEED, 4, AB, env=_sky() if env else None, tile=TILE)
            a = _render(c, sp, vo, 32, 32, 4, 4, AB, surfaces=False, tile=tile)
            b = _render(c, sp, vo, 32, 32, 4, 4, AB, surfaces=True, tile=tile)
            assert_bits_equal(b[0], a[0], f"env={env}: image with and without the flag")
            assert_bits_equal(b[0], r.image, f"env={env}: image against lit_ref")
            assert_bits_equal(b[1], a[1], f"env={env}: accum")
            for k in ("rays", "trace_launches", "pipeline", "slow_paths", "streams"):
                assert a[2][k] == b[2][k], k
            assert b[2]["rays"] == r.rays + r.nlive


# ---------------------------------------------------------------- glass, and scenes with one feature
def test_glass_slab_with_a_lamp_behind_it():
    so, sp = GC.build_pair(GC.recipe_slab(accel="trivial"))
    c = LC.SLAB
    vo = _orc().canonical_viewport(c["w"], c["h"])
    f = SimpleNamespace()
    ref = _ref(so, f, [LC.SLAB_LAMP], vo, c["w"], c["h"], c["spp"], c["depth"], keep=True)
    assert ref.pt.kinds[0]["glass"] > 20 and LS.total(ref.pt, "occluded") >= 20 and LS.total(ref.pt, "visible") >= 20
    for j in range(c["depth"] - 1):  # every candidate whose segment crosses the slab is occluded
        cd = ref.pt.cand[j][0]
        lamp = cd["o"][:, :3].astype(np.float64) + cd["dir"][:, :3].astype(np.float64) * cd["r"][:, None].astype(np.float64)
        cross = LC.crosses_slab(cd["o"][:, :3], lamp, shrink=1e-3)[cd["live"]]
        assert (cd["occ"][cross] != 0).all()
    _both_variants(_R().HipRayCaster(seed=SEED), so, sp, f, vo, c["w"], c["h"], c["spp"], c["depth"], [LC.SLAB_LAMP], "glass slab")
    so, sp = GC.build_pair(GC.recipe_slab())
    ref = _ref(so, f, [LC.SLAB_LAMP], vo, c["w"], c["h"], c["spp"], c["depth"])
    _check(_R().HipRayCaster(seed=SEED), ref, sp, vo, c["w"], c["h"], c["spp"], c["depth"], [LC.SLAB_LAMP], "glass slab in its octree")


@pytest.mark.parametrize("only", ["normals", "textures", "maps"])
def test_scenes_with_only_one_feature(only):
    """The empty-table paths of the one kernel set.  The patch has glass among its kinds whatever else is set."""
    so, sp = GC.build_pair(NC.recipe_patch())
    p = LC.patch_inputs(so)
    LC.feature_patch(sp, p, normals=only == "normals", textures=only == "textures", maps=only == "maps")
    import tex_ref as TR
    f = SimpleNamespace(normals=p.normals if only == "normals" else None,
                        tex=None if only == "normals" else (p.tex if only == "textures" else TR.textures(NC.images(), p.uvs, np.zeros_like(p.tot))),
                        nm=p.nm if only == "maps" else None)
    c = LC.PATCH
    vo = LC.patch_view(_orc())
    ref = _ref(so, f, AB, vo, c["w"], c["h"], c["spp"], 3)
    full = LS.render(_orc(), so, vo, c["w"], c["h"], c["spp"], SEED, 3, AB, normals=p.normals, tex=p.tex, nm=p.nm)
    assert ref.nlive > 100 and not np.array_equal(ref.image, full.image)
    caster = _R().HipRayCaster(seed=SEED)
    _check(caster, ref, sp, vo, c["w"], c["h"], c["spp"], 3, AB, f"{only} only, host")
    _check(caster, ref, sp, vo, c["w"], c["h"], c["spp"], 3, AB, f"{only} only, device", tile=(0, c["h"], c["h"], 0))


# ---------------------------------------------------------------- explicit rays and the bake
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_explicit_rays_with_the_frames_keys_give_the_frames_bits(teapot):
    import torch
    so, sp, t = teapot
    c = LC.TEAPOT
    vo = _orc().canonical_viewport(c["w"], c["h"])
    ref = _ref(so, t, AB, vo, c["w"], c["h"], c["spp"], c["depth"])
    caster = _R().HipRayCaster(seed=SEED)
    n = len(ref.o4)
    keys = np.ascontiguousarray(np.stack([ref.pixel, ref.sample], axis=1).astype(np.uint32))
    outs = dict(color=torch.full((n, 4), -7.0, device="cuda"), mean=torch.full((n // c["spp"], 4), -7.0, device="cuda"))
    ctx = caster.walk_rays_explicit_lit_device(sp, _dev(ref.o4), _dev(ref.d4), c["depth"], caster.lit_params(AB, surfaces=True), group=c["spp"],
                                               keys=_dev(keys.view(np.int32)), **outs)
    torch.cuda.synchronize()
    assert_bits_equal(outs["color"].cpu().numpy(), ref.color, "explicit rays: the sample colours")
    assert_bits_equal(outs["mean"].cpu().numpy().reshape(c["h"], c["w"], 4), ref.image, "explicit rays: the group means are the frame")
    assert ctx.total_rays == ref.rays + ref.nlive and ctx.stats["trace_launches"] == 2 * c["depth"]
    host, hctx = caster.walk_rays_explicit_lit(sp, ref.o4, ref.d4, c["depth"], caster.lit_params(AB, surfaces=True), group=c["spp"], keys=keys)
    assert_bits_equal(host["color"], ref.color, "explicit rays, host variant")
    assert hctx.total_rays == ref.rays + ref.nlive


def test_bake_on_first_hit_elements_of_the_featured_teapot(teapot):
    import torch
    so, sp, t = teapot
    pos, nrm = BL.elements(_orc(), so)
    K, depth = BL.K, 3
    caster = _R().HipRayCaster(seed=SEED)
    params = caster.bake_params("points", rays=K, maxdepth=depth, pixel0=BL.PIXEL0)
    exp = LS.bake(_orc(), so, SEED, pos, nrm, K, depth, AB, pixel0=BL.PIXEL0, normals=t.normals, tex=t.tex, nm=t.nm)
    M = nrm.shape[0]
    shape = dict(light=(M, 4), open=(M,), orig=(M * K, 4), dir=(M * K, 4), direct=(M, 4))
    outs = {k: torch.full(s, -7.0, device="cuda") for k, s in shape.items()}
    ctx = caster.bake_lit_device(sp, _dev(pos), _dev(nrm), params, caster.lit_params(AB, surfaces=True), **outs)
    torch.cuda.synchronize()
    for k in shape:
        assert_bits_equal(getattr(exp, k), outs[k].cpu().numpy(), f"bake: {k}")
    bare = BL.bake_lit_ref(_orc(), so, SEED, pos, nrm, K, depth, AB, pixel0=BL.PIXEL0)
    assert_bits_equal(exp.direct, bare.direct, "direct keeps the caller's normal: the bare scene's")
    assert not np.array_equal(exp.light, bare.light) and exp.pt.nlive > 20 and LS.total(exp.pt, "differs") > 50 and exp.el.live > 100
    assert ctx.total_rays == exp.rays and ctx.stats["trace_launches"] == 2 * depth + 1
    # direct alone traces no gather ray
    alone = torch.full((M, 4), -7.0, device="cuda")
    ctx = caster.bake_lit_device(sp, _dev(pos), _dev(nrm), params, caster.lit_params(AB, surfaces=True), direct=alone)
    torch.cuda.synchronize()
    assert_bits_equal(alone.cpu().numpy(), exp.direct, "direct alone")
    assert ctx.total_rays == exp.el.live and ctx.stats["trace_launches"] == 1
    host, hctx = caster.bake_lit(sp, pos, nrm, params, caster.lit_params(AB, surfaces=True), light=True, direct=True)
    assert_bits_equal(host["light"], exp.light, "host variant: light")
    assert_bits_equal(host["direct"], exp.direct, "host variant: direct")


# ---------------------------------------------------------------- refusals
def _refused(c, sp, word, surfaces=False):
    import torch
    vp = _R().canonical_viewport(16, 16, 4, 1)
    lit = c.lit_params(AB, surfaces=surfaces)
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_lit(vp, sp, lit)
    acc = torch.zeros(16 * 16 * 4, dtype=torch.float32, device="cuda:0")
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_lit_device(vp, sp, lit, acc)
    assert (acc == 0).all()
    o4, d4 = np.zeros((4, 4), F32), np.tile(np.array([0, 0, 1, 0], F32), (4, 1))
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_explicit_lit(sp, o4, d4, 3, lit)
    with pytest.raises(RuntimeError, match=word):
        c.bake_lit(sp, o4, d4, c.bake_params("points", rays=2, maxdepth=2), lit, direct=True)


def test_without_the_flag_each_featured_scene_is_still_refused_and_the_handle_renders_afterwards(teapot, patch):
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    so, sp, t = teapot
    _refused(c, sp, "vertex normals")
    ct = LC.TEAPOT
    vo = _orc().canonical_viewport(ct["w"], ct["h"])
    _check(c, _ref(so, t, AB, vo, ct["w"], ct["h"], ct["spp"], ct["depth"]), sp, vo, ct["w"], ct["h"], ct["spp"], ct["depth"], AB, "after the refusal")
    so2, sp2 = CT.build_pair(CT.recipe_canonical())
    sp2.set_textures([TC.images()[3]], None, None)
    sp2.project_uvs(1, LC.NTEAPOT, LC.LO, LC.SCALE, 1)
    _refused(c, sp2, "textures")
    sp2.set_normal_maps(np.full(LC.NTEAPOT, 1, np.uint32))
    _refused(c, sp2, "normal maps")
    _refused(c, patch[1], "dielectric")
    _refused(c, GC.build_pair(GC.recipe_slab())[1], "dielectric")


def test_analytic_spheres_are_refused_with_the_flag():
    R = _R()
    spheres = CT.recipe_circles_analytic()(CT.ProductApi(R))
    _refused(R.HipRayCaster(seed=SEED), spheres, "analytic spheres", surfaces=True)
    _refused(R.HipRayCaster(seed=SEED), spheres, "analytic spheres", surfaces=False)
