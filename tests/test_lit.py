"""-m gpu: box lights inside the path trace (rtmi_render_lit / rtmi_render_lit_device; HipRayCaster.walk_rays_lit*) against their
definition, every float bit for bit: tests/lit_ref.py restates include/rtmi.h in NumPy on the oracle's rays, closest hits, triangle
records and RNG (tests/test_lit_cpu.py pins it, holds it against a float64 referee and confirms the conditions these cases rely
on), so no expected value comes from the code under test.  Three tests need no restatement: without lights the call is the plain
progressive pass, at a depth of 1 likewise, and a depth of 0 writes zeros.  The references are computed once per case and shared."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import env_ref as ER
import lit_ref as LT

pytestmark = pytest.mark.gpu
F32 = np.float32
W = H = 32
SPP, SEED, MAXDEPTH = 4, 5, 4
FULL = None  # tile: the whole frame through the host variant
TILE = (1, 12, 3, 8)
AB = (LT.A, LT.B)
SUN = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.95, sun_color=(30.0, 24.0, 16.0))
NTEAPOT = 6320  # triangles 1 .. 6320 of the canonical scene are the teapot's
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


@pytest.fixture(scope="module")
def teapot():
    """The canonical Matte / Reflective scene in its octree, no environment"""
    return CT.build_pair(CT.recipe_canonical())


@pytest.fixture(scope="module")
def teapot_sky():
    """The same scene under the generated sky, n = 16"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_sky(16, **SUN)
    return so, sp, SimpleNamespace(table=ER.sky_table(16, SUN), frame=None)


@pytest.fixture(scope="module")
def teapot_list():
    """The same scene as a linear list"""
    return CT.build_pair(CT.recipe_canonical(accel="trivial", obj=CT.TEAPOT))


def _ref(so, lights, w=W, h=H, spp=SPP, maxdepth=MAXDEPTH, seed=SEED, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), str(lights), w, h, spp, maxdepth, seed, tuple(sorted((k, id(v) if k == "env" else str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = LT.render(_orc(), so, _orc().canonical_viewport(w, h), w, h, spp, seed, maxdepth, lights, **kw)
    return _REFS[key]


def _render(c, sp, lights, inverse_square=False, w=W, h=H, spp=SPP, maxdepth=MAXDEPTH, sample0=0, nsamples=None, tile=FULL, accum=None):
    """(image (rows, w, 4), accum, stats) of one call: the host variant for the whole frame, the device variant on torch tensors
    with guard floats for a tile"""
    vp = _R().canonical_viewport(w, h, maxdepth, spp)
    lit = c.lit_params(lights, inverse_square)
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


def _plain(c, sp, w=W, h=H, spp=SPP, maxdepth=MAXDEPTH):
    """rtmi_render_samples_device of the whole frame: (image, stats)"""
    import torch
    vp = _R().canonical_viewport(w, h, maxdepth, spp)
    acc, out = (torch.zeros(h * w * 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
    ctx = c.walk_samples_device(vp, sp, (0, h, h, 0), 0, spp, acc.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(h, w, 4), ctx.stats


def _check(c, ref, sp, lights, what, **kw):
    """One call against the restatement: the image, the sums, stats.rays and the launch bookkeeping"""
    img, acc, st = _render(c, sp, lights, **kw)
    maxdepth = kw.get("maxdepth", MAXDEPTH)
    assert_bits_equal(img, ref.image, f"{what}: image")
    assert_bits_equal(acc, ref.accum, f"{what}: accum")
    assert st["rays"] == ref.rays + ref.nlive, f"{what}: rays {st['rays']} vs {ref.rays} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0
    assert st["trace_launches"] >= 2 * maxdepth and st["trace_launches"] % (2 * maxdepth) == 0
    assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] >= 0
    return st


# ---------------------------------------------------------------- against the restatement
def test_octree_scene_whole_frame(teapot):
    so, sp = teapot
    ref = _ref(so, AB)
    c = _R().HipRayCaster(seed=SEED)
    st = _check(c, ref, sp, AB, "octree, whole frame, lights A + B")
    plain, pst = _plain(c, sp)
    assert not np.array_equal(plain, ref.image) and st["rays"] - ref.nlive == pst["rays"] == ref.rays


def test_octree_scene_striped_tile(teapot):
    so, sp = teapot
    ref = _ref(so, AB, tile=TILE)
    assert ref.nlive > 100
    _check(_R().HipRayCaster(seed=SEED), ref, sp, AB, f"octree, tile {TILE}", tile=TILE)


def test_four_lights_one_unbounded_one_with_its_own_bias_inverse_square(teapot):
    so, sp = teapot
    ref = _ref(so, LT.FOUR, inverse_square=True)
    assert all(ref.live[0][l] > 0 for l in range(4)) and ref.nlive > 2000  # more live rays than a pass has paths to spare: 4 per path
    _check(_R().HipRayCaster(seed=SEED), ref, sp, LT.FOUR, "four lights, inverse square", inverse_square=True)


def test_linear_list_scene(teapot_list):
    so, sp = teapot_list
    ref = _ref(so, AB, w=16, h=16)
    assert ref.nlive > 100 and sum(sum(x) for x in ref.occluded) > 10
    _check(_R().HipRayCaster(seed=SEED), ref, sp, AB, "linear list", w=16, h=16)


def test_scene_with_an_environment(teapot_sky):
    so, sp, env = teapot_sky
    ref = _ref(so, AB, env=env)
    dark = _ref(so, AB)
    assert ref.nlive == dark.nlive and not np.array_equal(ref.image, dark.image)  # the same candidates under another sky
    _check(_R().HipRayCaster(seed=SEED), ref, sp, AB, "generated sky, n = 16")


@pytest.mark.parametrize("tile", [FULL, TILE], ids=["frame", "tile"])
def test_progressive_continuation_equals_one_call(teapot, tile):
    so, sp = teapot
    c = _R().HipRayCaster(seed=SEED)
    ref = _ref(so, AB) if tile is FULL else _ref(so, AB, tile=TILE)
    acc, img = None, None
    for s0, n in ((0, 2), (2, 2)):
        img, acc, _ = _render(c, sp, AB, sample0=s0, nsamples=n, tile=tile, accum=acc)
    assert_bits_equal(img, ref.image, "passes [0,2) [2,4): out")
    assert_bits_equal(acc, ref.accum, "passes [0,2) [2,4): accum")


def test_several_streams_and_batches_change_no_bit(teapot):
    so, sp = teapot
    R = _R()
    try:
        st = _check(R.HipRayCaster(seed=SEED, tuning=dict(streams=3, batch_paths=600, subtile_min_paths=1)), _ref(so, AB), sp, AB,
                    "3 streams, batches of 600")
        assert st["streams"] == 3 and st["trace_launches"] >= 2 * MAXDEPTH * 3 * 2
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


def test_a_light_far_behind_every_candidate_culled_no_walk_ray(teapot):
    so, sp = teapot
    ref = _ref(so, (LT.FAR_BEHIND,))
    none = _ref(so, ())
    assert ref.nlive == 0 and ref.culled[0][0] == ref.candidates[0][0] > 300
    assert_bits_equal(ref.image, none.image, "the restatement: every candidate culled")
    c = _R().HipRayCaster(seed=SEED)
    st = _check(c, ref, sp, (LT.FAR_BEHIND,), "light far behind")
    _, pst = _plain(c, sp)
    assert st["rays"] == pst["rays"] == ref.rays


def test_odd_size_whose_count_is_no_multiple_of_256(teapot):
    so, sp = teapot
    ref = _ref(so, AB, w=33, h=31, spp=3)
    assert (33 * 31 * 3) % 256 != 0 and all(p % 256 != 0 for p in ref.passes if p) and ref.nlive > 100
    _check(_R().HipRayCaster(seed=SEED), ref, sp, AB, "33 x 31, spp 3", w=33, h=31, spp=3)


# ---------------------------------------------------------------- independent of the restatement
def test_without_lights_the_call_is_the_plain_progressive_pass(teapot):
    so, sp = teapot
    c = _R().HipRayCaster(seed=SEED)
    img, _, st = _render(c, sp, (), tile=(0, H, H, 0))
    plain, pst = _plain(c, sp)
    assert_bits_equal(img, plain, "nlights = 0 against rtmi_render_samples_device")
    assert st["rays"] == pst["rays"] and st["trace_launches"] == 2 * MAXDEPTH * st["streams"]
    _check(c, _ref(so, ()), sp, (), "nlights = 0 against the restatement")


def test_depth_1_is_the_plain_call_and_depth_0_writes_zeros(teapot):
    so, sp = teapot
    c = _R().HipRayCaster(seed=SEED)
    img, _, st = _render(c, sp, AB, maxdepth=1, tile=(0, H, H, 0))
    plain, pst = _plain(c, sp, maxdepth=1)
    assert_bits_equal(img, plain, "depth 1 against rtmi_render_samples_device")
    assert st["rays"] == pst["rays"] == W * H * SPP  # the exhausted level gets no candidate
    for tile in (FULL, TILE):
        img, acc, st = _render(c, sp, AB, maxdepth=0, tile=tile, accum=np.full((H if tile is FULL else TILE[1], W, 4), 3.0, F32))
        assert (img == 0).all() and (acc == 0).all() and st["rays"] == 0


# ---------------------------------------------------------------- refusals
def test_invalid_arguments_are_refused_before_the_scene_is_used():
    LT.check_invalid_arguments()
    c = _R().HipRayCaster
    for bad in (dict(orig=(0, 0, float("nan"))), dict(orig=(0, 0, 0), len2=-1.0), dict(orig=(0, 0, 0), color=(1, float("inf"), 1)),
                dict(orig=(0, 0, 0), rays=2), dict(orig=(0, 0, 0), flags=2), dict(len2=1.0)):
        with pytest.raises(ValueError, match="light 1"):
            c.lit_params([LT.A, bad])
    with pytest.raises(ValueError, match="at most 4"):
        c.lit_params([LT.A] * 5)
    p = c.lit_params([LT.A, dict(LT.B, flags=1)], inverse_square=True)
    assert p.nlights == 2 and p.flags == 1 and p.lights[1].flags == 1 and p.lights[0].rays == 1 and list(p.light_color[1]) == [F32(0.2), F32(0.3), F32(0.5)]


def _refused(c, sp, word):
    import torch
    vp = _R().canonical_viewport(16, 16, MAXDEPTH, 1)
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_lit(vp, sp, AB)
    acc = torch.zeros(16 * 16 * 4, dtype=torch.float32, device="cuda:0")
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_lit_device(vp, sp, AB, acc)
    assert (acc == 0).all()


def test_scenes_the_call_does_not_take_are_refused_and_the_handle_stays_usable():
    import glass_cases as GC
    import tex_cases as TC
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.smooth_normals(1, NTEAPOT)
    _refused(c, sp, "vertex normals")
    sp.clear_vertex_normals()
    sp.set_textures([TC.images()[3]], None, None)
    sp.project_uvs(1, NTEAPOT, (-1.7, -0.4, 3.1), 0.9, 1)
    _refused(c, sp, "textures")
    sp.set_normal_maps(np.full(NTEAPOT, 1, np.uint32))
    _refused(c, sp, "normal maps")
    sp.clear_textures()
    # ... and the same handle renders once the scene is one the call takes: the lit frame, and the plain frame
    _check(c, _ref(so, AB, w=16, h=16, spp=2), sp, AB, "after the refusals", w=16, h=16, spp=2)
    vo = _orc().canonical_viewport(16, 16)
    want, _ = so.render(16, 16, vo, MAXDEPTH, 2, seed=SEED)
    plain, _ = _plain(c, sp, w=16, h=16, spp=2)
    assert_bits_equal(plain, want, "the plain frame after the refusals")
    glass = GC.build_pair(GC.recipe_slab())[1]
    _refused(R.HipRayCaster(seed=SEED), glass, "dielectric")
    spheres = CT.recipe_circles_analytic()(CT.ProductApi(R))
    _refused(R.HipRayCaster(seed=SEED), spheres, "analytic spheres")


def test_a_refused_scene_returns_unsupported_with_cleared_stats_through_the_raw_abi():
    """What the Python layer's exception hides: rc == RTMI_ERR_UNSUPPORTED and stats cleared, for both variants, on a real handle
    with an analytic sphere and then with vertex normals; with both removed the handle renders the plain frame"""
    import test_gpu_abi_raw as RAW
    from test_gpu_abi_raw import Vp, _abi_arrays, _boxes, _create, _lib

    class Sphere(C.Structure):
        _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("surface_kind", C.c_uint32), ("color", C.c_float * 3),
                    ("alpha", C.c_float), ("scattering", C.c_float)]
    orc = _orc()
    L, ffi = _lib()
    L.rtmi_scene_set_spheres.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    so = CT.recipe_circles(maxdepth=4, minobjs=6)(CT.OracleApi(orc))
    tris, geo, topo, refs = _abi_arrays(so)
    rc, hnd = _create(L, tris, _boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    try:
        vp12 = orc.canonical_viewport(8, 8)
        vp = Vp(8, 8, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]), (C.c_float * 3)(*vp12[9:12]), 4, 2)
        acc, out = np.full((8, 8, 4), 3.0, F32), np.full((8, 8, 4), 5.0, F32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lit = _R().HipRayCaster.lit_params(AB)

        def both(word):
            for dev in (False, True):
                st = ffi.Stats()
                st.rays, st.trace_launches = 123, 7
                if dev:  # (refused before the pointers are used: host memory will do)
                    tile = ffi.Tile(0, 8, 8, 0)
                    rc = L.rtmi_render_lit_device(hnd, C.byref(vp), 3, C.byref(tile), 0, 2, C.byref(lit), p(acc), p(out), None, C.byref(st))
                else:
                    rc = L.rtmi_render_lit(hnd, C.byref(vp), 3, 0, 8, 0, 2, C.byref(lit), p(acc), p(out), C.byref(st))
                assert rc == 3 and word in L.rtmi_last_error(), (rc, L.rtmi_last_error())  # RTMI_ERR_UNSUPPORTED
                assert st.rays == 0 and st.trace_launches == 0 and st.kernel_ms == 0
            assert (acc == 3.0).all() and (out == 5.0).all()
        sph = Sphere((C.c_float * 3)(0.0, 0.5, 5.0), 0.5, 0, (C.c_float * 3)(1.0, 0.0, 0.0), 0.0, 0.0)
        assert L.rtmi_scene_set_spheres(hnd, C.byref(sph), 1) == 0, L.rtmi_last_error()
        both(b"analytic spheres")
        assert L.rtmi_scene_set_spheres(hnd, None, 0) == 0, L.rtmi_last_error()
        rec, _, _ = so.triangles()
        n = rec.shape[0]
        corners = np.ascontiguousarray(rec[:, 20:29])
        nrm = np.ascontiguousarray(np.repeat(rec[:, None, 3:6], 3, axis=1).astype(F32))
        assert L.rtmi_scene_set_normals(hnd, p(corners), p(nrm), n) == 0, L.rtmi_last_error()
        both(b"vertex normals")
        assert L.rtmi_scene_set_normals(hnd, p(corners), None, n) == 0, L.rtmi_last_error()
        got, _ = RAW._render(L, ffi, hnd, vp12, 8, 8, 4, 2, 3)
        want, _ = so.render(8, 8, vp12, 4, 2, seed=3)
        assert_bits_equal(got, want, "the plain frame after the refusals")
        # ... and the lit frame through the raw ABI, against the restatement
        st = ffi.Stats()
        assert L.rtmi_render_lit(hnd, C.byref(vp), 3, 0, 8, 0, 2, C.byref(lit), p(acc), p(out), C.byref(st)) == 0, L.rtmi_last_error()
        ref = LT.render(orc, so, vp12, 8, 8, 2, 3, 4, AB)
        assert_bits_equal(out, ref.image, "raw ABI: image")
        assert_bits_equal(acc, ref.accum, "raw ABI: accum")
        assert st.rays == ref.rays + ref.nlive
    finally:
        L.rtmi_scene_destroy(hnd)
