"""-m gpu: environment sampling at matte hits (rtmi_render_envlight / rtmi_render_envlight_device, rtmi_scene_get_env_sampler;
HipRayCaster.walk_rays_envlight*, env_sampler) against its definition, every float and every integer bit for bit:
tests/envlight_ref.py restates include/rtmi.h in NumPy on the oracle's rays, closest hits, triangle records and RNG
(tests/test_envlight_cpu.py pins it and checks that the definition is unbiased), so no expected value comes from the code under
test.  Two tests need no restatement: under an all-zero environment the image is the plain progressive pass's, and at a depth of 1
the call is the plain call.  The references are computed once per case and shared."""
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import env_ref as ER
from envlight_cases import SUN, hdr as _hdr, rotation as _rotation  # shared with tests/shadow_matrix_cases.py
import envlight_ref as EL
import features_ref as FR

pytestmark = pytest.mark.gpu
F32 = np.float32
W = H = 32
SPP, SEED, MAXDEPTH = 4, 5, 4
FULL = None  # tile: the whole frame through the host variant
TILE = (1, 12, 3, 8)
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
    """The canonical Matte / Reflective scene in its octree under the generated sky, n = 16, the sun on one side"""
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_sky(16, **SUN)
    return so, sp, SimpleNamespace(table=ER.sky_table(16, SUN), frame=None)


@pytest.fixture(scope="module")
def teapot_list():
    """The same scene as a linear list, under a random HDR table of 5 x 5 texels in a rotated frame"""
    so, sp = CT.build_pair(CT.recipe_canonical(accel="trivial", obj=CT.TEAPOT))
    env = SimpleNamespace(table=_hdr(5), frame=_rotation())
    sp.set_environment(env.table, env.frame)
    return so, sp, env


def _ref(so, env, w=W, h=H, spp=SPP, maxdepth=MAXDEPTH, seed=SEED, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), id(env), w, h, spp, maxdepth, seed, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = EL.render(_orc(), so, _orc().canonical_viewport(w, h), w, h, spp, seed, maxdepth, env, **kw)
    return _REFS[key]


def _render(c, sp, w=W, h=H, spp=SPP, maxdepth=MAXDEPTH, bias=None, sample0=0, nsamples=None, tile=FULL, accum=None):
    """(image (rows, w, 4), accum, stats) of one call: the host variant for the whole frame, the device variant on torch tensors
    with guard floats for a tile"""
    vp = _R().canonical_viewport(w, h, maxdepth, spp)
    if tile is FULL:
        img, ctx = c.walk_rays_envlight(vp, sp, accum=accum, bias=bias, sample0=sample0, nsamples=nsamples)
        return img, ctx.accum, ctx.stats
    import torch
    n = tile[1] * w * 4
    bufs = [torch.full((n + 128,), 7.5, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    if accum is not None:
        bufs[0][64:64 + n] = torch.from_numpy(np.ascontiguousarray(accum, F32).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_envlight_device(vp, sp, bufs[0][64:64 + n], bufs[1][64:64 + n], tile=tile, bias=bias, sample0=sample0, nsamples=nsamples)
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


def _check(c, ref, sp, what, **kw):
    """One call against the restatement: the image, the sums, stats.rays and the launch bookkeeping"""
    img, acc, st = _render(c, sp, **kw)
    maxdepth = kw.get("maxdepth", MAXDEPTH)
    assert_bits_equal(img, ref.image, f"{what}: image")
    assert_bits_equal(acc, ref.accum, f"{what}: accum")
    assert st["rays"] == ref.rays + ref.nlive, f"{what}: rays {st['rays']} vs {ref.rays} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0
    assert st["trace_launches"] >= 2 * maxdepth and st["trace_launches"] % (2 * maxdepth) == 0
    assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] >= 0
    return st


# ---------------------------------------------------------------- (e) the sampler table
@pytest.mark.parametrize("name", list(EL.table_cases()) + ["hdr129"])
def test_sampler_table_is_the_definitions(name):
    table = _hdr(129) if name == "hdr129" else EL.table_cases()[name]
    so, sp = CT.build_pair(CT.recipe_axis_box())
    sp.set_environment(table)
    q, total = _R().HipRayCaster(seed=SEED).env_sampler(sp)
    wq, wtotal = EL.sampler_table(table)
    assert q.dtype == np.uint32 and np.array_equal(q, wq), f"{name}: {(q != wq).sum()} of {q.size} weights differ"
    assert total == wtotal == int(wq.astype(np.uint64).sum())
    assert q.min() >= 1 and q.max() <= 1048577


def test_sampler_table_of_the_generated_sky_and_set_replace_clear():
    R = _R()
    so, sp = CT.build_pair(CT.recipe_axis_box())
    c = R.HipRayCaster(seed=SEED)
    assert c.env_sampler(sp) is None
    sp.set_sky(256)
    q, total = c.env_sampler(sp)
    wq, wtotal = EL.sampler_table(ER.sky_table(256))
    assert np.array_equal(q, wq) and total == wtotal
    assert q.max() >= 1048576 and (q > 500000).sum() < 0.01 * q.size  # the sun is a few texels (wmax * fl(2^20 / wmax) may round down)
    sp.set_environment(_hdr(5))  # replaced: the table is the new map's
    q, total = c.env_sampler(sp)
    wq, wtotal = EL.sampler_table(_hdr(5))
    assert q.shape == (5, 5) and np.array_equal(q, wq) and total == wtotal
    sp.clear_environment()
    assert c.env_sampler(sp) is None


# ---------------------------------------------------------------- (f) the pass
def test_octree_scene_whole_frame(teapot):
    so, sp, env = teapot
    ref = _ref(so, env)
    pt = ref.pt
    assert sum(pt.nlive) > 300 and sum(pt.nlive) - sum(pt.occluded) > 30 and sum(pt.occluded) > 100 and sum(pt.culled) > 100 and pt.nlive[1] > 0 and pt.nlive[2] > 0
    assert pt.nlive[MAXDEPTH - 1] == 0 and pt.candidates[MAXDEPTH - 1] == 0  # no sample at the exhausted level
    plain = EL.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, SPP, SEED, MAXDEPTH, env, nee=False)
    assert plain.rays == ref.rays and not np.array_equal(plain.image, ref.image)
    _check(_R().HipRayCaster(seed=SEED), ref, sp, "octree, whole frame")


def test_octree_scene_striped_tile(teapot):
    so, sp, env = teapot
    ref = _ref(so, env, tile=TILE)
    assert ref.nlive > 100
    _check(_R().HipRayCaster(seed=SEED), ref, sp, f"octree, tile {TILE}", tile=TILE)


@pytest.mark.parametrize("tile", [FULL, TILE], ids=["frame", "tile"])
def test_progressive_continuation_equals_one_call(teapot, tile):
    so, sp, env = teapot
    c = _R().HipRayCaster(seed=SEED)
    ref = _ref(so, env) if tile is FULL else _ref(so, env, tile=TILE)
    acc, img = None, None
    for s0, n in ((0, 1), (1, 2), (3, 1)):
        img, acc, _ = _render(c, sp, sample0=s0, nsamples=n, tile=tile, accum=acc)
    assert_bits_equal(img, ref.image, "passes [0,1) [1,3) [3,4): out")
    assert_bits_equal(acc, ref.accum, "passes [0,1) [1,3) [3,4): accum")
    # one pass with sample0 > 0 on sums of its own, against the restatement
    acc0 = np.full(ref.accum.shape, 0.25, F32)
    part = EL.render(_orc(), so, _orc().canonical_viewport(W, H), W, H, SPP, SEED, MAXDEPTH, env, sample0=1, nsamples=2,
                     tile=None if tile is FULL else TILE, accum0=acc0)
    img, acc, st = _render(c, sp, sample0=1, nsamples=2, tile=tile, accum=acc0.copy())
    assert_bits_equal(img, part.image, "pass [1,3): out")
    assert_bits_equal(acc, part.accum, "pass [1,3): accum")
    assert st["rays"] == part.rays + part.nlive


def test_linear_list_scene_rotated_frame(teapot_list):
    so, sp, env = teapot_list
    assert EL.frame_is_rotation(env.frame)
    ref = _ref(so, env, w=16, h=16)
    assert ref.nlive > 100 and sum(ref.pt.occluded) > 10
    _check(_R().HipRayCaster(seed=SEED), ref, sp, "linear list, rotated frame", w=16, h=16)
    ref7 = _ref(so, env, w=16, h=16, seed=7, bias=0.05)
    _check(_R().HipRayCaster(seed=7), ref7, sp, "linear list, seed 7, bias 0.05", w=16, h=16, bias=0.05)


def test_several_streams_and_batches_change_no_bit(teapot):
    so, sp, env = teapot
    R = _R()
    try:
        st = _check(R.HipRayCaster(seed=SEED, tuning=dict(streams=3, batch_paths=600, subtile_min_paths=1)), _ref(so, env), sp, "3 streams, batches of 600")
        assert st["streams"] == 3 and st["trace_launches"] >= 2 * MAXDEPTH * 3 * 2
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


# ---------------------------------------------------------------- (g), (h) independent of the restatement
def test_all_zero_environment_is_the_plain_progressive_pass():
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_environment(np.zeros((4, 4, 3), F32))
    c = _R().HipRayCaster(seed=SEED)
    img, _, st = _render(c, sp, tile=(0, H, H, 0))
    plain, pst = _plain(c, sp)
    assert (img == plain).all() and np.isfinite(img).all() and (plain[..., :3] > 0).any()
    assert st["rays"] == pst["rays"]  # nothing to sample: no candidate is live


def test_depth_1_is_the_plain_call_with_its_hits_and_rays(teapot):
    """Pass 0 on the same arguments.  The envlight call returns no ids of its own, so what ties its pass 0 to the plain call's is
    the ray count and the image: with nothing behind pass 0 both are the plain call's (an exhausted level gets no sample), and at
    depth 4 the rays less the live shadow rays are the plain call's too."""
    so, sp, env = teapot
    c = _R().HipRayCaster(seed=SEED)
    img, _, st = _render(c, sp, maxdepth=1, tile=(0, H, H, 0))
    plain, pst = _plain(c, sp, maxdepth=1)
    assert_bits_equal(img, plain, "depth 1 against rtmi_render_samples_device")
    assert st["rays"] == pst["rays"] == W * H * SPP
    ref = _ref(so, env)
    _, _, st4 = _render(c, sp, tile=(0, H, H, 0))
    _, pst4 = _plain(c, sp)
    assert st4["rays"] - ref.nlive == pst4["rays"] == ref.rays


def test_depth_0_writes_zeros(teapot):
    so, sp, env = teapot
    c = _R().HipRayCaster(seed=SEED)
    for tile in (FULL, TILE):
        img, acc, st = _render(c, sp, maxdepth=0, tile=tile, accum=np.full((H if tile is FULL else TILE[1], W, 4), 3.0, F32))
        assert (img == 0).all() and (acc == 0).all() and st["rays"] == 0


# ---------------------------------------------------------------- (i) refusals
def test_invalid_arguments_are_refused_before_the_scene_is_used():
    EL.check_invalid_arguments()


def _refused(c, sp, word):
    import torch
    vp = _R().canonical_viewport(16, 16, MAXDEPTH, 1)
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_envlight(vp, sp)
    acc = torch.zeros(16 * 16 * 4, dtype=torch.float32, device="cuda:0")
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_envlight_device(vp, sp, acc)
    assert (acc == 0).all()


def test_a_refused_scene_returns_unsupported_with_cleared_stats_through_the_raw_abi():
    """What the Python layer's exception hides: rc == RTMI_ERR_UNSUPPORTED and stats cleared, for both variants, on a real handle
    without an environment and then under a frame that is no rotation"""
    import ctypes as C
    from test_gpu_abi_raw import Vp, _abi_arrays, _boxes, _create, _lib
    orc = _orc()
    L, ffi = _lib()
    so = CT.recipe_circles(maxdepth=4, minobjs=6)(CT.OracleApi(orc))
    tris, geo, topo, refs = _abi_arrays(so)
    rc, hnd = _create(L, tris, _boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    try:
        vp12 = orc.canonical_viewport(8, 8)
        vp = Vp(8, 8, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]), (C.c_float * 3)(*vp12[9:12]), 4, 2)
        acc, out = np.full((8, 8, 4), 3.0, F32), np.full((8, 8, 4), 5.0, F32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def both(word):
            for dev in (False, True):
                st = ffi.Stats()
                st.rays, st.trace_launches = 123, 7
                if dev:  # (refused before the pointers are used: host memory will do)
                    tile = ffi.Tile(0, 8, 8, 0)
                    rc = L.rtmi_render_envlight_device(hnd, C.byref(vp), 3, C.byref(tile), 0, 2, None, p(acc), p(out), None, C.byref(st))
                else:
                    rc = L.rtmi_render_envlight(hnd, C.byref(vp), 3, 0, 8, 0, 2, None, p(acc), p(out), C.byref(st))
                assert rc == 3 and word in L.rtmi_last_error(), (rc, L.rtmi_last_error())  # RTMI_ERR_UNSUPPORTED
                assert st.rays == 0 and st.trace_launches == 0 and st.kernel_ms == 0
            assert (acc == 3.0).all() and (out == 5.0).all()
        both(b"no environment")
        table = np.ones((4, 4, 3), F32)
        e = ffi.Environment()
        L.rtmi_environment_defaults(C.byref(e))
        e.frame[1] = 0.01
        assert L.rtmi_scene_set_environment(hnd, p(table), 4, C.byref(e)) == 0, L.rtmi_last_error()
        both(b"not a rotation")
        n, total = C.c_uint32(0), C.c_uint64(0)
        assert L.rtmi_scene_get_env_sampler(hnd, None, C.byref(total), C.byref(n)) == 0 and n.value == 4 and total.value > 16
    finally:
        L.rtmi_scene_destroy(hnd)


def test_scenes_the_call_does_not_take_are_refused_and_the_handle_stays_usable():
    import glass_cases as GC
    import tex_cases as TC
    R = _R()
    c = R.HipRayCaster(seed=SEED)
    so, sp = CT.build_pair(CT.recipe_canonical())
    _refused(c, sp, "no environment")
    sp.set_sky(8, **SUN)
    env = SimpleNamespace(table=ER.sky_table(8, SUN), frame=None)
    sp.smooth_normals(1, NTEAPOT)
    _refused(c, sp, "vertex normals")
    sp.clear_vertex_normals()
    sp.set_textures([TC.images()[3]], None, None)
    sp.project_uvs(1, NTEAPOT, (-1.7, -0.4, 3.1), 0.9, 1)
    _refused(c, sp, "textures")
    sp.set_normal_maps(np.full(NTEAPOT, 1, np.uint32))
    _refused(c, sp, "normal maps")
    sp.clear_textures()
    skew = np.eye(3, dtype=F32)
    skew[0, 1] = 0.01
    sp.set_environment(env.table, skew)
    _refused(c, sp, "not a rotation")
    sp.set_environment(env.table, np.eye(3, dtype=F32) * F32(1.001))
    _refused(c, sp, "not a rotation")
    sp.set_sky(8, **SUN)  # ... and the same handle renders once the scene is one the call takes
    _check(c, _ref(so, env, w=16, h=16, spp=2), sp, "after the refusals", w=16, h=16, spp=2)
    glass = GC.build_pair(GC.recipe_slab())[1]
    glass.set_sky(8, **SUN)
    _refused(R.HipRayCaster(seed=SEED), glass, "dielectric")
    spheres = CT.recipe_circles_analytic()(CT.ProductApi(R))
    spheres.set_sky(8, **SUN)
    _refused(R.HipRayCaster(seed=SEED), spheres, "analytic spheres")
