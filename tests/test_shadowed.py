"""-m gpu: the shadowed path-trace (rtmi_render_shadowed / rtmi_render_shadowed_device, HipRayCaster.walk_rays_shadowed*) against
its definition, every float bit for bit: tests/shadowed_ref.py restates the whole bounce loop of include/rtmi.h in float32 NumPy
on the oracle's rays, closest hits, triangle records and RNG (tests/test_shadowed_cpu.py pins it to the oracle's own render), so
no expected value comes from the code under test.  The two modes that are not bit-exact by design, RTMI_OPT_BVH and
RTMI_OPT_FAST, are held against the restatement fed by the product's own rtmi_trace / rtmi_occluded.  One test needs no
restatement at all: at a depth of 1 the image follows from the features and the direct-light calls.  The references are
computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

from conftest import TEAPOT, OracleApi, ProductApi, assert_bits_equal, build_pair, recipe_canonical, recipe_circles, recipe_circles_analytic
import occluded_ref as OR
import shadowed_ref as SR
from test_shadowed_cpu import CANONICAL_LIVE, CANONICAL_PASSES, CANONICAL_RAYS

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = ("box_tests", "tri_tests", "full_tests", "nodes", "leaves")
FULL = None  # tile: the whole frame through the host variant
LIGHT = OR.LIGHT  # (-3, 6, 1)
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _ref(so, w, h, maxdepth, spp, seed, light=LIGHT, len2=0.5, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), w, h, maxdepth, spp, seed, None if light is None else tuple(light), len2, tuple(sorted(kw.items())))
    if key not in _REFS:
        orc = _orc()
        _REFS[key] = SR.shadowed_ref(orc, so, w, h, orc.canonical_viewport(w, h), maxdepth, spp, seed, light, len2, **kw)
    return _REFS[key]


def _render(c, sp, w, h, maxdepth, spp, light=LIGHT, len2=0.5, bias=None, flags=0, sample0=0, nsamples=None, tile=FULL, accum=None):
    """(image (rows, w, 4), accum, stats) of one call: the host variant for the whole frame, the device variant on torch tensors
    with guard floats for a tile"""
    vp = _R().canonical_viewport(w, h, maxdepth, spp)
    lk = dict(orig=light, len2=len2, unbounded=bool(flags & SR.LR.UNBOUNDED), bias=bias, sample0=sample0, nsamples=nsamples)
    if tile is FULL:
        img, ctx = c.walk_rays_shadowed(vp, sp, accum=accum, **lk)
        return img, ctx.accum, ctx.stats
    import torch
    n = tile[1] * w * 4
    bufs = [torch.full((n + 128,), 7.5, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    if accum is not None:
        bufs[0][64:64 + n] = torch.from_numpy(np.ascontiguousarray(accum, F32).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_shadowed_device(vp, sp, bufs[0][64:64 + n], bufs[1][64:64 + n], tile=tile, **lk)
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        g = b.cpu().numpy()
        assert (g[:64] == 7.5).all() and (g[64 + n:] == 7.5).all(), "guard floats"
        out.append(g[64:64 + n].reshape(tile[1], w, 4))
    return out[1], out[0], ctx.stats


def _check(c, so, sp, w, h, maxdepth, spp, seed, what, ref=None, **kw):
    """One call against the restatement: the image, the sums, stats.rays and the launch bookkeeping.  -> (reference, stats)"""
    if ref is None:
        ref_kw = {k: v for k, v in kw.items() if k != "bias" or v is not None}
        ref = _ref(so, w, h, maxdepth, spp, seed, **ref_kw)
    img, acc, st = _render(c, sp, w, h, maxdepth, spp, **kw)
    assert img.dtype == np.float32
    assert_bits_equal(img, ref.image, f"{what}: image")
    assert_bits_equal(acc, ref.accum, f"{what}: accum")
    assert st["rays"] == ref.rays + ref.nlive, f"{what}: rays {st['rays']} vs {ref.rays} + {ref.nlive}"
    assert st["pipeline"] == 1 and st["slow_paths"] == 0
    if maxdepth:
        assert st["trace_launches"] >= 2 * maxdepth and st["trace_launches"] % (2 * maxdepth) == 0
        assert st["kernel_ms"] > 0 and st["primary_ms"] > 0 and st["bounce_ms"] >= 0
        assert abs(st["trace_ms"] - (st["primary_ms"] + st["bounce_ms"])) <= 1e-3 * st["trace_ms"]
    return ref, st


# ---------------------------------------------------------------- 1: the canonical case
def test_canonical_case_host_variant(canonical_pair):
    so, sp = canonical_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "canonical")
    assert tuple((p["tested"], p["culled"], p["live"], p["occluded"]) for p in ref.passes) == CANONICAL_PASSES
    assert st["rays"] == CANONICAL_RAYS + CANONICAL_LIVE


def test_canonical_case_device_variant_on_a_striped_tile(canonical_pair):
    so, sp = canonical_pair
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "tile {1, 12, 3, 8}", tile=(1, 12, 3, 8))
    assert ref.nlive > 100 and ref.passes[0]["shadowed"] > 0 and ref.passes[2]["tested"] > 0


# ---------------------------------------------------------------- 2: independent of the restatement
def test_depth_1_follows_from_the_features_and_the_direct_light_calls(canonical_pair):
    """maxdepth = 1, S = 1: a pixel's colour is mix_color(lit ? colour : black, black, alpha) of its first hit (colour or
    black for a Solid), the sky for a miss and black for an edge face, with `colour` and the hit from rtmi_render_features and
    `lit` the shadow plane (0 or 1) of rtmi_render_light with K = 1 -- whose candidate k = 0 this call's shadow ray is."""
    so, sp = canonical_pair
    R = _R()
    w = h = 48
    c = R.HipRayCaster(seed=1)
    vp = R.canonical_viewport(w, h, 1, 1)
    img, ctx = c.walk_rays_shadowed(vp, sp, orig=LIGHT, len2=0.5)
    alb, _, ids, _ = c.walk_rays_features(vp, sp)
    shadow, _, _ = c.walk_rays_light(vp, sp, orig=LIGHT, len2=0.5, rays=1, irradiance=False)
    assert set(np.unique(shadow)) == {0.0, 1.0}
    _, kinds, surf = so.triangles()
    tri, face = ids & np.uint32(0x3FFFFFFF), ids >> np.uint32(30)
    miss, edge = tri == 0, (tri != 0) & ((face & 2) != 0)
    lit = shadow == 1.0
    col = np.zeros((h, w, 4), F32)
    col[..., :3] = alb[..., :3]
    col[~lit] = 0.0
    alpha = surf[tri, 3].astype(F32)[..., None]
    mixed = ((col * (F32(1.0) - alpha)).astype(F32) + (np.zeros_like(col) * alpha).astype(F32)).astype(F32)
    want = np.where((kinds[tri] == SR.SOLID)[..., None], col, mixed)
    want[edge] = 0.0
    want[miss] = np.array([*SR.FR.SKY, 0.0], F32)
    surface = ~miss & ~edge
    assert (surface & lit).sum() > 100 and (surface & ~lit).sum() > 100 and edge.sum() > 0
    assert_bits_equal(img, want.astype(F32), "depth 1 from features and light")
    assert w * h < ctx.stats["rays"] <= w * h + int(surface.sum())


# ---------------------------------------------------------------- 3, 4: the anchors on the wall
@pytest.fixture(scope="module")
def wall_pair():
    return build_pair(SR.recipe_wall())


def _plain(c, sp, w, h, maxdepth, spp, tile=(0, 32, 32, 0)):
    """rtmi_render_samples_device of the whole frame: (image, stats)"""
    import torch
    vp = _R().canonical_viewport(w, h, maxdepth, spp)
    acc, out = (torch.zeros(tile[1] * w * 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
    ctx = c.walk_samples_device(vp, sp, tile, 0, spp, acc.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(tile[1], w, 4), ctx.stats


def test_unshadowed_anchor(wall_pair):
    """The light behind the camera, a depth of 1 (tests/test_shadowed_cpu.py says why): no hit is shadowed, the image is the
    plain progressive pass's"""
    so, sp = wall_pair
    c = _R().HipRayCaster(seed=1)
    ref, st = _check(c, so, sp, 32, 32, 1, 2, 1, "wall, light behind the camera", light=SR.BEHIND_CAMERA, len2=0.0)
    assert ref.passes[0]["shadowed"] == 0 and ref.nlive == 2048
    img, _, _ = _render(c, sp, 32, 32, 1, 2, light=SR.BEHIND_CAMERA, len2=0.0, tile=(0, 32, 32, 0))
    plain, pst = _plain(c, sp, 32, 32, 1, 2)
    assert_bits_equal(img, plain, "unshadowed wall against rtmi_render_samples_device")
    assert st["rays"] == pst["rays"] + 2048


def test_all_culled_anchor(wall_pair):
    """The light behind the wall: every hit is culled, no ray is walked, and the image is the plain render of the same wall
    painted black"""
    so, sp = wall_pair
    c = _R().HipRayCaster(seed=1)
    ref, st = _check(c, so, sp, 32, 32, 1, 2, 1, "wall, light behind it", light=SR.BEHIND_WALL, len2=0.0)
    assert ref.passes[0]["culled"] == 2048 and ref.nlive == 0
    img, _, _ = _render(c, sp, 32, 32, 1, 2, light=SR.BEHIND_WALL, len2=0.0, tile=(0, 32, 32, 0))
    black, pst = _plain(c, SR.recipe_wall(color=(0, 0, 0))(ProductApi(_R())), 32, 32, 1, 2)
    assert_bits_equal(img, black, "culled wall against the black wall")
    assert st["rays"] == pst["rays"] == 2048


# ---------------------------------------------------------------- 5: progressive passes
def test_progressive_passes_end_in_the_bits_of_one_call(canonical_pair):
    so, sp = canonical_pair
    c = _R().HipRayCaster(seed=1)
    for tile in (FULL, (1, 12, 3, 8)):
        one, acc1, _ = _render(c, sp, 32, 32, 5, 4, tile=tile)
        acc, img = None, None
        for s0, n in ((0, 1), (1, 2), (3, 1)):
            img, acc, _ = _render(c, sp, 32, 32, 5, 4, sample0=s0, nsamples=n, tile=tile, accum=acc)
        assert_bits_equal(img, one, f"passes [0,1) [1,3) [3,4), tile {tile}: out")
        assert_bits_equal(acc, acc1, f"passes [0,1) [1,3) [3,4), tile {tile}: accum")
    ref = _ref(so, 32, 32, 5, 4, 1)
    assert_bits_equal(one, ref.image[SR.FR.tile_rows((1, 12, 3, 8))], "S = 4 against the restatement")


# ---------------------------------------------------------------- 6: the scene kinds
def test_linear_list_scene():
    so, sp = build_pair(recipe_canonical(accel="trivial", obj=TEAPOT))
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 4, 2, 1, "linear list")
    assert ref.nlive > 50 and sum(p["occluded"] for p in ref.passes) > 0 and ref.passes[1]["tested"] > 0


def test_option_generic_keeps_the_path_queues_hit_records(canonical_pair):
    """RTMI_OPT_GENERIC: the shadow rays' walk is a closest-hit launch, which must not write over the hit records the shading
    of the same pass still reads"""
    so, sp = canonical_pair
    R = _R()
    _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 5, 2, 1, "RTMI_OPT_GENERIC")
    _check(R.HipRayCaster(seed=1, options=R.OPT_GENERIC), so, sp, 32, 32, 5, 2, 1, "RTMI_OPT_GENERIC, tile", tile=(1, 12, 3, 8))


def test_generic_tree_through_the_raw_abi():
    """A tree that is no octree (nudged, grown boxes): the generic kernel traces the paths and the shadow rays"""
    from test_gpu_abi_raw import Vp, _abi_arrays, _boxes, _create, _lib
    orc = _orc()
    L, ffi = _lib()
    so = recipe_circles(maxdepth=4, minobjs=6)(OracleApi(orc))
    tris, geo, topo, refs = _abi_arrays(so)
    rng = np.random.default_rng(5)
    geo = geo.copy()
    geo[:, 0:3] += rng.uniform(-0.01, 0.01, (len(geo), 3)).astype(np.float32)
    geo[:, 3] *= np.float32(1.07)
    so.set_tree(geo, topo, refs)
    rc, hnd = _create(L, tris, _boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    try:
        w = h = 24
        vp12 = orc.canonical_viewport(w, h)
        light = (-2.0, 6.0, 3.0)
        ref = SR.shadowed_ref(orc, so, w, h, vp12, 4, 2, 3, light, 0.5)
        assert ref.nlive > 100 and sum(p["occluded"] for p in ref.passes) > 0 and ref.passes[1]["tested"] > 0
        vp = Vp(w, h, (C.c_float * 3)(*vp12[0:3]), (C.c_float * 3)(*vp12[3:6]), (C.c_float * 3)(*vp12[6:9]), (C.c_float * 3)(*vp12[9:12]), 4, 2)
        li = ffi.Light((C.c_float * 3)(*light), 0.5, 1, 0, 0.005)
        acc, out = np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32)
        st = ffi.Stats()
        rc = L.rtmi_render_shadowed(hnd, C.byref(vp), 3, 0, h, 0, 2, C.byref(li), acc.ctypes.data_as(C.c_void_p),
                                    out.ctypes.data_as(C.c_void_p), C.byref(st))
        assert rc == 0, L.rtmi_last_error()
        assert_bits_equal(out, ref.image, "generic tree: image")
        assert st.rays == ref.rays + ref.nlive and st.pipeline == 1
    finally:
        L.rtmi_scene_destroy(hnd)


@pytest.mark.parametrize("opt", ["OPT_BVH", "OPT_FAST"])
def test_options_bvh_and_fast_against_their_own_trace_and_occluded(canonical_pair, opt):
    so, sp = canonical_pair
    R, orc = _R(), _orc()
    c = R.HipRayCaster(seed=1, options=getattr(R, opt))
    ref = SR.shadowed_ref(orc, so, 32, 32, orc.canonical_viewport(32, 32), 5, 2, 1, LIGHT, 0.5,
                          trace=lambda o, d: c.trace(sp, o, d)[:3], occluded=lambda o, d, tm: c.occluded(sp, o, d, tm)[0])
    assert ref.nlive > 300 and sum(p["occluded"] for p in ref.passes) > 0 and sum(p["culled"] for p in ref.passes) > 0
    _check(c, so, sp, 32, 32, 5, 2, 1, opt, ref=ref)


def test_analytic_spheres_are_unsupported():
    R = _R()
    sp = recipe_circles_analytic()(ProductApi(R))
    c = R.HipRayCaster()
    with pytest.raises(RuntimeError, match="analytic spheres"):
        c.walk_rays_shadowed(R.canonical_viewport(16, 16, 5, 1), sp, orig=LIGHT)
    import torch
    acc = torch.zeros(16 * 16 * 4, dtype=torch.float32, device="cuda:0")
    with pytest.raises(RuntimeError, match="analytic spheres"):
        c.walk_rays_shadowed_device(R.canonical_viewport(16, 16, 5, 1), sp, acc, orig=LIGHT)
    assert (acc == 0).all()


# ---------------------------------------------------------------- 7: streams and batches
@pytest.mark.parametrize("tuning", [dict(streams=3, batch_paths=600, subtile_min_paths=1), dict(streams=1, batch_paths=500),
                                    dict(streams=2, batch_paths=4096, subtile_min_paths=1)],
                         ids=lambda t: ",".join(f"{k}={v}" for k, v in t.items()))
def test_tuning_changes_no_bit(canonical_pair, tuning):
    so, sp = canonical_pair
    R = _R()
    try:
        for options in (0, R.OPT_GENERIC):
            _, st = _check(R.HipRayCaster(seed=1, options=options, tuning=tuning), so, sp, 32, 32, 5, 2, 1, f"tuning {tuning}, options {options}")
            assert st["streams"] == tuning["streams"]
            if tuning["batch_paths"] < 1000:  # several batches per sub-tile, each of 5 passes with two launches
                assert st["trace_launches"] >= 10 * 3 * tuning["streams"]
    finally:
        R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


# ---------------------------------------------------------------- 8: parameters and depths
def test_unbounded_light_and_point_light(canonical_pair):
    so, sp = canonical_pair
    _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "unbounded", flags=SR.LR.UNBOUNDED)
    # a light inside the scene, between the teapot and the upper mirror: what lies beyond it shadows only when unbounded
    inside = (2.5, 2.0, 6.0)
    u, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "unbounded, inside", light=inside, flags=SR.LR.UNBOUNDED)
    i, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "bounded, inside", light=inside)
    assert u.passes[0]["occluded"] > 100 > 10 > i.passes[0]["occluded"] and u.nlive == i.nlive
    b = _ref(so, 32, 32, 5, 2, 1)
    p, _ = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 5, 2, 1, "len2 = 0", len2=0.0)
    assert p.nlive > 0 and not np.array_equal(p.image, b.image)
    _check(_R().HipRayCaster(seed=7), so, sp, 32, 32, 5, 2, 7, "seed 7, bias 0.05", bias=0.05)


def test_depth_32_on_the_wall(wall_pair):
    so, sp = wall_pair
    ref, st = _check(_R().HipRayCaster(seed=1), so, sp, 32, 32, 32, 2, 1, "wall, depth 32", light=SR.BEHIND_CAMERA, len2=0.0)
    assert len(ref.passes) == 32 and ref.passes[1]["culled"] > 500 and ref.passes[2]["live"] > 200
    assert st["trace_launches"] % 64 == 0


def test_depth_32_in_the_corridor_sets_bit_31():
    so, sp = build_pair(SR.recipe_corridor())
    ref, _ = _check(_R().HipRayCaster(seed=1), so, sp, 16, 16, 32, 1, 1, "corridor, depth 32", light=SR.CORRIDOR_LIGHT, len2=SR.CORRIDOR_LEN2)
    assert ref.passes[31]["tested"] == 256 and 0 < ref.passes[31]["shadowed"] < 256


def test_depth_0_writes_zeros(canonical_pair):
    so, sp = canonical_pair
    c = _R().HipRayCaster(seed=1)
    for tile in (FULL, (1, 12, 3, 8)):
        img, acc, st = _render(c, sp, 32, 32, 0, 2, tile=tile, accum=np.full((32 if tile is FULL else 12, 32, 4), 3.0, F32))
        assert (img == 0).all() and (acc == 0).all() and st["rays"] == 0


def test_device_variant_on_a_torch_stream_without_a_preview(canonical_pair):
    """out = NULL, a stream of the caller's, work queued behind the call on it, and a larger call in between (the buffers grow)"""
    import torch
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1)
    small, large = _ref(so, 32, 32, 5, 2, 1), _ref(so, 48, 48, 3, 1, 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a1 = torch.full((4096 + 128,), 7.5, dtype=torch.float32, device="cuda:0")
        ctx = c.walk_rays_shadowed_device(R.canonical_viewport(32, 32, 5, 2), sp, a1[64:64 + 4096], None, orig=LIGHT, len2=0.5, stream=st)
        total = a1[64:64 + 4096].sum(dtype=torch.float64)  # queued behind the call on the same stream
        a2, o2 = (torch.zeros(48 * 48 * 4, dtype=torch.float32, device="cuda:0") for _ in range(2))
        c.walk_rays_shadowed_device(R.canonical_viewport(48, 48, 3, 1), sp, a2, o2, orig=LIGHT, len2=0.5, stream=st)
        a3, o3 = (torch.zeros(4096, dtype=torch.float32, device="cuda:0") for _ in range(2))
        c.walk_rays_shadowed_device(R.canonical_viewport(32, 32, 5, 2), sp, a3, o3, orig=LIGHT, len2=0.5, stream=st.cuda_stream)
    st.synchronize()
    g = a1.cpu().numpy()
    assert (g[:64] == 7.5).all() and (g[64 + 4096:] == 7.5).all(), "guard floats"
    assert_bits_equal(g[64:64 + 4096].reshape(32, 32, 4), small.accum, "no preview: accum")
    assert abs(float(total) - float(small.accum.astype(np.float64).sum())) <= 1e-9 * float(total)
    assert_bits_equal(o2.cpu().numpy().reshape(48, 48, 4), large.image, "48 x 48, depth 3, S = 1")
    assert_bits_equal(o3.cpu().numpy().reshape(32, 32, 4), small.image, "32 x 32 again")
    assert ctx.stats["rays"] == small.rays + small.nlive and ctx.total_rays == ctx.stats["rays"]


# ---------------------------------------------------------------- 9: counters
def test_counters_include_the_walks(canonical_pair):
    so, sp = canonical_pair
    R = _R()
    try:
        ref, st = _check(R.HipRayCaster(seed=1, options=R.OPT_COUNTERS), so, sp, 32, 32, 5, 2, 1, "counters")
        _, pst = _plain(R.HipRayCaster(seed=1, options=R.OPT_COUNTERS, tuning=dict(pipeline=1)), sp, 32, 32, 5, 2)
        assert pst["pipeline"] == 1 and pst["rays"] == ref.rays
        print({k: (st[k], pst[k]) for k in COUNTERS})
        for k in COUNTERS:
            assert st[k] >= pst[k] > 0, k
        assert st["rays"] == ref.rays + ref.nlive == CANONICAL_RAYS + CANONICAL_LIVE
        assert st["box_tests"] > pst["box_tests"] and st["tri_tests"] > pst["tri_tests"]  # 587 rays were walked
    finally:
        R.HipRayCaster().upload(sp)


# ---------------------------------------------------------------- 10: refused arguments
def test_bad_arguments_are_refused_before_the_scene_is_used():
    SR.check_refusals()


def test_a_refused_call_leaves_the_handle_usable(canonical_pair):
    so, sp = canonical_pair
    R = _R()
    c = R.HipRayCaster(seed=1)
    with pytest.raises(ValueError):
        c.walk_rays_shadowed(R.canonical_viewport(32, 32, 5, 2), sp, orig=LIGHT, len2=-1.0)
    L = __import__("rust_raytrace_amd._ffi", fromlist=["lib"]).lib()
    assert L.rtmi_render_shadowed(None, None, 1, 0, 0, 0, 1, None, None, None, None) == 1
    _check(c, so, sp, 32, 32, 5, 2, 1, "after the refusals")
    # ... and a plain render on the same handle afterwards equals a fresh handle's
    vp = R.canonical_viewport(48, 32, 5, 2)
    after, fresh = np.zeros((32, 48, 4), F32), np.zeros((32, 48, 4), F32)
    c.walk_rays(vp, sp, after, 1, False)
    R.HipRayCaster(seed=1).walk_rays(vp, recipe_canonical()(ProductApi(R)), fresh, 1, False)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32))
