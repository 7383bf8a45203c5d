"""-m gpu: the built-in camera models (rtmi_render_camera / rtmi_render_camera_device, HipRayCaster.walk_*_camera*) against their
definition, every float bit for bit.  The pinhole is anchored to the reference itself: it must be rtmi_render_samples_device.
The thin lens and the orthographic camera are held against tests/camera_ref.py, the float32 NumPy restatement of include/rtmi.h
on the oracle's closest hits, triangle records and RNG (tests/test_camera_cpu.py pins it to the oracle), so no expected value
comes from the code under test.  The two modes that are not bit-exact by design, RTMI_OPT_BVH and RTMI_OPT_FAST, are held against
the restatement fed by the product's own rtmi_trace; analytic spheres against rtmi_render_rays fed the restatement's rays.  The
references are computed once per case and shared."""
import numpy as np
import pytest

from conftest import assert_bits_equal, build_pair, recipe_canonical, recipe_circles_analytic
import camera_ref as CR
import rays_ref as RR

pytestmark = pytest.mark.gpu
F32 = np.float32
FULL = None  # tile: the whole frame through the host variant
LENS = dict(w=24, h=24, spp=4, seed=7, maxdepth=5, radius=0.05, focus=4.0)  # test 2's case
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _cam(model, radius=0.0, focus=1.0):
    from rust_raytrace_amd import _ffi
    return _ffi.Camera(model, 0, radius, focus)


def _ref(so, vp12, w, h, spp, seed, model, maxdepth, radius=0.0, focus=1.0, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), tuple(np.asarray(vp12, F32).tolist()), w, h, spp, seed, model, maxdepth, radius, focus,
           tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = CR.render(_orc(), so, vp12, w, h, spp, seed, CR.cam(model, radius, focus), maxdepth, **kw)
    return _REFS[key]


def _call(c, sp, vp, cam, sample0=0, nsamples=None, tile=FULL, accum=None, guides=True):
    """One call -> dict(image, accum, albedo, normal, ids, stats): the host variant for the whole frame, the device variant on
    torch tensors with guard words for a tile"""
    w = vp.width
    n = vp.samples_per_pixel - sample0 if nsamples is None else nsamples
    if tile is FULL:
        acc = np.zeros((vp.height, w, 4), F32) if accum is None else np.array(accum, F32)
        img = np.full((vp.height, w, 4), -7.0, F32)
        g = (True, True, True) if guides else (None, None, None)
        ctx = c.walk_samples_camera(vp, sp, 0, vp.height, cam, sample0, n, acc, img, *g)
        return dict(image=img, accum=acc, albedo=ctx.albedo, normal=ctx.normal, ids=ctx.ids, stats=ctx.stats)
    import torch
    npix = tile[1] * w
    sizes = dict(accum=npix * 4, out=npix * 4, albedo=npix * 4, normal=npix * 4, ids=npix)
    names = ("accum", "out") + (("albedo", "normal", "ids") if guides else ())
    bufs = {k: torch.full((sizes[k] + 128,), 7 if k == "ids" else 7.5, dtype=torch.int32 if k == "ids" else torch.float32, device="cuda:0")
            for k in names}
    if accum is not None:
        bufs["accum"][64:64 + npix * 4] = torch.from_numpy(np.ascontiguousarray(accum, F32).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx = c.walk_rays_camera_device(vp, sp, cam, tile=tile, sample0=sample0, nsamples=n, **{k: b[64:64 + sizes[k]] for k, b in bufs.items()})
    torch.cuda.synchronize()
    res = dict(albedo=None, normal=None, ids=None, stats=ctx.stats)
    for k, b in bufs.items():
        g = b.cpu().numpy()
        assert (g[:64] == g[0]).all() and (g[64 + sizes[k]:] == g[0]).all() and g[0] in (7, 7.5), f"guard words of {k}"
        a = g[64:64 + sizes[k]]
        res["image" if k == "out" else k] = a.view(np.uint32).reshape(tile[1], w) if k == "ids" else a.reshape(tile[1], w, 4)
    return res


def _assert_equal(got, ref, what, guides=True):
    assert_bits_equal(got["image"], ref.image, f"{what}: out")
    assert_bits_equal(got["accum"], ref.accum, f"{what}: accum")
    if guides:
        assert_bits_equal(got["albedo"], ref.albedo, f"{what}: albedo")
        assert_bits_equal(got["normal"], ref.normal, f"{what}: normal")
        assert np.array_equal(got["ids"], ref.ids), f"{what}: ids"
    assert got["stats"]["rays"] == ref.rays, f"{what}: rays {got['stats']['rays']} vs {ref.rays}"
    assert got["stats"]["pipeline"] == 1 and got["stats"]["slow_paths"] == 0


# ---------------------------------------------------------------- 1: the pinhole is rtmi_render_samples_device
@pytest.mark.parametrize("variant", ["device", "host"])
def test_pinhole_equals_render_samples(canonical_pair, variant):
    import torch
    R = _R()
    _, sp = canonical_pair
    w, h, spp = 33, 17, 4
    vp = R.canonical_viewport(w, h, 5, spp)
    c = R.HipRayCaster(seed=7)
    cam = c.camera_params(vp, "pinhole")
    tile = (1, 8, 2, 4)
    acc = np.zeros((8, w, 4), F32)  # the sums so far: both calls continue the same ones
    for k0, n in ((0, 1), (1, 3)):
        if variant == "device":  # the striped tile {1, 8, 2, 4}
            got = _call(c, sp, vp, cam, k0, n, tile=tile, accum=acc, guides=False)
            ta = torch.from_numpy(acc.reshape(-1).copy()).to("cuda:0")
            to = torch.zeros_like(ta)
            ctx = c.walk_samples_device(vp, sp, tile, k0, n, ta.data_ptr(), to.data_ptr())
            torch.cuda.synchronize()
            want_acc, want_out = ta.cpu().numpy().reshape(8, w, 4), to.cpu().numpy().reshape(8, w, 4)
        else:  # rows [1, 9)
            a0, img = acc.copy(), np.zeros((8, w, 4), F32)
            p = c.walk_samples_camera(vp, sp, 1, 8, cam, k0, n, a0, img)
            got = dict(image=img, accum=a0, stats=p.stats)
            want_acc, want_out = acc.copy(), np.zeros((8, w, 4), F32)
            ctx = c.walk_samples(vp, sp, 1, 8, k0, n, want_acc, want_out)
        assert_bits_equal(got["accum"], want_acc, f"{variant} [{k0}, {k0 + n}): accum")
        assert_bits_equal(got["image"], want_out, f"{variant} [{k0}, {k0 + n}): out")
        assert got["stats"]["rays"] == ctx.stats["rays"] > 0 and got["stats"]["pipeline"] == 1
        acc = want_acc
    assert np.abs(want_out).max() > 0 and len(np.unique(want_out)) > 100


# ---------------------------------------------------------------- 2: the thin lens
@pytest.fixture(scope="module")
def lens(canonical_pair):
    so, _ = canonical_pair
    c = LENS
    return _ref(so, _orc().canonical_viewport(c["w"], c["h"]), c["w"], c["h"], c["spp"], c["seed"], CR.THIN_LENS, c["maxdepth"], c["radius"], c["focus"])


def _lens_case():
    R, c = _R(), LENS
    return R.canonical_viewport(c["w"], c["h"], c["maxdepth"], c["spp"]), _cam(CR.THIN_LENS, c["radius"], c["focus"])


@pytest.mark.parametrize("variant", ["host", "device"])
def test_thin_lens_equals_the_restatement(canonical_pair, lens, variant):
    _, sp = canonical_pair
    vp, cam = _lens_case()
    got = _call(_R().HipRayCaster(seed=LENS["seed"]), sp, vp, cam, tile=FULL if variant == "host" else (0, 24, 24, 0))
    _assert_equal(got, lens, f"thin lens, {variant}")
    assert got["stats"]["trace_launches"] == LENS["maxdepth"] and got["stats"]["streams"] == 1
    assert (lens.cr.taken != 0).any() and lens.passes[3] > 0  # later candidates and deep paths take part
    assert not np.array_equal(lens.cr.o4, lens.cr.p)


def test_thin_lens_passes_continue_the_sums(canonical_pair, lens):
    so, sp = canonical_pair
    c = LENS
    vp, cam = _lens_case()
    caster = _R().HipRayCaster(seed=c["seed"])
    vo = _orc().canonical_viewport(c["w"], c["h"])
    first = _call(caster, sp, vp, cam, 0, 1)
    ref1 = _ref(so, vo, c["w"], c["h"], c["spp"], c["seed"], CR.THIN_LENS, c["maxdepth"], c["radius"], c["focus"], sample0=0, nsamples=1)
    _assert_equal(first, ref1, "samples [0, 1)")
    rest = _call(caster, sp, vp, cam, 1, 3, accum=first["accum"])
    ref2 = _ref(so, vo, c["w"], c["h"], c["spp"], c["seed"], CR.THIN_LENS, c["maxdepth"], c["radius"], c["focus"], sample0=1, nsamples=3,
                accum0=ref1.accum)
    _assert_equal(rest, ref2, "samples [1, 4)")  # the guides are those of samples 1..3
    assert_bits_equal(rest["image"], lens.image, "1 + 3 samples against one pass of 4: out")
    assert_bits_equal(rest["accum"], lens.accum, "1 + 3 samples against one pass of 4: accum")
    assert first["stats"]["rays"] + rest["stats"]["rays"] == lens.rays


def test_thin_lens_of_radius_zero(canonical_pair):
    so, sp = canonical_pair
    c = LENS
    ref = _ref(so, _orc().canonical_viewport(c["w"], c["h"]), c["w"], c["h"], c["spp"], c["seed"], CR.THIN_LENS, c["maxdepth"], 0.0, c["focus"])
    vp, _ = _lens_case()
    got = _call(_R().HipRayCaster(seed=c["seed"]), sp, vp, _cam(CR.THIN_LENS, 0.0, c["focus"]))
    _assert_equal(got, ref, "lens_radius = 0")


def test_maxdepth_zero_writes_zeros_and_still_gives_the_guides(canonical_pair):
    so, sp = canonical_pair
    c = LENS
    ref = _ref(so, _orc().canonical_viewport(16, 16), 16, 16, 2, c["seed"], CR.THIN_LENS, 0, c["radius"], c["focus"])
    got = _call(_R().HipRayCaster(seed=c["seed"]), sp, _R().canonical_viewport(16, 16, 0, 2), _cam(CR.THIN_LENS, c["radius"], c["focus"]))
    assert not got["image"].any() and not got["accum"].any() and not ref.image.any()
    assert_bits_equal(got["albedo"], ref.albedo, "albedo")
    assert_bits_equal(got["normal"], ref.normal, "normal")
    assert np.array_equal(got["ids"], ref.ids) and ref.ids.any()


# ---------------------------------------------------------------- 3: the orthographic camera
def test_ortho_tilted_camera(canonical_pair):
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    vo = RR.second_viewport(orc)
    ref = _ref(so, vo, 16, 16, 2, 7, CR.ORTHO, 5)
    # the second camera's orig / cam / vu / vv over a 16 x 16 frame, on both sides
    got = _call(R.HipRayCaster(seed=7), sp, R.Viewport(16, 16, vo, 5, 2), _cam(CR.ORTHO), tile=(0, 16, 16, 0))
    _assert_equal(got, ref, "ortho, tilted")
    assert (ref.ids != 0).any() and (ref.ids == 0).any()


def test_ortho_axis_aligned_camera_all_rays_have_zero_components(canonical_pair):
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    ref = _ref(so, orc.canonical_viewport(8, 8), 8, 8, 1, 7, CR.ORTHO, 5)
    assert ((ref.cr.d4[:, :3] == 0).sum(axis=1) == 2).all()
    got = _call(R.HipRayCaster(seed=7), sp, R.canonical_viewport(8, 8, 5, 1), _cam(CR.ORTHO, 9.0, -1.0))  # lens fields ignored
    _assert_equal(got, ref, "ortho, axis-aligned")


# ---------------------------------------------------------------- 4: scene kinds
KIND = dict(w=16, h=16, spp=2, seed=3, maxdepth=4)


def _kind(pair, options=0, trace=False):
    orc, R = _orc(), _R()
    so, sp = pair
    k = KIND
    caster = R.HipRayCaster(seed=k["seed"], options=options)
    kw = dict(trace=lambda o, d: caster.trace(sp, o, d)[:3]) if trace else {}
    ref = CR.render(orc, so, orc.canonical_viewport(k["w"], k["h"]), k["w"], k["h"], k["spp"], k["seed"],
                    CR.cam(CR.THIN_LENS, LENS["radius"], LENS["focus"]), k["maxdepth"], **kw)
    got = _call(caster, sp, R.canonical_viewport(k["w"], k["h"], k["maxdepth"], k["spp"]), _cam(CR.THIN_LENS, LENS["radius"], LENS["focus"]))
    return got, ref


def test_scene_kind_octree(canonical_pair):
    _assert_equal(*_kind(canonical_pair), "octree")


def test_scene_kind_linear_list():
    _assert_equal(*_kind(build_pair(recipe_canonical(accel="trivial"))), "linear list")


def test_scene_kind_generic_tree(canonical_pair):
    _assert_equal(*_kind(canonical_pair, _R().OPT_GENERIC), "RTMI_OPT_GENERIC")


@pytest.mark.parametrize("option", ["OPT_FAST", "OPT_BVH"])
def test_scene_kind_fast_and_bvh_against_their_own_trace(canonical_pair, option):
    _assert_equal(*_kind(canonical_pair, getattr(_R(), option), trace=True), option)


def test_scene_kind_analytic_spheres():
    orc, R = _orc(), _R()
    so, sp = build_pair(recipe_circles_analytic())
    k = KIND
    cr = CR.camera_rays(orc, orc.canonical_viewport(k["w"], k["h"]), k["w"], k["h"], k["spp"], k["seed"], CR.cam(CR.THIN_LENS, 0.05, 4.0))
    caster = R.HipRayCaster(seed=k["seed"])
    want, wctx = caster.walk_rays_explicit(sp, cr.o4, cr.d4, k["maxdepth"], group=k["spp"], keys=cr.keys, color=False, mean=True)
    vp, cam = R.canonical_viewport(k["w"], k["h"], k["maxdepth"], k["spp"]), _cam(CR.THIN_LENS, 0.05, 4.0)
    got = _call(caster, sp, vp, cam, guides=False)
    assert_bits_equal(got["image"].reshape(-1, 4), want["mean"], "analytic spheres: out")
    assert got["stats"]["rays"] == wctx.total_rays
    for tile in (FULL, (0, 16, 16, 0)):  # the guides are refused, and the handle stays usable
        with pytest.raises(RuntimeError, match="analytic spheres"):
            _call(caster, sp, vp, cam, tile=tile)
    again = _call(caster, sp, vp, cam, tile=(0, 16, 16, 0), guides=False)
    assert_bits_equal(again["image"], got["image"], "after the refusals")


# ---------------------------------------------------------------- 5, 6: tuning invariance and stats
# (tuning, sub-tiles, batches per sub-tile) for 24 x 24 x 4 = 2304 paths: 256 paths per batch -> 64 pixels -> 9 batches of the one
# sub-tile; three streams (subtile_min_paths lowered, or a tile this small stays whole) -> three sub-tiles of 8 rows, one batch each
@pytest.mark.parametrize("tuning,nsub,batches", [(dict(batch_paths=256), 1, 9), (dict(streams=1), 1, 1),
                                                  (dict(streams=3, subtile_min_paths=1), 3, 1)])
def test_tuning_changes_no_bit_and_stats_count_the_launches(canonical_pair, lens, tuning, nsub, batches):
    _, sp = canonical_pair
    vp, cam = _lens_case()
    got = _call(_R().HipRayCaster(seed=LENS["seed"], tuning=tuning), sp, vp, cam, tile=(0, 24, 24, 0))
    _assert_equal(got, lens, f"tuning {tuning}")
    st = got["stats"]
    assert st["streams"] == nsub and st["trace_launches"] == LENS["maxdepth"] * batches * nsub
    assert st["kernel_ms"] > 0 and st["trace_ms"] > 0


# ---------------------------------------------------------------- 7: walk_rays_camera
def test_walk_rays_camera_in_passes_of_one_sample(canonical_pair, lens):
    _, sp = canonical_pair
    vp, cam = _lens_case()
    c = _R().HipRayCaster(seed=LENS["seed"])
    one = np.zeros((24, 24, 4), F32)
    ctx1 = c.walk_rays_camera(vp, sp, one, cam, albedo=True, normal=True, ids=True)
    assert_bits_equal(one, lens.image, "one call of S samples")
    assert_bits_equal(ctx1.albedo, lens.albedo, "albedo")
    assert_bits_equal(ctx1.normal, lens.normal, "normal")
    assert np.array_equal(ctx1.ids, lens.ids)
    img = np.zeros((24, 24, 4), F32)
    ctx = c.walk_rays_camera(vp, sp, img, cam, pass_samples=1)
    assert_bits_equal(img, one, "passes of one sample against one call")
    assert_bits_equal(ctx.accum, lens.accum, "accum")
    assert ctx.samples_done == 4 and ctx.total_rays == ctx1.total_rays == lens.rays and ctx.albedo is None
    assert ctx.stats["trace_launches"] == 4 * LENS["maxdepth"]
