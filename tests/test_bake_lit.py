"""-m gpu: box lights on explicit rays and in the bake (rtmi_render_rays_lit*, rtmi_bake_lit*) bit for bit.  orig, dir and open
against tests/bake_ref.py, light and direct against tests/bake_lit_ref.py (the header's arithmetic in float32 NumPy on the oracle's
hits; tests/test_bake_lit_cpu.py pins it and holds it against float64 referees), light against rtmi_render_rays_lit_device on the
dumped rays, explicit rays against tests/lit_ref.py and against rtmi_render_lit_device's frame.  No tolerances.  The references
are computed once per case and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest as CT
from conftest import assert_bits_equal
import ao_ref as AR
import bake_lit_ref as BL
import bake_ref as BR
import env_ref as ER
import lit_ref as LT

pytestmark = pytest.mark.gpu
F32 = np.float32
OUTS = ("light", "open", "orig", "dir", "direct")
SEED, PIXEL0 = BL.SEED, BL.PIXEL0
AB, FOUR = BL.AB, BL.FOUR
_REFS = {}


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(caster, sp, pos4, nrm4, params, lights, inverse_square=False, want=OUTS, stream=None):
    """bake_lit_device on fresh, pre-filled tensors -> (dict of NumPy arrays, ctx)"""
    import torch
    M = nrm4.shape[0]
    n = M * params.rays
    shape = dict(light=(M, 4), open=(M,), orig=(n, 4), dir=(n, 4), direct=(M, 4))
    outs = {k: torch.full(shape[k], -7.0, device="cuda") for k in want}
    ctx = caster.bake_lit_device(sp, _dev(pos4), _dev(nrm4), params, caster.lit_params(lights, inverse_square), stream=stream, **outs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, ctx


def _plain(caster, sp, pos4, nrm4, params, want=("light", "open", "orig", "dir")):
    """rtmi_bake_device for the same arguments"""
    import torch
    M = nrm4.shape[0]
    n = M * params.rays
    shape = dict(light=(M, 4), open=(M,), orig=(n, 4), dir=(n, 4))
    outs = {k: torch.full(shape[k], -7.0, device="cuda") for k in want}
    ctx = caster.bake_device(sp, _dev(pos4), _dev(nrm4), params, **outs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, ctx


def _rays_lit(caster, sp, orig, dirs, maxdepth, lights, inverse_square=False, group=1, keys=None, pixel0=0, make_ray=False,
              want=("mean",), lit=True):
    """rtmi_render_rays_lit_device (lit=False: rtmi_render_rays_device) -> (dict of NumPy arrays, ctx)"""
    import torch
    n, ng = orig.shape[0], orig.shape[0] // group
    shape = dict(color=(n, 4), mean=(ng, 4), albedo=(ng, 4), normal=(ng, 4))
    outs = {k: torch.full(shape[k], -7.0, device="cuda") for k in want if k != "ids"}
    if "ids" in want:
        outs["ids"] = torch.full((ng,), 77, dtype=torch.int32, device="cuda")
    tk = _dev(np.ascontiguousarray(keys, np.uint32).view(np.int32)) if keys is not None else None
    kw = dict(group=group, keys=tk, pixel0=pixel0, make_ray=make_ray, **outs)
    if lit:
        ctx = caster.walk_rays_explicit_lit_device(sp, _dev(orig), _dev(dirs), maxdepth, caster.lit_params(lights, inverse_square), **kw)
    else:
        ctx = caster.walk_rays_explicit_device(sp, _dev(orig), _dev(dirs), maxdepth, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, ctx


def _ref(so, pos, nrm, K, depth, lights, **kw):
    """The restatement of one case on the oracle, computed once (tests must not modify it)"""
    key = (id(so), pos.tobytes(), nrm.tobytes(), K, depth, str(lights), tuple(sorted((k, id(v) if k == "env" else str(v)) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = BL.bake_lit_ref(_orc(), so, SEED, pos, nrm, K, depth, lights, **kw)
    return _REFS[key]


def _check(got, exp, what, outs=OUTS):
    for k in outs:
        assert_bits_equal(getattr(exp, k), got[k], f"{what}: {k}")


@pytest.fixture(scope="module")
def elements(canonical_pair):
    so, _ = canonical_pair
    return BL.elements(_orc(), so)


def _cycle(elements, M, step=7):
    pos, nrm = elements
    idx = (np.arange(M) * step) % pos.shape[0]
    return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx])


# ---------------------------------------------------------------- points and triangles
def test_points_equal_the_definition_and_render_rays_lit(canonical_pair, elements):
    R = _R()
    so, sp = canonical_pair
    pos, nrm = elements
    K, depth = 5, 3
    caster = R.HipRayCaster(seed=SEED)
    params = caster.bake_params("points", rays=K, maxdepth=depth, pixel0=PIXEL0)
    got, ctx = _call(caster, sp, pos, nrm, params, AB)
    exp = _ref(so, pos, nrm, K, depth, AB, pixel0=PIXEL0)
    plain = BR.bake_ref(_orc(), so, SEED, pos, nrm, K, depth, PIXEL0)
    for k in ("orig", "dir", "open"):
        assert_bits_equal(getattr(plain, k), got[k], f"{k} vs bake_ref")
    _check(got, exp, "points vs bake_lit_ref")
    assert not np.array_equal(plain.light, got["light"]) and got["direct"][:, :3].any() and not got["direct"][:, 3].any()
    mean, rctx = _rays_lit(caster, sp, got["orig"], got["dir"], depth, AB, group=K, pixel0=PIXEL0)
    assert_bits_equal(mean["mean"], got["light"], "light vs rtmi_render_rays_lit_device(mean) on those rays")
    assert ctx.total_rays == exp.rays == rctx.total_rays + exp.el.live
    assert ctx.stats["pipeline"] == 1 and ctx.stats["streams"] == 1 and ctx.stats["trace_launches"] == 2 * depth + 1
    assert rctx.stats["trace_launches"] == 2 * depth
    host, hctx = caster.bake_lit(sp, pos, nrm, params, AB, light=True, open=True, orig=True, dir=True, direct=True)
    for k in OUTS:
        assert_bits_equal(got[k], host[k], f"host variant: {k}")
    assert hctx.total_rays == exp.rays


def test_triangles_on_both_sides_equal_the_definition(canonical_pair):
    R = _R()
    so, sp = canonical_pair
    FIRST = 1000  # (triangles 1 .. 40, tests/test_bake.py's, see neither lamp from either side: every candidate is culled or occluded)
    corners, nrm = BR.scene_triangles(so, FIRST, 40)
    K, depth, pixel0 = 5, 3, 17
    caster = R.HipRayCaster(seed=SEED)
    params = caster.bake_params("triangles", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = _call(caster, sp, corners, nrm, params, AB)
    exp = _ref(so, corners, nrm, K, depth, AB, pixel0=pixel0, mode="triangles")
    plain = BR.bake_ref(_orc(), so, SEED, corners, nrm, K, depth, pixel0, mode="triangles")
    for k in ("orig", "dir", "open"):
        assert_bits_equal(getattr(plain, k), got[k], f"{k} vs bake_ref")
    _check(got, exp, "triangles vs bake_lit_ref")
    mean, _ = _rays_lit(caster, sp, got["orig"], got["dir"], depth, AB, group=K, pixel0=pixel0)
    assert_bits_equal(mean["mean"], got["light"], "light vs rtmi_render_rays_lit_device(mean) on those rays")
    assert ctx.total_rays == exp.rays
    assert not np.array_equal(got["direct"][:40], got["direct"][40:])  # the two sides differ
    assert exp.el.live > 50 and min(exp.el.visible) > 10
    host, hctx = caster.bake_lit(sp, corners, nrm, params, AB, light=True, open=True, orig=True, dir=True, direct=True)
    for k in OUTS:
        assert_bits_equal(got[k], host[k], f"host variant: {k}")
    rec, _, _ = so.triangles()
    front, _ = caster.bake_triangles_lit(sp, rec[FIRST:FIRST + 40, 20:29].reshape(40, 3, 3), rec[FIRST:FIRST + 40, 3:6], AB, rays=K, maxdepth=depth,
                                         pixel0=pixel0)
    for k in ("light", "direct"):
        assert_bits_equal(got[k][:40], front[k], f"bake_triangles_lit, front: {k}")


# ---------------------------------------------------------------- shapes, batches and keys
SHAPES = [(1, 1, 4), (85, 3, 4), (255, 1, 4), (257, 1, 4), (64, 5, 4), (341, 3, 4), (64, 5, 1)]


@pytest.mark.parametrize("M,K,depth", SHAPES)
def test_shapes_with_default_and_small_batches(canonical_pair, elements, M, K, depth):
    R = _R()
    so, sp = canonical_pair
    pos, nrm = _cycle(elements, M)
    exp = _ref(so, pos, nrm, K, depth, AB, pixel0=PIXEL0)
    if depth == 1:  # only the elements have candidates
        assert exp.pt.nlive == 0 and exp.el.live > 0
    # 101 is no multiple of 3 or 5: batches of 99 / 100 / 101 rays split the range mid-way
    for tuning in (None, {"batch_paths": 101}):
        caster = R.HipRayCaster(seed=SEED, tuning=tuning)
        params = caster.bake_params("points", rays=K, maxdepth=depth, pixel0=PIXEL0)
        got, ctx = _call(caster, sp, pos, nrm, params, AB)
        _check(got, exp, f"tuning {tuning}")
        assert ctx.total_rays == exp.rays
        nbatch = 1 if tuning is None else -(-M // max(101 // K, 1))
        assert ctx.stats["trace_launches"] == nbatch * (2 * depth + 1)
        host, _ = caster.bake_lit(sp, pos, nrm, params, AB, light=True, open=True, orig=True, dir=True, direct=True)
        for k in OUTS:
            assert_bits_equal(got[k], host[k], f"host variant: {k}, tuning {tuning}")
    R.HipRayCaster().upload(sp)  # back to the library's defaults for the tests that share the scene


def test_pixel0_is_the_key_and_a_split_call_changes_nothing(canonical_pair, elements):
    R = _R()
    _, sp = canonical_pair
    M, K, depth = 64, 5, 4
    pos, nrm = _cycle(elements, M, 1)
    caster = R.HipRayCaster(seed=SEED)
    whole, _ = _call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=900), AB)
    other, _ = _call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=901), AB)
    for k in ("light", "direct"):
        assert not np.array_equal(whole[k], other[k]), k
    cut = 23
    a, _ = _call(caster, sp, pos[:cut], nrm[:cut], caster.bake_params(rays=K, maxdepth=depth, pixel0=900), AB)
    b, _ = _call(caster, sp, pos[cut:], nrm[cut:], caster.bake_params(rays=K, maxdepth=depth, pixel0=900 + cut), AB)
    for k in OUTS:
        assert_bits_equal(whole[k], np.concatenate([a[k], b[k]]), f"two calls with pixel0 advanced by hand: {k}")


# ---------------------------------------------------------------- lights
def test_one_light(canonical_pair, elements):
    so, sp = canonical_pair
    pos, nrm = elements
    caster = _R().HipRayCaster(seed=SEED)
    got, ctx = _call(caster, sp, pos, nrm, caster.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=PIXEL0), (LT.A,))
    exp = _ref(so, pos, nrm, BL.K, BL.DEPTH, (LT.A,), pixel0=PIXEL0)
    _check(got, exp, "one light")
    assert ctx.total_rays == exp.rays


def test_four_lights_one_unbounded_one_with_its_own_bias_inverse_square(canonical_pair, elements):
    so, sp = canonical_pair
    pos, nrm = elements
    caster = _R().HipRayCaster(seed=SEED)
    got, ctx = _call(caster, sp, pos, nrm, caster.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=PIXEL0), FOUR, True)
    exp = _ref(so, pos, nrm, BL.K, BL.DEPTH, FOUR, pixel0=PIXEL0, inverse_square=True)
    _check(got, exp, "four lights, inverse square")
    assert ctx.total_rays == exp.rays and exp.el.live > pos.shape[0] * BL.K  # more live rays than the batch has entries: up to 4 each
    plain = _ref(so, pos, nrm, BL.K, BL.DEPTH, FOUR, pixel0=PIXEL0)
    assert not np.array_equal(plain.direct, exp.direct)


def test_a_light_far_behind_every_candidate_culled_no_walk_ray(canonical_pair, elements):
    so, sp = canonical_pair
    pos, nrm = elements
    caster = _R().HipRayCaster(seed=SEED)
    params = caster.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=PIXEL0)
    got, ctx = _call(caster, sp, pos, nrm, params, (LT.FAR_BEHIND,))
    exp = _ref(so, pos, nrm, BL.K, BL.DEPTH, (LT.FAR_BEHIND,), pixel0=PIXEL0)
    assert exp.el.live == 0 and exp.pt.nlive == 0 and exp.el.culled[0] == pos.shape[0] * BL.K
    _check(got, exp, "light far behind")
    assert not got["direct"].view(np.uint32).any()
    _, pctx = _plain(caster, sp, pos, nrm, params)
    assert ctx.total_rays == pctx.total_rays == exp.rays


def test_without_lights_the_calls_are_the_plain_ones(canonical_pair, elements):
    so, sp = canonical_pair
    pos, nrm = elements
    caster = _R().HipRayCaster(seed=SEED)
    params = caster.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=PIXEL0)
    got, ctx = _call(caster, sp, pos, nrm, params, ())
    plain, pctx = _plain(caster, sp, pos, nrm, params)
    for k in ("light", "open", "orig", "dir"):
        assert_bits_equal(plain[k], got[k], f"nlights = 0 against rtmi_bake_device: {k}")
    assert not got["direct"].view(np.uint32).any() and ctx.total_rays == pctx.total_rays
    want = ("color", "mean", "albedo", "normal", "ids")
    a, actx = _rays_lit(caster, sp, got["orig"], got["dir"], BL.DEPTH, (), group=BL.K, pixel0=PIXEL0, want=want)
    b, bctx = _rays_lit(caster, sp, got["orig"], got["dir"], BL.DEPTH, (), group=BL.K, pixel0=PIXEL0, want=want, lit=False)
    for k in want:
        assert_bits_equal(b[k], a[k], f"nlights = 0 against rtmi_render_rays_device: {k}")
    assert actx.total_rays == bctx.total_rays and actx.stats["trace_launches"] == 2 * BL.DEPTH


# ---------------------------------------------------------------- explicit rays against the frame
def test_explicit_rays_equal_the_restatement_and_the_lit_frame(canonical_pair):
    import torch
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    w = h = 32
    spp, depth, seed = 4, 4, 5
    ref = LT.render(orc, so, orc.canonical_viewport(w, h), w, h, spp, seed, depth, AB)
    keys = np.stack([ref.pixel, ref.sample], axis=1).astype(np.uint32)
    caster = R.HipRayCaster(seed=seed)
    want = ("color", "mean", "albedo", "normal", "ids")
    got, ctx = _rays_lit(caster, sp, ref.o4, ref.d4, depth, AB, group=spp, keys=keys, want=want)
    assert_bits_equal(ref.color, got["color"], "color vs lit_ref.path_trace")
    assert ctx.total_rays == ref.rays + ref.nlive and ctx.stats["trace_launches"] == 2 * depth
    vp = R.canonical_viewport(w, h, depth, spp)
    acc, out = (torch.zeros(h * w * 4, dtype=torch.float32, device="cuda") for _ in range(2))
    fctx = caster.walk_rays_lit_device(vp, sp, AB, acc, out)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy().reshape(-1, 4), got["mean"], "mean vs rtmi_render_lit_device's out")
    assert fctx.total_rays == ctx.total_rays
    # without keys a ray's key is (pixel0 + its group, its place in the group): the same keys here
    nokeys, _ = _rays_lit(caster, sp, ref.o4, ref.d4, depth, AB, group=spp, want=want)
    plain, _ = _rays_lit(caster, sp, ref.o4, ref.d4, depth, AB, group=spp, keys=keys, want=("albedo", "normal", "ids"), lit=False)
    for k in want:
        assert_bits_equal(got[k], nokeys[k], f"keys = NULL: {k}")
    for k in ("albedo", "normal", "ids"):
        assert_bits_equal(plain[k], got[k], f"the guides are rtmi_render_rays_device's: {k}")
    # RTMI_RAYS_MAKE_RAY: the library normalises as vunit does
    raw = (ref.d4 * F32(2.0)).astype(F32)
    made, _ = _rays_lit(caster, sp, ref.o4, raw, depth, AB, group=spp, keys=keys, make_ray=True, want=("color", "mean"))
    unit, _ = _rays_lit(caster, sp, ref.o4, AR.vunit(raw), depth, AB, group=spp, keys=keys, want=("color", "mean"))
    for k in ("color", "mean"):
        assert_bits_equal(unit[k], made[k], f"make_ray: {k}")
    host, hctx = caster.walk_rays_explicit_lit(sp, ref.o4, ref.d4, depth, AB, group=spp, keys=keys, color=True, mean=True)
    for k in ("color", "mean"):
        assert_bits_equal(got[k], host[k], f"host variant: {k}")
    assert hctx.total_rays == ctx.total_rays
    zero, zctx = _rays_lit(caster, sp, ref.o4, ref.d4, 0, AB, group=spp, want=("color", "mean"))
    assert not zero["color"].view(np.uint32).any() and not zero["mean"].view(np.uint32).any() and zctx.total_rays == 0


# ---------------------------------------------------------------- scene kinds
def _kind_case(pair, lights=AB, options=0, exact=True, env=None):
    orc, R = _orc(), _R()
    so, sp = pair
    pos, nrm = BL.elements(orc, so)
    K, depth = 4, 4
    caster = R.HipRayCaster(seed=SEED, options=options)
    got, ctx = _call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=50), lights)
    mean, rctx = _rays_lit(caster, sp, got["orig"], got["dir"], depth, lights, group=K, pixel0=50)
    assert_bits_equal(mean["mean"], got["light"], "light vs the handle's own rtmi_render_rays_lit_device on the dumped rays")
    alone, actx = _call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=50), lights, want=("direct",))
    assert_bits_equal(alone["direct"], got["direct"], "direct alone")
    assert ctx.total_rays == rctx.total_rays + actx.total_rays
    if exact:
        exp = BL.bake_lit_ref(orc, so, SEED, pos, nrm, K, depth, lights, pixel0=50, env=env)
        _check(got, exp, "vs bake_lit_ref")
        assert ctx.total_rays == exp.rays and exp.el.live > 20 and sum(exp.el.occluded) > 5 and exp.pt.nlive > 10
    return got


def test_scene_kind_linear_list():
    _kind_case(CT.build_pair(CT.recipe_canonical(accel="trivial", obj=CT.TEAPOT)))


def test_scene_kind_generic_tree(canonical_pair):
    _kind_case(canonical_pair, options=_R().OPT_GENERIC)


def test_scene_with_an_environment():
    sun = dict(sun_dir=(-0.75, 0.25, 0.6), sun_cos=0.95, sun_color=(30.0, 24.0, 16.0))
    so, sp = CT.build_pair(CT.recipe_canonical())
    sp.set_sky(16, **sun)
    from types import SimpleNamespace
    lit = _kind_case((so, sp), env=SimpleNamespace(table=ER.sky_table(16, sun), frame=None))
    dark = _ref(so, *BL.elements(_orc(), so), 4, 4, AB, pixel0=50)
    assert not np.array_equal(lit["light"], dark.light)
    assert_bits_equal(dark.direct, lit["direct"], "the elements' own light does not see the sky")


@pytest.mark.parametrize("option", ["OPT_BVH", "OPT_FAST"])
def test_scene_kind_bvh_and_fast_equal_their_own_render_rays_lit(canonical_pair, option):
    got = _kind_case(canonical_pair, options=getattr(_R(), option), exact=False)
    assert np.isfinite(got["direct"]).all() and got["direct"][:, :3].any()


# ---------------------------------------------------------------- output options
def test_every_output_alone_and_direct_does_not_depend_on_maxdepth(canonical_pair, elements):
    R = _R()
    so, sp = canonical_pair
    M, K, depth = 85, 3, 4
    pos, nrm = _cycle(elements, M, 1)
    caster = R.HipRayCaster(seed=SEED)
    params = caster.bake_params(rays=K, maxdepth=depth, pixel0=3)
    full, fctx = _call(caster, sp, pos, nrm, params, AB)
    exp = _ref(so, pos, nrm, K, depth, AB, pixel0=3)
    _check(full, exp, "all outputs")
    for k in OUTS:
        one, ctx = _call(caster, sp, pos, nrm, params, AB, want=(k,))
        assert_bits_equal(full[k], one[k], f"{k} alone")
        # only what the output needs is traced: nothing for the rays, pass 0 for open, every pass and its walk for light, the
        # elements' walk alone for direct (no gather ray)
        assert ctx.stats["trace_launches"] == dict(light=2 * depth, open=1, orig=0, dir=0, direct=1)[k]
        assert ctx.total_rays == dict(light=exp.pt.rays + exp.pt.nlive, open=M * K, orig=0, dir=0, direct=exp.el.live)[k]
        host, _ = caster.bake_lit(sp, pos, nrm, params, AB, **{o: o == k for o in OUTS})
        assert_bits_equal(full[k], host[k], f"{k} alone, host variant")
    for d in (0, 1):
        got, ctx = _call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=d, pixel0=3), AB)
        assert_bits_equal(full["direct"], got["direct"], f"direct at maxdepth {d}")
        for k in ("open", "orig", "dir"):
            assert_bits_equal(full[k], got[k], f"{k} at maxdepth {d}")
        if d == 0:
            assert not got["light"].view(np.uint32).any() and ctx.total_rays == M * K + exp.el.live
            assert ctx.stats["trace_launches"] == 2


# ---------------------------------------------------------------- streams
def test_elements_made_on_a_torch_stream_just_before_the_call(canonical_pair, elements):
    import torch
    R = _R()
    so, sp = canonical_pair
    pos, nrm = elements
    M = pos.shape[0]
    exp = _ref(so, pos, nrm, BL.K, BL.DEPTH, AB, pixel0=PIXEL0)
    src_p, src_n = _dev(pos * F32(0.5)), _dev(nrm)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    light, direct = torch.full((M, 4), -7.0, device="cuda"), torch.full((M, 4), -7.0, device="cuda")
    caster = R.HipRayCaster(seed=SEED)
    with torch.cuda.stream(stream):
        big = torch.ones(1 << 24, device="cuda")
        for _ in range(8):  # work in front of the elements on that stream
            big = big * 1.0001
        tp = src_p * 2.0  # exact: the points again
        tn = src_n.clone()
        ctx = caster.bake_lit_device(sp, tp, tn, caster.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=PIXEL0), AB, light=light, direct=direct,
                                     stream=stream)
        out_l, out_d = light.clone(), direct.clone()  # ordered behind the call on the same stream
    stream.synchronize()
    assert_bits_equal(exp.light, out_l.cpu().numpy(), "light of elements produced on the stream")
    assert_bits_equal(exp.direct, out_d.cpu().numpy(), "direct of elements produced on the stream")
    assert ctx.total_rays == exp.pt.rays + exp.pt.nlive + exp.el.live


# ---------------------------------------------------------------- refusals: nothing is launched, nothing is written
def test_every_refusal_leaves_the_outputs_untouched():
    import torch
    import test_bake_lit_cpu as TC
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    M, K = 12, 4
    bufs = dict(pos=torch.full((3 * M, 4), 2.5, device="cuda"), nrm=torch.full((M, 4), 2.5, device="cuda"),
                light=torch.full((M, 4), -7.0, device="cuda"), open=torch.full((M,), -7.0, device="cuda"),
                orig=torch.full((M * K, 4), -7.0, device="cuda"), dir=torch.full((M * K, 4), -7.0, device="cuda"),
                direct=torch.full((M, 4), -7.0, device="cuda"), keys=torch.full((M * K, 2), 3, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    B = TC.TB
    real = {B.POS: bufs["pos"].data_ptr(), B.NRM: bufs["nrm"].data_ptr(), B.LIGHT: bufs["light"].data_ptr(), B.OPEN: bufs["open"].data_ptr(),
            B.ORIG: bufs["orig"].data_ptr(), B.DIR: bufs["dir"].data_ptr(), TC.DIRECT: bufs["direct"].data_ptr()}

    def sub(p, table=real):
        """a stand-in address, or one inside its buffer, becomes the real buffer's (the far-apart ones, for counts no buffer could hold, stay)"""
        for base, ptr in table.items():
            if base <= p < base + 0x100000:
                return ptr + (p - base)
        return p
    for code, word, kw in TC.BAKE_REFUSALS:
        args = dict(pos=B.POS, nrm=B.NRM, out=(B.LIGHT, B.OPEN, B.ORIG, B.DIR, TC.DIRECT))
        args.update(kw)
        args["pos"], args["nrm"] = sub(args["pos"]), sub(args["nrm"])
        if args["out"] is not None:
            args["out"] = tuple(sub(p) for p in args["out"])
        for rc, msg, rays in TC.bake_both(**args):
            assert rc == code and word in msg and rays == 0, (kw, rc, msg)
            assert L.rtmi_last_error() == msg
    # explicit rays: orig / dir of the bake stand for the rays, light for color, direct for mean
    rreal = {TC.R_ORIG: bufs["orig"].data_ptr(), TC.R_DIR: bufs["dir"].data_ptr(), TC.R_KEYS: bufs["keys"].data_ptr(),
             TC.R_COLOR: bufs["light"].data_ptr(), TC.R_MEAN: bufs["direct"].data_ptr()}
    for code, word, kw in TC.RAYS_REFUSALS:
        args = dict(n=M, orig=TC.R_ORIG, dirs=TC.R_DIR, keys=TC.R_KEYS, out=(TC.R_COLOR, TC.R_MEAN, 0, 0, 0))
        args.update(kw)
        for k in ("orig", "dirs", "keys"):
            args[k] = sub(args[k], rreal)
        if args["out"] is not None:
            args["out"] = tuple(sub(p, rreal) for p in args["out"])
        for rc, msg, rays in TC.rays_both(**args):
            assert rc == code and word in msg and rays == 0, (kw, rc, msg)
    torch.cuda.synchronize()
    for k in OUTS:
        assert (bufs[k] == -7.0).all().item(), k
    assert (bufs["pos"] == 2.5).all().item() and (bufs["nrm"] == 2.5).all().item() and (bufs["keys"] == 3).all().item()


def _refused(c, sp, word, pos, nrm):
    import torch
    params = c.bake_params(rays=4, maxdepth=4)
    with pytest.raises(RuntimeError, match=word):
        c.bake_lit(sp, pos, nrm, params, AB)
    light, direct = (torch.full((pos.shape[0], 4), -7.0, device="cuda") for _ in range(2))
    with pytest.raises(RuntimeError, match=word):
        c.bake_lit_device(sp, _dev(pos), _dev(nrm), params, AB, light=light, direct=direct)
    o4, d4 = np.ascontiguousarray(pos), np.ascontiguousarray(nrm)
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_explicit_lit(sp, o4, d4, 4, AB)
    color = torch.full((pos.shape[0], 4), -7.0, device="cuda")
    with pytest.raises(RuntimeError, match=word):
        c.walk_rays_explicit_lit_device(sp, _dev(o4), _dev(d4), 4, AB, color=color)
    torch.cuda.synchronize()
    for t in (light, direct, color):
        assert (t == -7.0).all().item()


def test_scenes_the_calls_do_not_take_are_refused_and_the_handle_stays_usable():
    import glass_cases as GC
    import tex_cases as TXC
    orc, R = _orc(), _R()
    NTEAPOT = 6320
    c = R.HipRayCaster(seed=SEED)
    so, sp = CT.build_pair(CT.recipe_canonical())
    pos, nrm = BL.elements(orc, so)
    pos, nrm = pos[:24], nrm[:24]
    sp.smooth_normals(1, NTEAPOT)
    _refused(c, sp, "vertex normals", pos, nrm)
    sp.clear_vertex_normals()
    sp.set_textures([TXC.images()[3]], None, None)
    sp.project_uvs(1, NTEAPOT, (-1.7, -0.4, 3.1), 0.9, 1)
    _refused(c, sp, "textures", pos, nrm)
    sp.set_normal_maps(np.full(NTEAPOT, 1, np.uint32))
    _refused(c, sp, "normal maps", pos, nrm)
    sp.clear_textures()
    _refused(R.HipRayCaster(seed=SEED), GC.build_pair(GC.recipe_slab())[1], "dielectric", pos, nrm)
    _refused(R.HipRayCaster(seed=SEED), CT.recipe_circles_analytic()(CT.ProductApi(R)), "analytic spheres", pos, nrm)
    # bad parameters past Python's checks: the library refuses
    bad = c.lit_params(AB)
    bad.lights[1].rays = 2
    with pytest.raises(RuntimeError, match="light 1"):
        c.bake_lit(sp, pos, nrm, c.bake_params(rays=4), bad)
    with pytest.raises(RuntimeError, match="light 1"):
        c.walk_rays_explicit_lit(sp, pos, nrm, 4, bad)
    # ... and the same handle bakes with lamps once the scene is one the call takes; then an ordinary frame and a plain bake are exact
    params = c.bake_params(rays=4, maxdepth=4, pixel0=9)
    got, ctx = _call(c, sp, pos, nrm, params, AB)
    exp = BL.bake_lit_ref(orc, so, SEED, pos, nrm, 4, 4, AB, pixel0=9)
    _check(got, exp, "after the refusals")
    w, h, spp = 24, 20, 2
    want, cn = so.render(w, h, orc.canonical_viewport(w, h), 5, spp, seed=9, threads=8)
    img = np.zeros((h, w, 4), np.float32)
    fctx = R.HipRayCaster(seed=9).walk_rays(R.canonical_viewport(w, h, 5, spp), sp, img, 1, False)
    assert_bits_equal(want, img, "the plain frame after the lit bake")
    assert fctx.total_rays == cn["rays"]
    plain, _ = _plain(c, sp, pos, nrm, params)
    pref = BR.bake_ref(orc, so, SEED, pos, nrm, 4, 4, 9)
    for k in ("light", "open", "orig", "dir"):
        assert_bits_equal(getattr(pref, k), plain[k], f"the plain bake after the lit bake: {k}")


def test_a_refused_scene_returns_unsupported_with_cleared_stats_through_the_raw_abi():
    """What the Python layer's exception hides: rc == RTMI_ERR_UNSUPPORTED and stats cleared, for the four entry points, on a real
    handle with vertex normals; with them removed the handle bakes with lamps"""
    from test_gpu_abi_raw import _abi_arrays, _boxes, _create, _lib
    orc = _orc()
    L, ffi = _lib()
    so = CT.recipe_circles(maxdepth=4, minobjs=6)(CT.OracleApi(orc))
    tris, geo, topo, refs = _abi_arrays(so)
    rc, hnd = _create(L, tris, _boxes(geo, topo), refs)
    assert rc == 0, L.rtmi_last_error()
    try:
        o4, d4 = orc.primary_rays(8, 8, orc.canonical_viewport(8, 8), 1)
        tri, t, face, _ = so.trace(o4, d4)
        hit = np.nonzero(np.asarray(tri) != 0)[0][:16]
        assert len(hit) >= 8
        pos = np.ascontiguousarray(((d4[hit] * np.asarray(t, F32)[hit, None]).astype(F32) + o4[hit]).astype(F32))
        nrm = np.ascontiguousarray((d4[hit] * F32(-1.0)).astype(F32))
        M, K = len(hit), 3
        light, direct, color = np.full((M, 4), 3.0, F32), np.full((M, 4), 5.0, F32), np.full((M, 4), 6.0, F32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lit = _R().HipRayCaster.lit_params(AB)
        bake = ffi.Bake(0, K, 4, 11, 0, 0.001)
        bout = ffi.BakeLitOut(p(light), None, None, None, p(direct))
        rays = ffi.Rays(4, 1, 0, 0)
        rout = ffi.RaysOut(p(color), None, None, None, None)

        def calls():
            st = ffi.Stats()
            st.rays, st.trace_launches = 123, 7
            yield L.rtmi_bake_lit(hnd, M, p(pos), p(nrm), SEED, C.byref(bake), C.byref(lit), C.byref(bout), C.byref(st)), st
            st = ffi.Stats()
            st.rays, st.trace_launches = 123, 7  # (refused before the pointers are used: host memory will do)
            yield L.rtmi_bake_lit_device(hnd, M, p(pos), p(nrm), SEED, C.byref(bake), C.byref(lit), C.byref(bout), None, C.byref(st)), st
            st = ffi.Stats()
            st.rays, st.trace_launches = 123, 7
            yield L.rtmi_render_rays_lit(hnd, M, p(pos), p(nrm), None, SEED, C.byref(rays), C.byref(lit), C.byref(rout), C.byref(st)), st
            st = ffi.Stats()
            st.rays, st.trace_launches = 123, 7
            yield L.rtmi_render_rays_lit_device(hnd, M, p(pos), p(nrm), None, SEED, C.byref(rays), C.byref(lit), C.byref(rout), None, C.byref(st)), st
        rec, _, _ = so.triangles()
        n = rec.shape[0]
        corners = np.ascontiguousarray(rec[:, 20:29])
        vn = np.ascontiguousarray(np.repeat(rec[:, None, 3:6], 3, axis=1).astype(F32))
        assert L.rtmi_scene_set_normals(hnd, p(corners), p(vn), n) == 0, L.rtmi_last_error()
        for rc, st in calls():
            assert rc == 3 and b"vertex normals" in L.rtmi_last_error(), (rc, L.rtmi_last_error())  # RTMI_ERR_UNSUPPORTED
            assert st.rays == 0 and st.trace_launches == 0 and st.kernel_ms == 0
        assert (light == 3.0).all() and (direct == 5.0).all() and (color == 6.0).all()
        assert L.rtmi_scene_set_normals(hnd, p(corners), None, n) == 0, L.rtmi_last_error()
        st = ffi.Stats()
        assert L.rtmi_bake_lit(hnd, M, p(pos), p(nrm), SEED, C.byref(bake), C.byref(lit), C.byref(bout), C.byref(st)) == 0, L.rtmi_last_error()
        exp = BL.bake_lit_ref(orc, so, SEED, pos, nrm, K, 4, AB, pixel0=11, want_open=False)
        assert_bits_equal(exp.light, light, "raw ABI: light")
        assert_bits_equal(exp.direct, direct, "raw ABI: direct")
        assert st.rays == exp.rays
    finally:
        L.rtmi_scene_destroy(hnd)


# ---------------------------------------------------------------- the walk's two routes
_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import conftest as CT
from oracle import orc
from rust_raytrace_amd import raytrace as R
import bake_lit_ref as BL
so, sp = CT.build_pair(CT.recipe_canonical())
pos, nrm = BL.elements(orc, so)
c = R.HipRayCaster(seed=BL.SEED)
got, ctx = c.bake_lit(sp, pos, nrm, c.bake_params(rays=BL.K, maxdepth=BL.DEPTH, pixel0=BL.PIXEL0), BL.AB)
np.savez({out!r}, light=got["light"], direct=got["direct"], rays=np.array([ctx.total_rays]))
"""


def test_the_any_hit_route_gives_the_same_bits(canonical_pair, elements, tmp_path):
    """RTMI_LIT_FROM_HITS=0 is read when the scene is created: a fresh child process bakes with the any-hit kernel"""
    so, sp = canonical_pair
    pos, nrm = elements
    exp = _ref(so, pos, nrm, BL.K, BL.DEPTH, AB, pixel0=PIXEL0)
    out = str(tmp_path / "anyhit.npz")
    code = _CHILD.format(root=CT.ROOT, tests=os.path.join(CT.ROOT, "tests"), out=out)
    env = dict(os.environ, RTMI_LIT_FROM_HITS="0")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
    got = np.load(out)
    assert_bits_equal(exp.light, got["light"], "any-hit route: light")
    assert_bits_equal(exp.direct, got["direct"], "any-hit route: direct")
    assert int(got["rays"][0]) == exp.pt.rays + exp.pt.nlive + exp.el.live  # (light and direct: the gather rays are in the paths' count)
