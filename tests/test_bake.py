"""-m gpu: the light bake (rtmi_bake / rtmi_bake_device) bit for bit.  The gather rays against tests/bake_ref.py (the header's
arithmetic in float32 NumPy), `light` against rtmi_render_rays_device on those very rays and against the oracle (the anchor of
tests/test_bake_cpu.py), `open` against the oracle's closest hits; one statistical case against the float64 referee
(tests/draw_ref.py).  No tolerances."""
import numpy as np
import pytest

from conftest import ProductApi, assert_bits_equal, build_pair, recipe_canonical, recipe_circles_analytic
import bake_ref as BR
import test_bake_cpu as TB

pytestmark = pytest.mark.gpu
F32 = np.float32
OUTS = ("light", "open", "orig", "dir")
SEED = BR.ANCHOR["seed"]


def _orc():
    from oracle import orc
    return orc


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_call(caster, sp, pos4, nrm4, params, want=OUTS, stream=None):
    """bake_device on fresh, pre-filled tensors -> (dict of NumPy arrays, ctx)"""
    import torch
    M = nrm4.shape[0]
    n = M * params.rays
    shape = dict(light=(M, 4), open=(M,), orig=(n, 4), dir=(n, 4))
    outs = {k: torch.full(shape[k], -7.0, device="cuda") for k in want}
    ctx = caster.bake_device(sp, _dev(pos4), _dev(nrm4), params, stream=stream, **outs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, ctx


def _rays_mean(caster, sp, orig, dirs, maxdepth, K, pixel0):
    """rtmi_render_rays_device(mean) on dumped gather rays: keys = NULL, group = K, the same pixel0"""
    import torch
    mean = torch.full((orig.shape[0] // K, 4), -7.0, device="cuda")
    ctx = caster.walk_rays_explicit_device(sp, _dev(orig), _dev(dirs), maxdepth, group=K, pixel0=pixel0, mean=mean)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), ctx


def _own_open(caster, sp, orig, dirs, K):
    """open from the handle's own rtmi_trace of dumped gather rays"""
    tri, _, _, _ = caster.trace(sp, orig, dirs)
    return BR.open_from_hits(tri, K)


@pytest.fixture(scope="module")
def elements(canonical_pair):
    """The first hits of the canonical 16 x 16 view (points and normals) that every shape cycles through"""
    so, _ = canonical_pair
    return BR.first_hit_points(_orc(), so, 16, 16)


# ---------------------------------------------------------------- the rays, light and open of points and of triangles
def test_points_equal_the_definition_the_oracle_and_render_rays(canonical_pair):
    R = _R()
    so, sp = canonical_pair
    a, A = BR.ANCHOR, TB.anchor(so)
    caster = R.HipRayCaster(seed=a["seed"])
    params = caster.bake_params("points", rays=a["K"], maxdepth=a["maxdepth"], pixel0=a["pixel0"])
    got, ctx = _device_call(caster, sp, A["pos"], A["nrm"], params)
    exp = A["full"]
    assert_bits_equal(exp.orig, got["orig"], "orig vs bake_ref")
    assert_bits_equal(exp.dir, got["dir"], "dir vs bake_ref")
    assert_bits_equal(exp.light, got["light"], "light vs the oracle")
    assert_bits_equal(exp.open, got["open"], "open vs the oracle's closest hits")
    mean, rctx = _rays_mean(caster, sp, got["orig"], got["dir"], a["maxdepth"], a["K"], a["pixel0"])
    assert_bits_equal(mean, got["light"], "light vs rtmi_render_rays_device(mean) on those rays")
    assert ctx.total_rays == rctx.total_rays == exp.rays
    assert ctx.stats["pipeline"] == 1 and ctx.stats["streams"] == 1 and ctx.stats["trace_launches"] == a["maxdepth"]
    assert got["open"][-1] == F32(1.0)  # the sky point
    # depth 1: the sky point's light is the sky's colour folded
    one, _ = _device_call(caster, sp, A["pos"], A["nrm"], caster.bake_params("points", rays=a["K"], maxdepth=1, pixel0=a["pixel0"]), want=("light", "open"))
    assert_bits_equal(A["one"].light, one["light"], "light at depth 1 vs the oracle")
    assert_bits_equal(A["one"].open, one["open"], "open at depth 1")
    # the host variant: the same bits
    host, hctx = caster.bake(sp, A["pos"], A["nrm"], params, light=True, open=True, orig=True, dir=True)
    for k in OUTS:
        assert_bits_equal(got[k], host[k], f"host variant: {k}")
    assert hctx.total_rays == exp.rays


def test_triangles_on_both_sides_equal_the_definition(canonical_pair):
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    corners, nrm = BR.scene_triangles(so, 1, 40)
    K, depth, pixel0 = 5, 3, 17
    caster = R.HipRayCaster(seed=SEED)
    params = caster.bake_params("triangles", rays=K, maxdepth=depth, pixel0=pixel0)
    got, ctx = _device_call(caster, sp, corners, nrm, params)
    exp = BR.bake_ref(orc, so, SEED, corners, nrm, K, depth, pixel0, mode="triangles")
    assert exp.orig.shape == (80 * K, 4) and len(np.unique(exp.uv, axis=0)) == 80 * K
    assert_bits_equal(exp.orig, got["orig"], "orig vs bake_ref")
    assert_bits_equal(exp.dir, got["dir"], "dir vs bake_ref")
    assert_bits_equal(exp.open, got["open"], "open vs the oracle's closest hits")
    assert_bits_equal(exp.light, got["light"], "light vs the oracle")
    mean, _ = _rays_mean(caster, sp, got["orig"], got["dir"], depth, K, pixel0)
    assert_bits_equal(mean, got["light"], "light vs rtmi_render_rays_device(mean) on those rays")
    assert ctx.total_rays == exp.rays
    assert not np.array_equal(got["light"][:40], got["light"][40:])  # the two sides differ
    # the convenience wrapper and the host variant
    rec, _, _ = so.triangles()
    c3 = rec[1:41, 20:29].reshape(40, 3, 3)
    n3 = rec[1:41, 3:6]
    front, _ = caster.bake_triangles(sp, c3, n3, rays=K, maxdepth=depth, pixel0=pixel0, open=True, orig=True, dir=True)
    back, _ = caster.bake_triangles(sp, c3, -n3, rays=K, maxdepth=depth, pixel0=pixel0 + 40, open=True)
    for k in OUTS:
        assert_bits_equal(got[k][:front[k].shape[0]], front[k], f"bake_triangles, front: {k}")
    for k in ("light", "open"):
        assert_bits_equal(got[k][40:], back[k], f"bake_triangles, back with pixel0 advanced: {k}")


# ---------------------------------------------------------------- shapes, batches and keys
SHAPES = [(1, 1, 4), (1, 65536, 1), (85, 3, 4), (255, 1, 4), (257, 1, 4), (64, 5, 4), (341, 3, 4)]


@pytest.mark.parametrize("M,K,depth", SHAPES)
def test_shapes_with_default_and_small_batches(canonical_pair, elements, M, K, depth):
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    pos, nrm = elements
    idx = (np.arange(M) * 7) % pos.shape[0]
    pos, nrm = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx])
    pixel0 = 4000
    exp = BR.bake_ref(orc, so, SEED, pos, nrm, K, depth, pixel0, want_light=False)
    mean = None
    # 101 is no multiple of 3 or 5: batches of 99 / 100 / 101 rays (33 / 20 / 101 elements) split the range mid-way, and a
    # batch smaller than one element's rays is rounded up to them (K = 65536)
    for tuning in (None, {"batch_paths": 101}):
        caster = R.HipRayCaster(seed=SEED, tuning=tuning)
        params = caster.bake_params("points", rays=K, maxdepth=depth, pixel0=pixel0)
        got, ctx = _device_call(caster, sp, pos, nrm, params)
        assert_bits_equal(exp.orig, got["orig"], f"orig, tuning {tuning}")
        assert_bits_equal(exp.dir, got["dir"], f"dir, tuning {tuning}")
        assert_bits_equal(exp.open, got["open"], f"open, tuning {tuning}")
        if mean is None:
            mean, rctx = _rays_mean(R.HipRayCaster(seed=SEED), sp, got["orig"], got["dir"], depth, K, pixel0)
            rays = rctx.total_rays
        assert_bits_equal(mean, got["light"], f"light vs rtmi_render_rays_device(mean), tuning {tuning}")
        assert ctx.total_rays == rays
        nbatch = 1 if tuning is None else -(-M // max(101 // K, 1))
        assert ctx.stats["trace_launches"] == nbatch * depth
        # the host variant stages its batches differently: the same bits
        host, _ = caster.bake(sp, pos, nrm, params, light=True, open=True, orig=True, dir=True)
        for k in host:
            assert_bits_equal(got[k], host[k], f"host variant: {k}, tuning {tuning}")


def test_pixel0_is_the_key_and_a_split_call_changes_nothing(canonical_pair, elements):
    R = _R()
    _, sp = canonical_pair
    pos, nrm = elements
    M, K, depth = 64, 5, 4
    idx = np.arange(M) % pos.shape[0]
    pos, nrm = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx])
    caster = R.HipRayCaster(seed=SEED)
    whole, _ = _device_call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=900))
    other, _ = _device_call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=901))
    for k in ("light", "open", "dir"):
        assert not np.array_equal(whole[k], other[k]), k                       # two pixel0s: other draws
    assert_bits_equal(whole["orig"], other["orig"], "the origins of points draw nothing")
    cut = 23
    a, _ = _device_call(caster, sp, pos[:cut], nrm[:cut], caster.bake_params(rays=K, maxdepth=depth, pixel0=900))
    b, _ = _device_call(caster, sp, pos[cut:], nrm[cut:], caster.bake_params(rays=K, maxdepth=depth, pixel0=900 + cut))
    for k in OUTS:
        assert_bits_equal(whole[k], np.concatenate([a[k], b[k]]), f"two calls with pixel0 advanced by hand: {k}")


# ---------------------------------------------------------------- output options
def test_every_output_alone_and_depth_zero(canonical_pair, elements):
    R = _R()
    _, sp = canonical_pair
    pos, nrm = elements
    M, K, depth = 85, 3, 4
    idx = np.arange(M) % pos.shape[0]
    pos, nrm = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx])
    for mode, p4 in (("points", pos), ("triangles", np.ascontiguousarray(np.repeat(pos, 3, axis=0) + np.tile(np.eye(4, dtype=F32)[:3] * F32(0.01), (M, 1))))):
        caster = R.HipRayCaster(seed=SEED)
        params = caster.bake_params(mode, rays=K, maxdepth=depth, pixel0=3)
        full, fctx = _device_call(caster, sp, p4, nrm, params)
        for k in OUTS:
            one, ctx = _device_call(caster, sp, p4, nrm, params, want=(k,))
            assert_bits_equal(full[k], one[k], f"{mode}: {k} alone")
            # only what the output needs is traced: nothing for the rays, pass 0 for open, every pass for light
            assert ctx.stats["trace_launches"] == dict(light=depth, open=1, orig=0, dir=0)[k]
            assert ctx.total_rays == dict(light=fctx.total_rays, open=M * K, orig=0, dir=0)[k]
            host, _ = caster.bake(sp, p4, nrm, params, **{o: o == k for o in OUTS})
            assert_bits_equal(full[k], host[k], f"{mode}: {k} alone, host variant")
        # depth 0: light is zeros; the rays and open are still produced, and the rays are traced only for open
        zero = caster.bake_params(mode, rays=K, maxdepth=0, pixel0=3)
        got, ctx = _device_call(caster, sp, p4, nrm, zero)
        assert not got["light"].view(np.uint32).any()
        for k in ("open", "orig", "dir"):
            assert_bits_equal(full[k], got[k], f"{mode}: {k} at depth 0")
        assert ctx.stats["trace_launches"] == 1 and ctx.total_rays == M * K
        got, ctx = _device_call(caster, sp, p4, nrm, zero, want=("light", "orig", "dir"))
        assert not got["light"].view(np.uint32).any()
        assert_bits_equal(full["orig"], got["orig"], f"{mode}: orig at depth 0 without open")
        assert ctx.stats["trace_launches"] == 0 and ctx.total_rays == 0
        got, ctx = _device_call(caster, sp, p4, nrm, zero, want=("light",))
        assert not got["light"].view(np.uint32).any() and ctx.total_rays == 0
        host, hctx = caster.bake(sp, p4, nrm, zero, light=True, open=True, orig=True, dir=True)
        assert not host["light"].view(np.uint32).any() and hctx.total_rays == M * K
        for k in ("open", "orig", "dir"):
            assert_bits_equal(full[k], host[k], f"{mode}: {k} at depth 0, host variant")


# ---------------------------------------------------------------- scene kinds
def _kind_case(pair, options=0, oracle_open=True):
    orc, R = _orc(), _R()
    so, sp = pair
    o4, d4 = orc.primary_rays(16, 16, orc.canonical_viewport(16, 16), 1)
    caster = R.HipRayCaster(seed=SEED, options=options)
    tri, t, face, _ = caster.trace(sp, o4, d4)
    hit = np.nonzero(tri != 0)[0][:60]
    assert len(hit) >= 20
    pos = ((d4[hit] * t[hit, None]).astype(F32) + o4[hit]).astype(F32)
    nrm = (d4[hit] * F32(-1.0)).astype(F32)  # towards the camera: a side to bake on any kind of surface, spheres included
    K, depth, pixel0 = 4, 4, 50
    got, ctx = _device_call(caster, sp, pos, nrm, caster.bake_params(rays=K, maxdepth=depth, pixel0=pixel0))
    exp = BR.rays(orc, SEED, pos, nrm, K, pixel0)
    assert_bits_equal(exp.orig, got["orig"], "orig vs bake_ref")
    assert_bits_equal(exp.dir, got["dir"], "dir vs bake_ref")
    mean, rctx = _rays_mean(caster, sp, got["orig"], got["dir"], depth, K, pixel0)
    assert_bits_equal(mean, got["light"], "light vs the handle's own rtmi_render_rays_device on the dumped rays")
    assert_bits_equal(_own_open(caster, sp, got["orig"], got["dir"], K), got["open"], "open vs the handle's own rtmi_trace")
    assert ctx.total_rays == rctx.total_rays
    assert 0 < (got["open"] < 1).sum() and len(np.unique(got["light"], axis=0)) >= 5
    if oracle_open:
        full = BR.bake_ref(orc, so, SEED, pos, nrm, K, depth, pixel0)
        assert_bits_equal(full.open, got["open"], "open vs the oracle")
        assert_bits_equal(full.light, got["light"], "light vs the oracle")
    return got


def test_scene_kind_linear_list():
    _kind_case(build_pair(recipe_canonical(accel="trivial")))


def test_scene_kind_generic_tree(canonical_pair):
    _kind_case(canonical_pair, _R().OPT_GENERIC)


def test_scene_kind_analytic_spheres():
    _kind_case(build_pair(recipe_circles_analytic()), oracle_open=False)


@pytest.mark.parametrize("option", ["OPT_BVH", "OPT_FAST"])
def test_scene_kind_bvh_and_fast_equal_their_own_render_rays(canonical_pair, option):
    _kind_case(canonical_pair, getattr(_R(), option), oracle_open=False)


# ---------------------------------------------------------------- refusals: nothing is launched, nothing is written
def test_every_refusal_leaves_the_outputs_untouched():
    import torch
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    M, K = 12, 4
    bufs = dict(pos=torch.full((3 * M, 4), 2.5, device="cuda"), nrm=torch.full((M, 4), 2.5, device="cuda"),
                light=torch.full((M, 4), -7.0, device="cuda"), open=torch.full((M,), -7.0, device="cuda"),
                orig=torch.full((M * K, 4), -7.0, device="cuda"), dir=torch.full((M * K, 4), -7.0, device="cuda"))
    torch.cuda.synchronize()
    # the list's stand-in addresses become the real buffers (its far-apart ones, for counts no buffer could hold, stay)
    real = {TB.POS: bufs["pos"].data_ptr(), TB.NRM: bufs["nrm"].data_ptr(), TB.LIGHT: bufs["light"].data_ptr(),
            TB.OPEN: bufs["open"].data_ptr(), TB.ORIG: bufs["orig"].data_ptr(), TB.DIR: bufs["dir"].data_ptr()}
    sub = lambda p: real.get(p, p)
    for code, word, kw in TB.REFUSALS:
        args = dict(pos=TB.POS, nrm=TB.NRM, out=(TB.LIGHT, TB.OPEN, TB.ORIG, TB.DIR))
        args.update(kw)
        args["pos"], args["nrm"] = sub(args["pos"]), sub(args["nrm"])
        if args["out"] is not None:
            args["out"] = tuple(sub(p) for p in args["out"])
        for rc, msg, rays in TB.call_both(**args):
            assert rc == code and word in msg and rays == 0, (kw, rc, msg)
            assert L.rtmi_last_error() == msg
    torch.cuda.synchronize()
    for k in OUTS:
        assert (bufs[k] == -7.0).all().item(), k
    assert (bufs["pos"] == 2.5).all().item() and (bufs["nrm"] == 2.5).all().item()


def test_python_refusals_reach_no_kernel(canonical_pair, elements):
    import torch
    R = _R()
    _, sp = canonical_pair
    pos, nrm = elements
    caster = R.HipRayCaster(seed=SEED)
    light = torch.full((8, 4), -7.0, device="cuda")
    tp, tn = _dev(pos[:8]), _dev(nrm[:8])
    with pytest.raises(ValueError):
        caster.bake_device(sp, tp, tn, caster.bake_params(rays=4), light=light, open=light)          # wrong size
    with pytest.raises(ValueError):
        caster.bake_device(sp, tp, tn, caster.bake_params(rays=4), light=tp)                          # an output over an input
    bad = caster.bake_params(rays=4)
    bad.flags = 1                                                                                     # past Python's checks: the library refuses
    with pytest.raises(RuntimeError, match="flags"):
        caster.bake_device(sp, tp, tn, bad, light=light)
    with pytest.raises(RuntimeError, match="flags"):
        caster.bake(sp, pos[:8], nrm[:8], bad)
    torch.cuda.synchronize()
    assert (light == -7.0).all().item()
    got, _ = _device_call(caster, sp, pos[:8], nrm[:8], caster.bake_params(rays=4), want=("light",))   # the handle stays usable
    assert np.isfinite(got["light"]).all() and (got["light"] != -7.0).all()


# ---------------------------------------------------------------- streams and the shared workspace
def test_points_made_on_a_torch_stream_just_before_the_call(canonical_pair):
    import torch
    R = _R()
    so, sp = canonical_pair
    a, A = BR.ANCHOR, TB.anchor(so)
    M = A["pos"].shape[0]
    src_p, src_n = _dev(A["pos"] * F32(0.5)), _dev(A["nrm"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    light, open_ = torch.full((M, 4), -7.0, device="cuda"), torch.full((M,), -7.0, device="cuda")
    caster = R.HipRayCaster(seed=a["seed"])
    with torch.cuda.stream(stream):
        big = torch.ones(1 << 24, device="cuda")
        for _ in range(8):  # work in front of the points on that stream
            big = big * 1.0001
        tp = src_p * 2.0  # exact: the points again
        tn = src_n.clone()
        ctx = caster.bake_device(sp, tp, tn, caster.bake_params(rays=a["K"], maxdepth=a["maxdepth"], pixel0=a["pixel0"]), light=light, open=open_,
                                 stream=stream)
        out_l, out_o = light.clone(), open_.clone()  # ordered behind the call on the same stream
    stream.synchronize()
    assert_bits_equal(A["full"].light, out_l.cpu().numpy(), "light of points produced on the stream")
    assert_bits_equal(A["full"].open, out_o.cpu().numpy(), "open of points produced on the stream")
    assert ctx.total_rays == A["full"].rays


def test_an_ordinary_frame_stays_exact_after_a_bake(canonical_pair):
    orc, R = _orc(), _R()
    so, sp = canonical_pair
    a, A = BR.ANCHOR, TB.anchor(so)
    w, h, spp = 40, 28, 3
    ref, cn = so.render(w, h, orc.canonical_viewport(w, h), 5, spp, seed=9, threads=8)
    caster = R.HipRayCaster(seed=a["seed"])
    vp = R.canonical_viewport(w, h, 5, spp)
    for pipeline in (0, 1):
        frame = R.HipRayCaster(seed=9, tuning={"pipeline": pipeline})
        before = np.zeros((h, w, 4), np.float32)
        frame.walk_rays(vp, sp, before, 1, False)
        got, _ = _device_call(caster, sp, A["pos"], A["nrm"], caster.bake_params(rays=a["K"], maxdepth=a["maxdepth"], pixel0=a["pixel0"]))
        host, _ = caster.bake(sp, A["pos"], A["nrm"], caster.bake_params(rays=a["K"], maxdepth=a["maxdepth"], pixel0=a["pixel0"]))
        after = np.zeros((h, w, 4), np.float32)
        ctx = frame.walk_rays(vp, sp, after, 1, False)
        assert_bits_equal(ref, before, f"before, pipeline {pipeline}")
        assert_bits_equal(ref, after, f"after, pipeline {pipeline}")
        assert_bits_equal(A["full"].light, got["light"], "the bake in between")
        assert_bits_equal(A["full"].light, host["light"], "the host bake in between")
        assert ctx.total_rays == cn["rays"]


# ---------------------------------------------------------------- the draws on the device against the float64 referee
def test_open_at_the_probes_floor_points_against_the_referee():
    R = _R()
    case = TB.open_case()
    print()
    for accel in ("octree", "list"):
        sp = TB.open_recipe(accel)(ProductApi(R))
        for seed in TB.D.SEEDS:
            caster = R.HipRayCaster(seed=seed)
            got, ctx = _device_call(caster, sp, case["pos"], case["nrm"], caster.bake_params(rays=TB.OPEN_K, maxdepth=0, bias=TB.OPEN_BIAS), want=("open",))
            assert ctx.total_rays == case["pos"].shape[0] * TB.OPEN_K
            TB.check_open(got["open"], f"rtmi_bake_device {accel} seed {seed}")
