"""-m gpu: every sampling mode on every shading level, each mode held with an argument that can tell a position from a pixel.
launch_shade (rtmi_device.hip) picks one of 30 kernels, k_shade{,_samples,_list,_views,_rays}{,_glass,_env,_smooth,_tex,_nmap}, and
appends the mode's own argument and the level's tables.  tests/test_sampling_matrix.py holds the modes to the trace variants at level
PLAIN; the level files hold every level to every mode with the most benign argument of each mode.  Here the argument is real.

Every expected float comes from tests/nmap_ref.py on the oracle (tests/shade_level_cases.py; tests/test_shade_level_matrix_cpu.py
shows that no cell passes vacuously), and every comparison is bit for bit.  W = H = 32, S = 8, M = P = 2, depth 5, seed 5.

Row     scene                                        LIST                        PASS               VIEWS              RAYS
glass   the glass slab                               each row, each cell:        [0,1) [1,3) [3,8)  three cameras,     the frame's rays
env     canonical + sky                              a count map with 2, 4, 6    from a NaN accum,  three seeds, spp   permuted, keyed;
smooth  canonical + generated normals                and 8, refinement lists     full tile and      4; one batch with  whole and in
tex     canonical + normals + sky + texture          of 70 to 357 pixels in 46   striped tile,      two view borders,  batches of 500;
nmap    tex + the height-field normal map            to 165 runs; host and       default tuning     and batches of     un-keyed in groups
all     the normal-map patch + normals + sky         device variant; full and    and four streams   147 pixels that    of 4 with means
        (glass, mirror, matte, solid, mapped and     striped tile on a caller's  with batches of    straddle them, on  and guides
        unmapped triangles)                          stream; 4 streams x 5-pixel 10 paths           one and on three
                                                     batches; 1 stream x 250                        streams
The adaptive denoised wrapper runs on tex, nmap and all with the same count maps.  The last test walks the levels over one device
scene and one caster, so that the workspace's colour stack is allocated, left unused, reused and regrown."""
import numpy as np
import pytest

from conftest import assert_bits_equal
import shade_level_cases as K

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, S, M, P, SEED = K.W, K.H, K.S, K.M, K.P, K.SEED
FULL = (0, H, H, 0)
GUARD = 64  # floats (or counts) before and after every device buffer: a tile's call writes nothing outside its rows
BATCH_600_STREAMS = {"streams": 3, "batch_paths": K.VIEW_BATCH, "subtile_min_paths": 1}


def _R():
    from rust_raytrace_amd import raytrace as R
    return R


_SCENES = {}


@pytest.fixture(scope="module", params=K.ROWS)
def case(request):
    """(row name, product scene): one device scene per row, shared by the row's tests"""
    return request.param, _scene(request.param)


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = K.product(name)
    return _SCENES[name]


@pytest.fixture(scope="module", autouse=True)
def _release_scenes():
    yield
    _SCENES.clear()


def _caster(tuning=None):
    return _R().HipRayCaster(seed=SEED, tuning=tuning)


def _list_device(c, sp, tile, on_stream):
    """walk_adaptive_device on guarded torch buffers, accum / sumsq / out NaN and counts 0 before: dict of host arrays and ctx"""
    import torch
    dev = torch.device("cuda", 0)
    nrows = tile[1]
    n = nrows * W
    bufs = {k: torch.full((n * 4 + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev) for k in ("accum", "sumsq", "out")}
    cnt = torch.zeros((n + 2 * GUARD,), dtype=torch.int32, device=dev)
    for t in bufs.values():
        t[:GUARD] = 7.5
        t[GUARD + n * 4:] = 7.5
    cnt[:GUARD] = 77
    cnt[GUARD + n:] = 77
    stream = torch.cuda.Stream(device=dev) if on_stream else None
    torch.cuda.synchronize()
    e = K.expect("glass")  # every row's tolerance is the first of TOLS (the CPU file pins it)
    ctx = c.walk_adaptive_device(K.viewport(), sp, tile, bufs["accum"][GUARD:].data_ptr(), bufs["sumsq"][GUARD:].data_ptr(),
                                 cnt[GUARD:].data_ptr(), bufs["out"][GUARD:].data_ptr(), stream.cuda_stream if on_stream else None,
                                 M, P, *e.tol)
    if on_stream:
        stream.synchronize()
    torch.cuda.synchronize()
    got = {}
    for k, t in bufs.items():
        g = t.cpu().numpy()
        assert (g[:GUARD] == 7.5).all() and (g[GUARD + n * 4:] == 7.5).all(), f"{k}: written outside the tile's rows"
        got[k] = g[GUARD:GUARD + n * 4].reshape(nrows, W, 4)
    g = cnt.cpu().numpy()
    assert (g[:GUARD] == 77).all() and (g[GUARD + n:] == 77).all(), "counts: written outside the tile's rows"
    got["counts"] = g[GUARD:GUARD + n].reshape(nrows, W).view(np.uint32)
    return got, ctx


def _check_list(got, ctx, e, what):
    assert np.array_equal(got["counts"], e.counts), f"{what}: {int((got['counts'] != e.counts).sum())} counts differ from the replay"
    assert_bits_equal(got["accum"], e.accum, f"{what}: accum vs the replay")
    assert_bits_equal(got["sumsq"], e.sumsq, f"{what}: sumsq vs the replay")
    assert_bits_equal(got["out"], e.out, f"{what}: out vs accum * (1 / count)")
    assert (ctx.passes, int(ctx.samples), ctx.unconverged) == (e.passes, e.samples, e.unconverged)
    assert ctx.total_rays == e.rays and ctx.stats["pipeline"] == 1


def _expect(name, tile):
    return K.expect(name) if tile == FULL else K.expect_tile(name, tile)


def _list_launches(e, npix, tuning):
    """The closest-hit launches of an adaptive call: one per bounce pass of every batch of every sampling pass, by the restated plan"""
    sizes = [(npix, M)] + [(len(lst), P) for lst in e.lists]
    return K.DEPTH * sum(len(b) for n, k in sizes for b in K.plan_batches(n, k, tuning, refinement=n < npix))


# ---------------------------------------------------------------- LIST
def test_list_host_variant(case):
    name, sp = case
    e = K.expect(name)
    img = np.full((H, W, 4), np.nan, F32)
    ctx = _caster().walk_rays_adaptive(K.viewport(), sp, img, min_samples=M, pass_samples=P, rel_tol=e.tol[0], abs_tol=e.tol[1])
    assert np.array_equal(ctx.counts, e.counts), f"{int((ctx.counts != e.counts).sum())} counts differ from the replay"
    assert (ctx.passes, int(ctx.samples), ctx.unconverged) == (e.passes, e.samples, e.unconverged)
    assert_bits_equal(img, e.out, "every pixel at its own count")
    assert ctx.total_rays == e.rays and ctx.stats["pipeline"] == 1


@pytest.mark.parametrize("tile", [FULL, K.STRIPED], ids=["full", "striped"])
def test_list_device_variant(case, tile):
    name, sp = case
    got, ctx = _list_device(_caster(), sp, tile, on_stream=tile != FULL)
    e = _expect(name, tile)
    _check_list(got, ctx, e, f"{name}, tile {tile}")
    assert ctx.stats["trace_launches"] == _list_launches(e, tile[1] * W, {})


@pytest.mark.parametrize("tile", [FULL, K.STRIPED], ids=["full", "striped"])
@pytest.mark.parametrize("tuning", [K.SMALL, K.ONE_STREAM], ids=["four_streams_batch_40", "one_stream_batch_500"])
def test_list_under_two_tunings(case, tuning, tile):
    name, sp = case
    got, ctx = _list_device(_caster(tuning), sp, tile, on_stream=tile != FULL)
    e = _expect(name, tile)
    _check_list(got, ctx, e, f"{name}, tile {tile}, tuning {tuning}")
    # the tuning did cut every pass as planned
    assert ctx.stats["streams"] == tuning["streams"]
    assert ctx.stats["trace_launches"] == _list_launches(e, tile[1] * W, tuning)


# ---------------------------------------------------------------- PASS
def _passes_host(c, sp):
    accum, out, rays, accums = np.full((H, W, 4), np.nan, F32), np.full((H, W, 4), np.nan, F32), 0, []
    for i, (k0, n) in enumerate(K.PASSES):
        ctx = c.walk_samples(K.viewport(), sp, 0, H, k0, n, accum, out if i == len(K.PASSES) - 1 else None)
        assert ctx.stats["pipeline"] == 1
        rays += ctx.total_rays
        accums.append(accum.copy())
    return accums, out, rays


def _passes_device(c, sp, tile):
    import torch
    n = tile[1] * W * 4
    accum, out = (torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(2))
    for t in (accum, out):
        t[:GUARD] = 7.5
        t[GUARD + n:] = 7.5
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    rays, accums = 0, []
    for i, (k0, ns) in enumerate(K.PASSES):
        last = i == len(K.PASSES) - 1
        ctx = c.walk_samples_device(K.viewport(), sp, tile, k0, ns, accum[GUARD:].data_ptr(), out[GUARD:].data_ptr() if last else None,
                                    stream.cuda_stream)
        stream.synchronize()
        assert ctx.stats["pipeline"] == 1
        rays += ctx.total_rays
        accums.append(accum.cpu().numpy()[GUARD:GUARD + n].reshape(tile[1], W, 4))
    for t in (accum, out):
        g = t.cpu().numpy()
        assert (g[:GUARD] == 7.5).all() and (g[GUARD + n:] == 7.5).all(), "written outside the tile's rows"
    return accums, out.cpu().numpy()[GUARD:GUARD + n].reshape(tile[1], W, 4), rays


@pytest.mark.parametrize("tile", [None, K.STRIPED], ids=["full", "striped"])
@pytest.mark.parametrize("tuning", [None, K.SMALL], ids=["default", "four_streams_batch_40"])
def test_uneven_passes(case, tuning, tile):
    name, sp = case
    refs = K.pass_refs(name, tile)
    accums, out, rays = _passes_host(_caster(tuning), sp) if tile is None else _passes_device(_caster(tuning), sp, tile)
    for (k0, n), got, ref in zip(K.PASSES, accums, refs):
        assert_bits_equal(got, ref.accum, f"{name}: accum after samples [{k0}, {k0 + n})")
    assert_bits_equal(out, refs[-1].image, f"{name}: out of the last pass")
    assert rays == sum(r.rays for r in refs)


# ---------------------------------------------------------------- VIEWS
@pytest.mark.parametrize("tuning", [None, {"batch_paths": K.VIEW_BATCH}, BATCH_600_STREAMS], ids=["default", "batch_600", "batch_600_three_streams"])
def test_three_views_three_seeds(case, tuning):
    name, sp = case
    refs = K.view_refs(name)
    vps = [K.viewport(K.VIEW_SPP, v) for v in K.views()]
    ctx = _caster(tuning).walk_rays_views(vps, sp, seeds=[SEED + k for k in range(3)])
    for k, ref in enumerate(refs):
        assert_bits_equal(ctx.data[k], ref.image, f"{name}: view {k}")
    assert ctx.total_rays == sum(r.rays for r in refs) and ctx.stats["pipeline"] == 1
    # the tuning did cut the stacked image as planned
    assert ctx.stats["trace_launches"] == K.DEPTH * sum(len(b) for b in K.plan_batches(3 * W * H, K.VIEW_SPP, tuning or {}, nrows=3 * H))


# ---------------------------------------------------------------- RAYS
@pytest.mark.parametrize("tuning", [None, {"batch_paths": K.RAYS_BATCH}], ids=["default", "batch_500"])
def test_permuted_rays_with_their_keys(case, tuning):
    name, sp = case
    c = K.rays_case(name)
    got, ctx = _caster(tuning).walk_rays_explicit(sp, c.o4, c.d4, K.DEPTH, keys=c.keys)
    assert_bits_equal(got["color"], c.color, f"{name}: the restatement's rows in the permuted order")
    assert ctx.total_rays == c.rays and ctx.stats["pipeline"] == 1


def test_unkeyed_rays_in_groups(case):
    name, sp = case
    c = K.rays_case(name)
    got, ctx = _caster({"batch_paths": K.RAYS_BATCH}).walk_rays_explicit(sp, c.o4, c.d4, K.DEPTH, group=K.G, color=True, mean=True, albedo=True,
                                                                        normal=True, ids=True)
    assert_bits_equal(got["color"], c.group_color, f"{name}: pixel = group, sample = place in group")
    assert_bits_equal(got["mean"], c.mean, f"{name}: group means")
    assert_bits_equal(got["albedo"], c.albedo, f"{name}: the albedo guide")
    assert_bits_equal(got["normal"], c.normal, f"{name}: the normal guide")
    assert np.array_equal(got["ids"], c.ids)
    assert ctx.total_rays == c.group_rays and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- the adaptive denoised wrapper
@pytest.mark.parametrize("name", K.WRAPPED)
def test_adaptive_denoised_wrapper_with_a_real_count_map(name):
    sp = _scene(name)
    e, wi = K.expect(name), K.wrapper_inputs(name)
    c = _caster()
    want = c.denoise_var(wi.color, wi.albedo, wi.normal, wi.var, scene=sp)
    got = np.full((H, W, 4), np.nan, F32)
    ctx = c.walk_rays_adaptive_denoised(K.viewport(), sp, got, min_samples=M, pass_samples=P, rel_tol=e.tol[0], abs_tol=e.tol[1])
    assert np.array_equal(ctx.counts, e.counts)
    assert_bits_equal(got, want, f"{name}: rtmi_render_adaptive_denoised = denoise_var of the restatement's colour, guides and variance")
    assert (ctx.passes, int(ctx.samples), ctx.unconverged) == (e.passes, e.samples, e.unconverged) and ctx.stats["pipeline"] == 1


# ---------------------------------------------------------------- one caster, one device scene, the levels in turn
def test_levels_in_turn_on_one_workspace():
    """A workspace belongs to a device scene, and a caster keeps the device scene of a Scene while its geometry stays: the canonical
    Scene is dressed as nmap (striped tile: the colour stack is allocated), plain (full tile: the workspace grows, the stack is not
    touched), tex (full tile: the stack is regrown and reused), then env and smooth; glass and all follow on their own scenes under
    the same caster.  Each LIST result is the replay's."""
    c = _caster()
    sp = K.product("nmap")
    steps = [("nmap", K.STRIPED), ("plain", FULL), ("tex", FULL), ("glass", FULL), ("all", FULL), ("env", K.STRIPED), ("smooth", FULL)]
    for name, tile in steps:
        if name in ("glass", "all"):
            scene = K.product(name)
        else:
            scene = K.dress(K.dress(sp, "plain"), name)
        got, ctx = _list_device(c, scene, tile, on_stream=False)
        e = _expect(name, tile)
        assert e.tol == K.expect("glass").tol
        _check_list(got, ctx, e, f"step {name}, tile {tile}") if name != "plain" else _check_plain(got, ctx, e)


def _check_plain(got, ctx, e):
    """The plain canonical scene runs the path kernels (pipeline 3); everything else as _check_list"""
    assert np.array_equal(got["counts"], e.counts)
    for k in ("accum", "sumsq", "out"):
        assert_bits_equal(got[k], getattr(e, k), f"step plain: {k}")
    assert (ctx.passes, int(ctx.samples), ctx.unconverged, ctx.total_rays) == (e.passes, e.samples, e.unconverged, e.rays)
    assert ctx.stats["pipeline"] == 3
