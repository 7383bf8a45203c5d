"""No GPU: box lights on explicit rays and in the bake (rtmi_render_rays_lit*, rtmi_bake_lit*; include/rtmi.h defines them).  The
entry points exist and are declared, they refuse bad arguments before any HIP call and before the scene is used, and the
restatement the GPU tests compare with (tests/bake_lit_ref.py) is sound: without lights it is bake_ref's, its RNG blocks are
pairwise distinct, `direct` is held by a float64 referee on one Matte wall (a point light exactly, a box light in expectation), the
texel formula agrees with the lit render of the same points, and the conditions the GPU cases rely on hold."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
from conftest import ROOT
import bake_lit_ref as BL
import bake_ref as BR
import draw_ref as DR
import lit_ref as LT
import shadowed_ref as SR
import test_bake_cpu as TB

F32 = np.float32
RTMI_OK, RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED = 0, 1, 3
NAMES = ("rtmi_render_rays_lit", "rtmi_render_rays_lit_device", "rtmi_bake_lit", "rtmi_bake_lit_device", "rth_caster_walk_rays_explicit_lit",
         "rth_caster_walk_rays_explicit_lit_device", "rth_caster_bake_lit", "rth_caster_bake_lit_device")
BOGUS = TB.BOGUS
DIRECT = 0x1000000 * 7  # beside test_bake_cpu's stand-in addresses: never touched
R_ORIG, R_DIR, R_KEYS, R_COLOR, R_MEAN = (0x100000 * k for k in range(1, 6))
POINTS = TB.POINTS
DARK = SimpleNamespace(table=np.zeros((4, 4, 3), F32), frame=None)  # an all-zero environment: a path that escapes brings nothing
WALL_LIGHT = (3.0, 1.0, 2.0)        # in front of the wall (z ~ 6), off the camera's axis (tests/test_lit_cpu.py's)
WALL_COLOR = (0.9, 0.7, 0.5)
WALL_COLOR_SQ = (27.0, 21.0, 15.0)  # ... with RTMI_LIT_INVERSE_SQUARE: d2 is 16 to 60 on this wall
# test_a_point_light_at_wall_points_is_the_float64_formula: the largest relative deviation measured there, times 4
REL_F32 = 4 * 2.9e-7


def _orc():
    from oracle import orc
    return orc


def _lib():
    from rust_raytrace_amd import _ffi
    return _ffi, _ffi.lib()


def _lit(nlights=2, lit_flags=0, index=1, orig=None, color=None, **fields):
    """rtmi_lit_t from the defaults with `nlights` lights; `fields`, orig and color go to light `index`"""
    ffi, L = _lib()
    a = ffi.Lit()
    L.rtmi_lit_defaults(C.byref(a))
    a.nlights, a.flags = nlights, lit_flags
    for k, x in fields.items():
        setattr(a.lights[index], k, x)
    if orig is not None:
        a.lights[index].orig[0], a.lights[index].orig[1], a.lights[index].orig[2] = orig
    if color is not None:
        a.light_color[index][0], a.light_color[index][1], a.light_color[index][2] = color
    return a


# ---------------------------------------------------------------- the ABI
def bake_both(M=12, pos=TB.POS, nrm=TB.NRM, scene=BOGUS, bake=(POINTS, 4, 4, 0, 0, 0.001), out=(TB.LIGHT, TB.OPEN, TB.ORIG, TB.DIR, DIRECT),
              lit="dflt"):
    """(rc, message, stats.rays) of rtmi_bake_lit_device and rtmi_bake_lit for the same arguments; bake / out / lit None: NULL"""
    ffi, L = _lib()
    b = C.byref(ffi.Bake(*bake)) if bake is not None else None
    o = C.byref(ffi.BakeLitOut(*[p or None for p in out])) if out is not None else None
    a = _lit() if isinstance(lit, str) else lit
    e = C.byref(a) if a is not None else None
    ptr = lambda p: C.c_void_p(p) if p else None
    res = []
    for dev in (True, False):
        st = ffi.Stats()
        st.rays = 123
        if dev:
            rc = L.rtmi_bake_lit_device(scene, M, ptr(pos), ptr(nrm), 7, b, e, o, None, C.byref(st))
        else:
            rc = L.rtmi_bake_lit(scene, M, ptr(pos), ptr(nrm), 7, b, e, o, C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


def rays_both(n=48, orig=R_ORIG, dirs=R_DIR, keys=R_KEYS, scene=BOGUS, rays=(5, 4, 0, 0), out=(R_COLOR, R_MEAN, 0, 0, 0), lit="dflt"):
    """The same for rtmi_render_rays_lit_device and rtmi_render_rays_lit (no guide buffers: their check reads the scene)"""
    ffi, L = _lib()
    r = C.byref(ffi.Rays(*rays)) if rays is not None else None
    o = C.byref(ffi.RaysOut(*[p or None for p in out])) if out is not None else None
    a = _lit() if isinstance(lit, str) else lit
    e = C.byref(a) if a is not None else None
    ptr = lambda p: C.c_void_p(p) if p else None
    res = []
    for dev in (True, False):
        st = ffi.Stats()
        st.rays = 123
        if dev:
            rc = L.rtmi_render_rays_lit_device(scene, n, ptr(orig), ptr(dirs), ptr(keys), 7, r, e, o, None, C.byref(st))
        else:
            rc = L.rtmi_render_rays_lit(scene, n, ptr(orig), ptr(dirs), ptr(keys), 7, r, e, o, C.byref(st))
        res.append((rc, L.rtmi_last_error(), st.rays))
    return res


nan, inf = float("nan"), float("inf")
# rtmi_render_lit*'s checks of its parameters, which both calls make after their own: (a word of the message, rtmi_lit_t)
LIT_REFUSALS = [(b"rtmi_lit_t", None)] + [(b"nlights", _n) for _n in (5, 1 << 31)] + [(b"lit: unknown flags", _f) for _f in (2, 1 << 31)] + [
    (b"light 1", dict(rays=0)), (b"light 1", dict(rays=257)), (b"rays must be 1", dict(rays=2)), (b"light 1", dict(flags=2)),
    (b"len2", dict(len2=nan)), (b"len2", dict(len2=-1.0)), (b"len2", dict(len2=inf)), (b"bias", dict(bias=nan)), (b"bias", dict(bias=-inf)),
    (b"orig", dict(orig=(nan, 0.0, 0.0))), (b"orig", dict(orig=(0.0, 0.0, -inf))), (b"light_color", dict(color=(1.0, inf, 1.0))),
    (b"light 3", dict(nlights=4, index=3, len2=nan))]


def _lit_cases():
    for word, spec in LIT_REFUSALS:
        if isinstance(spec, int):
            yield word, (_lit(nlights=spec) if word == b"nlights" else _lit(lit_flags=spec))
        else:
            yield word, (None if spec is None else _lit(**spec))


# every refusal of rtmi_bake_lit*: rtmi_bake*'s list with the fifth output, direct among the overlaps, then the lit parameters.
# tests/test_bake_lit.py sends the same lists with real, pre-filled device buffers.
def _five(kw):
    kw = dict(kw)
    if kw.get("out") is not None and len(kw["out"]) == 4:
        kw["out"] = tuple(kw["out"]) + ((0,) if not any(kw["out"]) else (kw["out"][3] + (1 << 40) if kw["out"][3] >= TB.BIG else DIRECT,))
    return kw


BAKE_REFUSALS = [(code, word, _five(kw)) for code, word, kw in TB.REFUSALS] + [
    (RTMI_ERR_INVALID, b"all five outputs", dict(out=(0, 0, 0, 0, 0))),
    (RTMI_ERR_INVALID, b"light and direct", dict(out=(TB.LIGHT, TB.OPEN, TB.ORIG, TB.DIR, TB.LIGHT + 16 * 12 - 1))),
    (RTMI_ERR_INVALID, b"nrm4 and direct", dict(out=(0, 0, 0, 0, TB.NRM))),
] + [(RTMI_ERR_INVALID, word, dict(lit=lit)) for word, lit in _lit_cases() if lit is not None] + [(RTMI_ERR_INVALID, b"rtmi_lit_t", dict(lit=None))]
RAYS_REFUSALS = [
    (RTMI_ERR_INVALID, b"scene", dict(scene=None)),
    (RTMI_ERR_INVALID, b"(rays)", dict(rays=None)),
    (RTMI_ERR_INVALID, b"(out)", dict(out=None)),
    (RTMI_ERR_INVALID, b"group", dict(rays=(5, 0, 0, 0))),
    (RTMI_ERR_INVALID, b"multiple", dict(rays=(5, 5, 0, 0), n=48)),
    (RTMI_ERR_INVALID, b"flag", dict(rays=(5, 4, 0, 2))),
    (RTMI_ERR_INVALID, b"(orig4)", dict(orig=0)),
    (RTMI_ERR_INVALID, b"(dir4)", dict(dirs=0)),
    (RTMI_ERR_INVALID, b"outputs", dict(out=(0, 0, 0, 0, 0))),
    (RTMI_ERR_INVALID, b"overlap", dict(out=(R_COLOR, R_COLOR, 0, 0, 0))),
    (RTMI_ERR_INVALID, b"pixel0", dict(keys=0, rays=(5, 4, 0xFFFFFFFF - 1, 0))),
    (RTMI_ERR_UNSUPPORTED, b"maxdepth", dict(rays=(33, 4, 0, 0))),
] + [(RTMI_ERR_INVALID, word, dict(lit=lit)) for word, lit in _lit_cases() if lit is not None] + [(RTMI_ERR_INVALID, b"rtmi_lit_t", dict(lit=None))]


def test_entry_points_are_exported_declared_and_listed():
    ffi, L = _lib()
    text = open(os.path.join(ROOT, "include", "rtmi.h")).read() + open(os.path.join(ROOT, "include", "rtmi_host.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ffi.RTMI_SYMBOLS + ffi.RTH_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert C.sizeof(ffi.BakeLitOut) == 5 * C.sizeof(C.c_void_p) and ffi.BakeLitOut.direct.offset == C.sizeof(ffi.BakeOut)
    for f in ("light", "open", "orig", "dir"):
        assert getattr(ffi.BakeLitOut, f).offset == getattr(ffi.BakeOut, f).offset
    assert re.search(r"\}\s*rtmi_bake_lit_out_t;", text) and "0xC000FFFF" in text
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES[:4]:
        assert re.search(r"pub fn " + name + r"\(", doc), name
    from rust_raytrace_amd import raytrace as R
    for m in ("walk_rays_explicit_lit", "walk_rays_explicit_lit_device", "bake_lit", "bake_lit_device", "bake_triangles_lit"):
        assert callable(getattr(R.HipRayCaster, m)), m


@pytest.mark.parametrize("k", range(len(BAKE_REFUSALS)))
def test_every_bake_refusal_returns_its_code_and_clears_the_stats(k):
    code, word, kw = BAKE_REFUSALS[k]
    for rc, msg, rays in bake_both(**kw):
        assert rc == code and word in msg and rays == 0, (kw, rc, msg)


@pytest.mark.parametrize("k", range(len(RAYS_REFUSALS)))
def test_every_rays_refusal_returns_its_code_and_clears_the_stats(k):
    code, word, kw = RAYS_REFUSALS[k]
    for rc, msg, rays in rays_both(**kw):
        assert rc == code and word in msg and rays == 0, (kw, rc, msg)


def test_the_order_of_the_checks_and_the_empty_call():
    bad = _lit(nlights=5)
    # the call's own checks come before the lit parameters ...
    for rc, msg, _ in bake_both(bake=(POINTS, 4, 4, 0, 1, 0.001), lit=bad):
        assert rc == RTMI_ERR_INVALID and b"flags must be 0" in msg
    for rc, msg, _ in bake_both(bake=(POINTS, 4, 33, 0, 0, 0.001), lit=bad):
        assert rc == RTMI_ERR_UNSUPPORTED and b"maxdepth" in msg
    for rc, msg, _ in rays_both(rays=(33, 4, 0, 0), lit=None):
        assert rc == RTMI_ERR_UNSUPPORTED and b"maxdepth" in msg
    # ... and an empty call returns where the plain call returns: nothing is touched
    for kw in (dict(), dict(lit=None), dict(pos=0, nrm=0, out=(0, 0, 0, 0, 0))):
        for rc, _, rays in bake_both(M=0, **kw):
            assert rc == RTMI_OK and rays == 0, kw
    for kw in (dict(), dict(lit=None), dict(orig=0, dirs=0, out=(0, 0, 0, 0, 0))):
        for rc, _, rays in rays_both(n=0, **kw):
            assert rc == RTMI_OK and rays == 0, kw
    # direct alone is an output; an unused light is not looked at: the next check that fails is reached
    for rc, msg, _ in bake_both(out=(0, 0, 0, 0, DIRECT), bake=(POINTS, 4, 33, 0, 0, 0.001), lit=_lit(index=2, len2=nan)):
        assert rc == RTMI_ERR_UNSUPPORTED and b"maxdepth" in msg
    # direct next to light, not overlapping it
    for rc, msg, _ in bake_both(out=(TB.LIGHT, 0, 0, 0, TB.LIGHT + 16 * 12), bake=(POINTS, 4, 33, 0, 0, 0.001)):
        assert rc == RTMI_ERR_UNSUPPORTED and b"maxdepth" in msg


# ---------------------------------------------------------------- the restatement's footing
@pytest.fixture(scope="module")
def teapot():
    return CT.recipe_canonical()(CT.OracleApi(_orc()))


def test_without_lights_the_restatement_is_bake_refs(teapot):
    orc = _orc()
    pos, nrm = BL.elements(orc, teapot)
    for mode, p4, n4 in (("points", pos, nrm), ("triangles",) + BR.scene_triangles(teapot, 1, 12)):
        got = BL.bake_lit_ref(orc, teapot, BL.SEED, p4, n4, 3, 4, (), pixel0=BL.PIXEL0, mode=mode)
        want = BR.bake_ref(orc, teapot, BL.SEED, p4, n4, 3, 4, BL.PIXEL0, mode=mode)
        for k in ("orig", "dir", "open", "light"):
            CT.assert_bits_equal(getattr(want, k), getattr(got, k), f"{mode}, nlights = 0: {k}")
        assert got.rays == want.rays and not got.direct.view(np.uint32).any() and got.direct.shape == want.light.shape


def test_the_blocks_drawn_under_one_key_are_pairwise_distinct():
    b = BL.blocks()
    every = [x for v in b.values() for x in v]
    assert len(every) == len(set(every)) == 2 + 32 + 4 * 32 + 4
    assert all(x & 0xFFFF == 0xFFFF for x in b["element"]) and max(x & 0xFFFF for x in b["level"]) == 31
    assert b["element"] == [0xC000FFFF | l << 16 for l in range(4)]


# ---------------------------------------------------------------- the float64 referee on a wall
def _wall_elements(wall, w, h):
    """First hits of the wall's view: (pos4, nrm4 (the wall's unit normal, turned towards the camera), float64 point and normal)"""
    orc = _orc()
    pos, nrm = BR.first_hit_points(orc, wall, w, h)
    n64 = nrm[:, :3].astype(np.float64)
    assert np.abs((n64 * n64).sum(1) - 1).max() < 1e-6  # a unit normal, as the header asks for
    return pos, nrm, pos[:, :3].astype(np.float64), n64


def _g64(p, n, at, inverse_square):
    v = at - p
    d2 = (v * v).sum(-1)
    c = (n * v).sum(-1) / np.sqrt(d2)
    assert (c > 0).all()
    return c / d2 if inverse_square else c


@pytest.mark.parametrize("inverse_square", [False, True], ids=["cosine", "inverse square"])
def test_a_point_light_at_wall_points_is_the_float64_formula(inverse_square):
    """direct[m] = light_color * g with g in float64 at the element (the float32 inputs taken exactly).  A point light draws nothing
    that matters (the bias only moves the shadow ray's origin), so every d_k is the same and the fold of K = 4 is exact.  Measured:
    the largest relative deviation over 242 elements and three channels is 2.4e-7 (g = c) and 2.9e-7 (g = c / d2); asserted at four
    times the larger, REL_F32 = 1.16e-6."""
    orc = _orc()
    wall = SR.recipe_wall()(CT.OracleApi(orc))
    pos, nrm, p, n = _wall_elements(wall, 16, 16)
    li = LT.light(WALL_LIGHT, 0.0, WALL_COLOR_SQ if inverse_square else WALL_COLOR)
    r = BL.bake_lit_ref(orc, wall, 5, pos, nrm, 4, 0, [li], inverse_square, want_light=False, want_open=False)
    assert len(pos) > 200 and r.el.culled == [0] and r.el.occluded == [0] and r.el.visible == [4 * len(pos)]
    want = np.asarray(li["color"], np.float64)[None, :] * _g64(p, n, np.asarray(li["orig"], np.float64), inverse_square)[:, None]
    got = r.direct[:, :3].astype(np.float64)
    dev = float(np.abs(got / want - 1).max())
    print(f"point light, inverse_square={inverse_square}: largest relative deviation {dev:.3e} over {len(pos)} elements")
    assert dev <= REL_F32 and not r.direct[:, 3].any()


def test_a_box_light_at_wall_points_is_the_box_integral_in_expectation():
    """K = 256 candidates per element of a box light of edge 0.5: the mean has the expectation color_l E[g] and the variance
    color_l^2 Var[g] / K, both from a Gauss-Legendre rule of 8^3 points over the box in float64.  Two-sided at draw_ref's
    false-alarm probability over all elements, channels and both flags, plus REL_F32 for float32's rounding."""
    orc = _orc()
    wall = SR.recipe_wall()(CT.OracleApi(orc))
    pos, nrm, p, n = _wall_elements(wall, 6, 6)
    K = 256
    for inverse_square in (False, True):
        li = LT.light(WALL_LIGHT, 0.5, WALL_COLOR_SQ if inverse_square else WALL_COLOR)
        r = BL.bake_lit_ref(orc, wall, 5, pos, nrm, K, 0, [li], inverse_square, want_light=False, want_open=False)
        assert r.el.visible == [K * len(pos)]
        x, wq = np.polynomial.legendre.leggauss(8)
        x, wq = (x + 1) / 2, wq / 2
        gx, gy, gz = np.meshgrid(x, x, x, indexing="ij")
        nodes = np.asarray(li["orig"], np.float64) + li["len2"] * np.stack([gx, gy, gz], -1).reshape(-1, 3)
        wts = (wq[:, None, None] * wq[None, :, None] * wq[None, None, :]).reshape(-1)
        g = _g64(p[:, None, :], n[:, None, :], nodes[None, :, :], inverse_square)
        eg, eg2 = g @ wts, (g * g) @ wts
        lc = np.asarray(li["color"], np.float64)
        want = lc[None, :] * eg[:, None]
        var = (eg2 - eg ** 2)[:, None] * lc[None, :] ** 2 / K
        got = r.direct[:, :3].astype(np.float64)
        bound = DR.z_quantile(DR.P_FALSE / (2 * 3 * len(pos) * 2))
        z = np.abs(got - want) / np.sqrt(var)
        print(f"box light, inverse_square={inverse_square}: largest |z| {z.max():.2f} (bound {bound:.2f}), sd / mean {(np.sqrt(var) / want).max():.2e}")
        assert (np.abs(got - want) <= bound * np.sqrt(var) + REL_F32 * want).all()
        assert (np.sqrt(var) > 4 * REL_F32 * want).all()  # the test is about the draws, not about rounding


def test_the_texel_formula_agrees_with_the_lit_render_of_the_same_points():
    """mix_color(color, light + direct, alpha) of the restated bake against the mean of lit_ref's sample colours of the primary rays
    whose first hits the elements are, on the wall with a box light; the two draw different blocks, so this is a z-test on the two
    estimated variances, two-sided at draw_ref's false-alarm probability over all points and channels.
    The setting in which both sides have the same expectation: the reference starts a Matte bounce at point + rv * 0.001f, behind
    the surface for half of the draws, where it meets the surface's own back at once (tests/test_lit_cpu.py: _wall_points); the
    bake's gather ray starts at point + n * bias, always in front (DESIGN.md 4.15 says why).  So the inner colour of a camera path
    and the bake's `light` differ by what the surface's back passes on.  With alpha = 1 and an all-zero environment that is
    nothing: the camera path at depth 2 and the bake at depth 1 then both bring light + direct = the lamp alone through the whole
    formula, fold included.  The primary rays are the pixels' centre rays (S = 1 has no jitter), each repeated spp times with keys
    (pixel, s): a jittered sample would hit beside the element.
    K = spp = 1024: the standard error of either mean is 0.3 % of it (sd / mean of one sample is about 10 % on this wall), so an
    estimator that is off by 2 % -- a missing cosine is off by 30 % -- fails with near certainty, and the run takes a second."""
    orc = _orc()
    wall = SR.recipe_wall(alpha=1.0)(CT.OracleApi(orc))
    w = h = 4
    K = spp = 1024
    li = LT.light(WALL_LIGHT, 0.5, WALL_COLOR)
    o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), 1)
    tri, t, face, _ = wall.trace(o4, d4)
    hit = np.nonzero(np.asarray(tri) != 0)[0][:6]
    pos, nrm = BR.first_hit_points(orc, wall, w, h, 6)
    rec, kinds, surf = wall.triangles()
    col, alpha = surf[np.asarray(tri)[hit], 0:3].astype(F32), surf[np.asarray(tri)[hit], 3].astype(F32)
    assert len(hit) == 6 and (alpha == 1).all()
    b = BL.bake_lit_ref(orc, wall, 5, pos, nrm, K, 1, [li], env=DARK, keep=True)
    per_k = (b.color + b.el.dk).astype(F32)  # light + direct is linear in the per-ray values
    texel = BL.texel(col, alpha, b.light, b.direct)[:, :3].astype(np.float64)
    tb = np.stack([BL.texel(np.repeat(col, K, 0), np.repeat(alpha, K), per_k, np.zeros_like(per_k))[:, c].reshape(len(hit), K) for c in range(3)], -1)
    pix, smp = np.repeat(hit, spp), np.tile(np.arange(spp), len(hit))
    r = LT.path_trace(wall, np.repeat(o4[hit], spp, 0), np.repeat(d4[hit], spp, 0), pix, smp, 2, 5, [li], env=DARK)
    tr = r.color[:, :3].astype(np.float64).reshape(len(hit), spp, 3)
    assert r.live[0] == [len(hit) * spp] and r.occluded[0] == [0] and b.el.visible == [len(hit) * K]
    mean_r = tr.mean(1)
    se = np.sqrt(tb.astype(np.float64).var(1, ddof=1) / K + tr.var(1, ddof=1) / spp)
    bound = DR.z_quantile(DR.P_FALSE / (2 * 3 * len(hit)))
    z = np.abs(texel - mean_r) / se
    print(f"texel vs lit render: largest |z| {z.max():.2f} (bound {bound:.2f}), se / mean {(se / mean_r).max():.2e}")
    assert (z <= bound).all() and (se / mean_r).max() < 0.01 and (mean_r > 0.05).all()


# ---------------------------------------------------------------- what the GPU cases rely on
def test_the_gpu_cases_conditions_hold_on_the_restatement(teapot):
    """Measured on the 58 elements x K = 5 = 290 candidates per light: lights A + B culled 64 / 110, occluded 44 / 115, visible
    182 / 65; the four lights 64 / 110 / 145 / 81, 44 / 115 / 64 / 110, 182 / 65 / 81 / 99.  Live candidates per path level
    0 .. 2 with A + B: 9 + 14, 17 + 11, 7 + 12 (the four lights: 9 + 14 + 19 + 6, 17 + 11 + 9 + 16, 7 + 12 + 14 + 7); none at the
    exhausted level 3."""
    orc = _orc()
    pos, nrm = BL.elements(orc, teapot)
    n = len(pos) * BL.K
    for name, lights, sq in (("A + B", BL.AB, False), ("four lights", BL.FOUR, True)):
        r = BL.bake_lit_ref(orc, teapot, BL.SEED, pos, nrm, BL.K, BL.DEPTH, lights, sq, pixel0=BL.PIXEL0)
        print(f"{name}: {n} element candidates per light: culled {r.el.culled}, occluded {r.el.occluded}, visible {r.el.visible}; "
              f"live per level {r.pt.live}")
        for l in range(len(lights)):
            assert min(r.el.culled[l], r.el.occluded[l], r.el.visible[l]) >= 0.05 * n, (name, l)
            assert r.el.culled[l] + r.el.occluded[l] + r.el.visible[l] == n
            assert all(r.pt.live[j][l] > 0 for j in range(BL.DEPTH - 1))  # every level below the exhausted one
        assert r.pt.live[BL.DEPTH - 1] == [0] * len(lights)
    far = BL.bake_lit_ref(orc, teapot, BL.SEED, pos, nrm, BL.K, BL.DEPTH, [LT.FAR_BEHIND], pixel0=BL.PIXEL0)
    assert far.el.culled == [n] and far.el.live == 0 and far.pt.nlive == 0 and not far.direct.view(np.uint32).any()
