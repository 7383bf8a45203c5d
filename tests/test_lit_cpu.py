"""No GPU: the definition of box lights inside the path trace (include/rtmi.h "BOX LIGHTS IN THE PATH") as tests/lit_ref.py restates
it.  First the restatement's footing -- with no lights it is the oracle's render, and its candidate is light_ref's and
shadowed_ref's -- then what the definition must mean physically, held by a float64 referee on one Matte wall: (3) a point light
gives color * (1 - alpha) + alpha * light_color * g at every pixel, (4) a box light gives the box integral of the same in
expectation.  Last, the conditions tests/test_lit.py's GPU cases rely on, checked on the restatement alone."""
from types import SimpleNamespace

import numpy as np
import pytest

import conftest as CT
import draw_ref as DR
import geom_ref as GR
import light_ref as LR
import lit_ref as LT
import shadowed_ref as SR

F32 = np.float32
W = H = 32
SPP, SEED, MAXDEPTH = 4, 5, 4
DARK = SimpleNamespace(table=np.zeros((4, 4, 3), F32), frame=None)  # an all-zero environment: a path that escapes brings nothing
WALL_LIGHT = (3.0, 1.0, 2.0)        # in front of the wall (z ~ 6), off the camera's axis
WALL_COLOR = (0.9, 0.7, 0.5)
WALL_COLOR_SQ = (27.0, 21.0, 15.0)  # ... with RTMI_LIT_INVERSE_SQUARE: d2 is 16 to 60 on this wall
# test_a_point_light_on_a_wall_is_the_float64_formula: the largest relative deviation measured there, times 4
REL_F32 = 4 * 7.1e-7


def _orc():
    from oracle import orc
    return orc


@pytest.fixture(scope="module")
def teapot():
    return CT.recipe_canonical()(CT.OracleApi(_orc()))


@pytest.fixture(scope="module")
def wall():
    return SR.recipe_wall()(CT.OracleApi(_orc()))


# ---------------------------------------------------------------- 1, 2: the restatement's footing
def test_without_lights_the_restatement_is_the_oracles_render(teapot):
    orc = _orc()
    vo = orc.canonical_viewport(W, H)
    want, cn = teapot.render(W, H, vo, MAXDEPTH, SPP, SEED)
    got = LT.render(orc, teapot, vo, W, H, SPP, SEED, MAXDEPTH)
    CT.assert_bits_equal(got.image, want, "no lights against Scene.render")
    assert got.rays == cn["rays"] and got.nlive == 0 and got.candidates == [[] for _ in range(MAXDEPTH)]


def test_candidate_0_of_level_0_is_light_refs_and_shadowed_refs(teapot, wall):
    orc = _orc()
    w = h = 32
    vo = orc.canonical_viewport(w, h)
    li = LT.A
    r = LT.render(orc, teapot, vo, w, h, 2, SEED, MAXDEPTH, [li], keep=True)
    mine = r.pt.cand[0][0]
    tri, t, face = r.pt.hits0
    rec, kinds, _ = teapot.triangles()
    hit, o, dirs, rr, c = LR.candidates(orc, SEED, r.o4, r.d4, tri, t, face, rec[:, 3:6].astype(F32), r.pixel, r.sample, 1, li["orig"],
                                        li["len2"], li["bias"])
    matte = (kinds[tri[hit]] == SR.MATTE) & ((face[hit] & 2) == 0)
    assert np.array_equal(hit[matte], mine["idx"]) and 100 < matte.sum() < len(hit)  # Matte hits only: fewer than the hits
    for name, a, b in (("o", o[matte, 0], mine["o"]), ("dir", dirs[matte, 0], mine["dir"]), ("r", rr[matte, 0], mine["r"]),
                       ("c", c[matte, 0], mine["c"])):
        CT.assert_bits_equal(a, b, f"candidate k = 0 of light_ref: {name}")
    assert 0 < mine["live"].sum() < len(mine["live"])
    # shadowed_ref tests every surface hit; on a scene of Matte surfaces alone its level 0 is this call's, count for count.  The
    # light's box straddles the wall: some of its points lie behind it
    vo = orc.canonical_viewport(W, H)
    li = LT.light((2.0, 0.0, 5.9), 0.5)
    s = SR.shadowed_ref(orc, wall, W, H, vo, 2, 2, SEED, light=li["orig"], len2=li["len2"], bias=li["bias"])
    m = LT.render(orc, wall, vo, W, H, 2, SEED, 2, [li])
    p0 = s.passes[0]
    assert (p0["tested"], p0["culled"], p0["live"], p0["occluded"]) == (m.candidates[0][0], m.culled[0][0], m.live[0][0], m.occluded[0][0])
    assert p0["culled"] > 100 and p0["live"] > 100 and m.candidates[1] == [0]  # depth 2: level 1 is exhausted


# ---------------------------------------------------------------- 3, 4: the float64 referee on a wall
def _wall_points(wall, r):
    """float64, for every primary ray of r: whether it hit the wall (cov; the rest is meaningless where not), the hit point, the normal turned against the ray, the surface colour and alpha, and
    `inner`, what the bounce of level 0 brings back under an all-zero environment at depth 2.  That is 0 where the bounce escapes.
    The reference starts a Matte bounce at point + rv * 0.001f, behind the wall for half of the draws; such a bounce meets the
    wall's back at once, level 1 is pushed at exhausted depth and shows mix_color(color, black, alpha) = color * (1 - alpha)."""
    tri, _, face = r.pt.hits0
    cov = tri != 0  # (without jitter the rays through the wall's diagonal, an edge of thickness 0, miss both triangles)
    assert cov.mean() > 0.97 and ((face[cov] & 2) == 0).all()
    rec, kinds, surf = wall.triangles()
    assert (kinds[tri[cov]] == SR.MATTE).all()
    g = GR.geometry_from_records(rec)
    o, d = r.o4[:, :3].astype(np.float64), r.d4[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        n = g.nh[tri]
        t = (g.an[tri] / g.n_len[tri] - (n * o).sum(1)) / (n * d).sum(1)
        p = o + t[:, None] * d
        n = np.where(((n * d).sum(1) > 0)[:, None], -n, n)
    col, alpha = surf[tri, 0:3].astype(np.float64), surf[tri, 3].astype(np.float64)
    path1, tri1, _ = r.pt.hits[1]
    assert np.array_equal(path1, np.nonzero(cov)[0])  # every covered path bounces
    inner = np.zeros((len(tri), 3))
    inner[path1] = np.where((tri1 != 0)[:, None], surf[tri1, 0:3].astype(np.float64) * (1 - surf[tri1, 3].astype(np.float64))[:, None], 0.0)
    return cov, p, n, col, alpha, inner


def _g64(p, n, at, inverse_square):
    """g of light points `at` (..., 3) seen from (p, n) in float64"""
    v = at - p
    d2 = (v * v).sum(-1)
    c = (n * v).sum(-1) / np.sqrt(d2)
    assert (c > 0).all()
    return c / d2 if inverse_square else c


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("inverse_square", [False, True], ids=["cosine", "inverse square"])
def test_a_point_light_on_a_wall_is_the_float64_formula(inverse_square, alpha):
    """S = 1 (no jitter), depth 2, an all-zero environment, g in float64 at the float64 hit point.  Where the bounce of level 0
    escapes, a pixel is color * (1 - alpha) + alpha * light_color * g.  Where it meets the wall's back (_wall_points says why: about
    half of the pixels), the inner colour is the wall's own color * (1 - alpha) and not black, so the pixel is color * (1 - alpha) +
    alpha * (color * (1 - alpha) + light_color * g): with alpha = 1 that term vanishes and the first formula holds at every pixel,
    with alpha = 0.5 both kinds are asserted, each against its own formula.  Measured: the largest relative deviation over the
    covered pixels and three channels is 1.5e-7 (g = c) and 4.0e-7 (g = c / d2) at alpha = 0.5, 3.7e-7 and 7.1e-7 at alpha = 1
    (v = adj - point cancels a digit, and d2 squares the loss); asserted at four times the largest, REL_F32 = 2.84e-6."""
    orc = _orc()
    wall = SR.recipe_wall(alpha=alpha)(CT.OracleApi(orc))
    li = LT.light(WALL_LIGHT, 0.0, WALL_COLOR_SQ if inverse_square else WALL_COLOR)
    r = LT.render(orc, wall, orc.canonical_viewport(W, H), W, H, 1, SEED, 2, [li], inverse_square, env=DARK)
    cov, p, n, col, a, inner = (x for x in _wall_points(wall, r))
    ncov = int(cov.sum())
    assert r.candidates[0] == [ncov] and r.live[0] == [ncov] and r.occluded[0] == [0]
    p, n, col, a, inner = (x[cov] for x in (p, n, col, a, inner))  # every covered pixel
    assert (a == alpha).all()
    escaped = (inner == 0).all(1)
    assert (escaped.all() if alpha == 1.0 else 0.3 < escaped.mean() < 0.7)
    g = _g64(p, n, np.asarray(li["orig"], np.float64), inverse_square)
    lit = np.asarray(li["color"], np.float64)[None, :] * g[:, None]
    want = col * (1 - a)[:, None] + a[:, None] * (inner + lit)
    assert np.array_equal(want[escaped], (col * (1 - a)[:, None] + a[:, None] * lit)[escaped])  # the formula as it stands
    got = r.image.reshape(-1, 4)[cov, :3].astype(np.float64)
    assert (r.image.reshape(-1, 4)[~cov] == 0).all()
    dev = float(np.abs(got / want - 1).max())
    print(f"point light, inverse_square={inverse_square}, alpha={alpha}: largest relative deviation {dev:.3e}")
    assert dev <= REL_F32
    assert (r.image[..., 3] == 0).all()
    assert (a[:, None] * lit / want).min() > 0.04  # the light is a visible part of every pixel: 10^4 tolerances at the least


def test_a_box_light_on_a_wall_is_the_box_integral_in_expectation(wall):
    """256 samples per pixel (jittered) of a box light of edge 0.5.  Given a sample's path, its light point is uniform in the box
    and independent of everything else, so the pixel's mean has the expectation mean_s(color (1 - alpha) + alpha (inner_s + color_l
    E[g | p_s])) and the variance mean_s(Var[g | p_s]) (alpha color_l)^2 / 256, both from a Gauss-Legendre rule of 8^3 points over
    the box in float64 at the float64 hit points.  Two-sided at draw_ref's false-alarm probability over all pixels, channels and
    both flags, plus REL_F32 for float32's rounding."""
    orc = _orc()
    w = h = 6
    n_s = 256
    for inverse_square in (False, True):
        li = LT.light(WALL_LIGHT, 0.5, WALL_COLOR_SQ if inverse_square else WALL_COLOR)
        r = LT.render(orc, wall, orc.canonical_viewport(w, h), w, h, n_s, SEED, 2, [li], inverse_square, env=DARK)
        cov, p, n, col, alpha, inner = _wall_points(wall, r)
        assert cov.all() and r.live[0] == [w * h * n_s] and r.occluded[0] == [0]  # (jittered rays do not meet the diagonal)
        x, wq = np.polynomial.legendre.leggauss(8)
        x, wq = (x + 1) / 2, wq / 2
        gx, gy, gz = np.meshgrid(x, x, x, indexing="ij")
        nodes = np.asarray(li["orig"], np.float64) + li["len2"] * np.stack([gx, gy, gz], -1).reshape(-1, 3)
        wts = (wq[:, None, None] * wq[None, :, None] * wq[None, None, :]).reshape(-1)
        g = _g64(p[:, None, :], n[:, None, :], nodes[None, :, :], inverse_square)  # (paths, nodes)
        eg, eg2 = g @ wts, (g * g) @ wts
        lc = np.asarray(li["color"], np.float64)
        want = (col * (1 - alpha)[:, None] + alpha[:, None] * (inner + lc[None, :] * eg[:, None])).reshape(w * h, n_s, 3).mean(1)
        var = ((alpha ** 2 * (eg2 - eg ** 2))[:, None] * lc[None, :] ** 2).reshape(w * h, n_s, 3).mean(1) / n_s
        got = r.color[:, :3].astype(np.float64).reshape(w * h, n_s, 3).mean(1)
        bound = DR.z_quantile(DR.P_FALSE / (2 * 3 * w * h * 2))
        z = np.abs(got - want) / np.sqrt(var)
        print(f"box light, inverse_square={inverse_square}: largest |z| {z.max():.2f} (bound {bound:.2f}), sd / mean {(np.sqrt(var) / want).max():.2e}")
        assert (np.abs(got - want) <= bound * np.sqrt(var) + REL_F32 * want).all()
        assert (np.sqrt(var) > 4 * REL_F32 * want).all()  # the test is about the draws, not about rounding


# ---------------------------------------------------------------- 5: what the GPU cases rely on
def test_the_gpu_cases_conditions_hold_on_the_restatement(teapot):
    orc = _orc()
    vo = orc.canonical_viewport(W, H)
    r = LT.render(orc, teapot, vo, W, H, SPP, SEED, MAXDEPTH, [LT.A, LT.B])
    for l in range(2):
        n = r.candidates[0][l]
        culled, occluded = r.culled[0][l], r.occluded[0][l]
        visible = r.live[0][l] - occluded
        print(f"light {l}: level 0 candidates {n}, culled {culled}, occluded {occluded}, visible {visible}; live per level {[x[l] for x in r.live]}")
        assert n > 300 and min(culled, occluded, visible) >= 0.05 * n
        assert r.live[1][l] > 0 and r.live[2][l] > 0
    assert r.candidates[MAXDEPTH - 1] == [0, 0] and r.live[MAXDEPTH - 1] == [0, 0]  # no candidate at the exhausted level
    plain = LT.render(orc, teapot, vo, W, H, SPP, SEED, MAXDEPTH)
    assert plain.rays == r.rays and plain.passes == r.passes and not np.array_equal(plain.image, r.image)  # the paths do not move
    # the four-light case: every light has live candidates, the unbounded one is shadowed from beyond too
    f = LT.render(orc, teapot, vo, W, H, SPP, SEED, MAXDEPTH, LT.FOUR, True)
    assert all(f.live[0][l] > 0 and f.live[0][l] - f.occluded[0][l] > 0 for l in range(4))
    # the light far behind: every candidate is culled
    b = LT.render(orc, teapot, vo, W, H, SPP, SEED, MAXDEPTH, [LT.FAR_BEHIND])
    assert b.nlive == 0 and b.culled[0][0] == b.candidates[0][0] > 300
    CT.assert_bits_equal(b.image, plain.image, "every candidate culled: the image without lights")


def test_invalid_arguments_are_refused_before_the_scene_is_used():
    LT.check_invalid_arguments()
