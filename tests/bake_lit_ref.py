"""The definition of box lights on explicit rays and in the bake (rtmi_render_rays_lit*, rtmi_bake_lit*; include/rtmi.h "BOX LIGHTS ON
EXPLICIT RAYS AND IN THE BAKE") in float32 NumPy, from what already pins its parts: bake_ref's generator makes the gather rays and
the points they start from, lit_ref.path_trace (which takes arbitrary rays and keys) their colours with the lamps at every Matte
bounce, lit_ref.candidates the element's own candidates with the level field 0xFFFF, occluded_ref's rule on the oracle's closest
hits their visibility, rays_ref.fold (walk_ray_set's arithmetic) the two means.  A plain helper module of
tests/test_bake_lit_cpu.py and tests/test_bake_lit.py."""
from types import SimpleNamespace

import numpy as np

import bake_ref as BR
import lit_ref as LT
import occluded_ref as OR
from rays_ref import fold

F32 = np.float32
LEVEL = 0xFFFF  # the level field of an element's candidates: RNG block 0xC0000000 | l << 16 | 0xFFFF; path levels stop at 31


def blocks(nlights=LT.MAX_LIGHTS, maxdepth=32):
    """Every RNG block the call may draw under one key, by what draws it"""
    out = {"gather": [0], "point": [BR.BLOCK_POINT], "bounce": list(range(1, maxdepth + 1)),
           "level": [LT.LIT_BLOCK | (l << 16) | j for l in range(nlights) for j in range(maxdepth)],
           "element": [LT.LIT_BLOCK | (l << 16) | LEVEL for l in range(nlights)]}
    return out


def direct(so, seed, point, n4, pixel, sample, K, lights=(), inverse_square=False, trace=None, occluded=None, keep=False):
    """direct[m] of the header for the (element, k) pairs (point, n4) with keys (pixel, sample), element-major and k fastest ->
    namespace(direct (M, 4), dk (M K, 4), live (the candidates traced), and per light the counts culled / occluded / visible)"""
    n = len(pixel)
    dk = np.zeros((n, 4), F32)
    st = SimpleNamespace(dk=dk, live=0, culled=[], occluded=[], visible=[], cand=[])
    with np.errstate(all="ignore"):
        for l, li in enumerate(lights):
            o, dirs, d2, r, c = LT.candidates(seed, point, n4, pixel, sample, LEVEL, l, li)
            live = c > F32(0.0)
            g = (c / d2).astype(F32) if inverse_square else c
            occ = np.zeros(int(live.sum()), np.uint8)
            if live.any():
                l_o, l_d = np.ascontiguousarray(o[live]), np.ascontiguousarray(dirs[live])
                tmax = None if li.get("unbounded") else np.ascontiguousarray(r[live])
                if occluded is not None:
                    occ = np.asarray(occluded(l_o, l_d, tmax), np.uint8)
                else:
                    l_tri, l_t = (so.trace(l_o, l_d) if trace is None else trace(l_o, l_d))[:2]
                    occ = np.asarray(OR.from_hits(l_tri, l_t, tmax), np.uint8)
                vis = np.nonzero(live)[0][occ == 0]
                wgt = np.zeros((len(vis), 4), F32)
                wgt[:, :3] = (np.asarray(li.get("color", (1.0, 1.0, 1.0)), F32)[None, :] * g[vis, None]).astype(F32)
                dk[vis] = (dk[vis] + wgt).astype(F32)
            st.live += int(live.sum())
            st.culled.append(int((~live).sum()))
            st.occluded.append(int((occ != 0).sum()))
            st.visible.append(int((occ == 0).sum()))
            if keep:
                st.cand.append(dict(o=o, dir=dirs, d2=d2, r=r, c=c, g=g, live=live, occ=occ))
    st.direct = fold(dk, K)
    return st


def bake_lit_ref(orc, so, seed, pos4, nrm4, K, maxdepth, lights=(), inverse_square=False, pixel0=0, bias=0.001, mode="points", env=None,
                 trace=None, occluded=None, want_light=True, want_direct=True, want_open=True, keep=False):
    """Expected outputs of rtmi_bake_lit* on oracle scene `so` -> namespace(orig, dir, open, light, direct, rays, color, pt (lit_ref's
    path namespace: per-level counts), el (direct()'s namespace: per-light counts culled / occluded / visible)).  rays = the plain
    rays + the live candidates of the paths and of the elements, as stats.rays counts them for the outputs asked for."""
    lights = list(lights)
    r = BR.rays(orc, seed, pos4, nrm4, K, pixel0, bias, mode)
    tr = so.trace if trace is None else trace
    nrays, pt, el, light, dir_, open_ = 0, None, None, None, None, None
    if want_light and maxdepth:
        pt = LT.path_trace(so, r.orig, r.dir, r.pixel, r.sample, maxdepth, seed, lights, inverse_square, env, trace, occluded, keep)
        light = fold(pt.color, K)
        nrays += pt.rays + pt.nlive
        tri0 = pt.hits0[0]
    elif want_light:
        light = np.zeros((len(r.orig) // K, 4), F32)
    if want_open:
        if not (want_light and maxdepth):
            tri0 = np.asarray(tr(r.orig, r.dir)[0])
            nrays += len(r.orig)
        open_ = BR.open_from_hits(tri0, K)
    if want_direct:
        n = np.repeat(np.asarray(nrm4, F32).reshape(-1, 4), K, axis=0)
        el = direct(so, seed, r.point, n, r.pixel, r.sample, K, lights, inverse_square, trace, occluded, keep)
        dir_ = el.direct
        nrays += el.live
    return SimpleNamespace(orig=r.orig, dir=r.dir, open=open_, light=light, direct=dir_, rays=nrays, color=None if pt is None else pt.color,
                           pt=pt, el=el, pixel=r.pixel, sample=r.sample, point=r.point)


def texel(color, alpha, light, direct):
    """A lightmap texel of a surface (color, alpha): mix_color(color, light + direct, alpha)"""
    from shadowed_ref import mix_color
    m = light.shape[0]
    col = np.zeros((m, 4), F32)
    col[:, :3] = np.asarray(color, F32)[..., :3]
    return mix_color(col, (light + direct).astype(F32), np.broadcast_to(np.asarray(alpha, F32), (m,)).astype(F32))


# ---------------------------------------------------------------- the lights and elements the two test files share
AB = (LT.A, LT.B)
# lit_ref.FOUR's unbounded third light at (4, 5, 2) is occluded for 4 % of the element candidates of the GPU cases; moved to (3, 2, 7)
# it has 50 % culled, 21 % occluded and 29 % visible (tests/test_bake_lit_cpu.py asserts the shares of every light here)
FOUR = (LT.A, LT.B, LT.light((3.0, 2.0, 7.0), 0.25, (0.5, 0.0, 0.25), unbounded=True), LT.FOUR[3])
SEED, K, DEPTH, PIXEL0 = 7, 5, 4, 4000


def elements(orc, so):
    """The first hits of the canonical 16 x 16 view (points and normals) that the GPU cases cycle through"""
    return BR.first_hit_points(orc, so, 16, 16)
