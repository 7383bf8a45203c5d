"""The definition of box lights on shaded surfaces (RTMI_LIT_SURFACES; include/rtmi.h "BOX LIGHTS ON SHADED SURFACES") in float32
NumPy: the bounce loop of nmap_ref.path_trace (the oracle's closest hits, smooth_ref's shading normal and bounce, tex_ref's colour,
nmap_ref's mapped normal) with lit_ref's lamps at every Matte hit that bounces.  The parts are imported, not restated; what is new
here is `candidates`, lit_ref.candidates with two normals: the shading normal N gives c, the geometric normal ng gives the origin's
offset and the second liveness test.  It asserts that it equals lit_ref.candidates bit for bit when N is ng.  `path_trace` takes
arbitrary rays and keys (the explicit-ray form), `render` the camera's, `bake` is bake_lit_ref.bake_lit_ref with this path loop.
COUNTS names what is counted per level and light.  tests/test_lit_surfaces_cpu.py pins the restatement to lit_ref and nmap_ref and
holds it against a float64 referee before anything trusts it.  A plain helper module of tests/test_lit_surfaces_cpu.py and
tests/test_lit_surfaces.py."""
from types import SimpleNamespace

import numpy as np

import bake_lit_ref as BL
import bake_ref as BR
import envlight_ref as EL
import features_ref as FR
import light_ref as LR
import lit_ref as LT
import nmap_ref as NR
import occluded_ref as OR
import smooth_ref as SR
import tex_ref as TR
from camera_ref import fold
from env_ref import lookup as env_lookup
from glass_ref import DIELECTRIC, keys_of, random_vec_u
from rays_ref import fold as fold_rays
from shadowed_ref import SOLID, mix_color

F32 = np.float32
SURFACES = 4  # RTMI_LIT_SURFACES
# per level j and light l ([j][l]): candidates = culled_n + culled_ng + live, live = occluded + visible; differs: N != ng in at least
# one bit; mapped: the normal map's result is N (usem); back: on a back face; the last three count candidates, live or not
COUNTS = ("candidates", "culled_n", "culled_ng", "live", "occluded", "visible", "differs", "mapped", "back")


def candidates(seed, point, N4, ng4, pixel, sample, j, l, li):
    """The candidate of light l at the hits (point, N4, ng4) of level j with keys (pixel, sample): (o, dir, d2, r, c, cg) with
    c = vdot(N, dir) and cg = vdot(ng, dir), the origin offset along ng; every operation rounded to float32 on all four lanes"""
    m = len(pixel)
    w = EL.rng_blocks(seed, pixel, sample, LT.LIT_BLOCK | (l << 16) | j)
    u = EL.unit_f32(w)
    with np.errstate(all="ignore"):
        adj = np.zeros((m, 4), F32)
        adj[:, :3] = (np.asarray(li["orig"], F32)[None, :] + (u[:, :3] * F32(li["len2"])).astype(F32)).astype(F32)
        v = (adj - point).astype(F32)
        d2 = LR.odot(v, v)
        r = np.sqrt(d2).astype(F32)
        dirs = (v * (F32(1.0) / r).astype(F32)[:, None]).astype(F32)
        smudge = (F32(li.get("bias", LT.DEFAULT_BIAS)) * (u[:, 3] + F32(1.0)).astype(F32)).astype(F32)
        o = (point + (ng4 * smudge[:, None]).astype(F32)).astype(F32)
        c = LR.odot(N4, dirs)
        cg = LR.odot(ng4, dirs)
    if N4 is ng4:  # today's candidate, bit for bit
        old = LT.candidates(seed, point, ng4, pixel, sample, j, l, li)
        for a, b in zip((o, dirs, d2, r, c), old):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(cg.view(np.uint32), c.view(np.uint32))
    return o, dirs, d2, r, c, cg


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, lights=(), inverse_square=False, env=None, normals=None, tex=None, nm=None,
               trace=None, keep=False):
    """The sample colours of a lit call with RTMI_LIT_SURFACES for the rays (o4, d4) with keys (pixel, sample).  normals, tex, nm as
    nmap_ref.path_trace takes them (None: the scene lacks the feature).  Returns a namespace: color (m, 4), rays (the plain rays),
    passes, nlive, hits0, COUNTS as lists [j][l], and per level: kinds[j] = dict(matte, reflective, glass) of the levels pushed that
    bounce, lit_textured[j] = textured Matte levels whose direct is not zero; with keep: cand[j][l] = dict(idx, point, o, dir, d2,
    r, c, cg, live, occ, N, ng)."""
    lights = list(lights)
    assert len(lights) <= LT.MAX_LIGHTS
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    st = SimpleNamespace(color=color, rays=0, passes=[], nlive=0, cand=[], hits0=None, kinds=[], lit_textured=[], **{k: [] for k in COUNTS})
    if maxdepth == 0:
        return st
    recs, kinds, surf = so.triangles()
    norms = recs[:, 3:6].astype(F32)
    rec = None if normals is None else SR.records(recs[:, 20:29], normals)
    trec = None if tex is None else TR.records(recs[:, 20:29], tex.uvs, tex.tex_of_tri)
    fr = None if nm is None else NR.frames(recs[:, 20:29], tex.uvs, recs[:, 3:6], nm.nmap_of_tri)
    sky = np.array([FR.SKY[0], FR.SKY[1], FR.SKY[2], 0.0], F32)
    path = np.arange(npaths)
    cur_o, cur_d = o4, d4
    levels = []  # per pass: (paths that pushed a surface, its colour (k, 4), its alpha (k,), its direct light (k, 4))
    with np.errstate(all="ignore"):
        for j in range(maxdepth):
            st.passes.append(len(path))
            for k in COUNTS:
                getattr(st, k).append([0] * len(lights))
            st.cand.append([None] * len(lights))
            st.kinds.append(dict(matte=0, reflective=0, glass=0))
            st.lit_textured.append(0)
            if len(path) == 0:
                continue
            tri, t, face = (so.trace(cur_o, cur_d) if trace is None else trace(cur_o, cur_d))[:3]
            tri, face, t = np.asarray(tri, np.uint32), np.asarray(face, np.uint32), np.asarray(t, F32)
            if j == 0:
                st.hits0 = (tri, t, face)
            miss = tri == 0
            edge = ~miss & ((face & 2) != 0)
            surface = ~miss & ~edge
            if env is None:
                color[path[miss]] = sky
            elif miss.any():
                color[path[miss]] = env_lookup(env.table, env.frame, cur_d[miss])
            color[path[edge]] = 0.0
            kind = np.where(surface, kinds[tri], -1)
            col = np.zeros((len(path), 4), F32)
            col[:, :3] = surf[tri, 0:3].astype(F32)
            textured = np.zeros(len(path), bool)
            if trec is not None and surface.any():
                pt_all = ((cur_d[surface] * t[surface, None]).astype(F32) + cur_o[surface]).astype(F32)  # Ray::at
                c, det = TR.colour(trec, tex.images, tri[surface], pt_all, surf[tri[surface], 0:3], detail=True)
                col[surface] = c
                textured[surface] = det.textured
            solid = kind == SOLID
            color[path[solid]] = col[solid]
            go = surface & ~solid
            direct = np.zeros((int(go.sum()), 4), F32)
            levels.append((path[go], col[go], surf[tri[go], 3].astype(F32), direct))
            if maxdepth - j - 1 == 0:  # project_ray at depth 0: black, and no sample
                color[path[go]] = 0.0
                path = path[:0]
                continue
            point = ((cur_d[go] * t[go, None]).astype(F32) + cur_o[go]).astype(F32)  # Ray::at
            nrm = np.zeros((int(go.sum()), 4), F32)
            nrm[:, :3] = norms[tri[go]]
            back = (face[go] & 1) != 0
            nrm[back] = nrm[back] * F32(-1.0)
            path = path[go]
            tg, rdg = tri[go], cur_d[go]
            rv, u = random_vec_u(orc, seed, pixel[path], sample[path], j + 1)
            kg, scat = kind[go], surf[tg, 4].astype(F32)
            # ---- N: ng to start with, smooth_normal's result where use, nmap_normal's where usem
            use = np.zeros(len(path), bool)
            shade = nrm
            if rec is not None:
                sn = SR.shading_normal(rec, tg, back, point, rdg, nrm)
                use = np.array(sn.use, bool)
                shade = np.array(sn.norm, F32)
            usem = np.zeros(len(path), bool)
            if fr is not None:
                mapped = fr.nmap[tg] != 0
                if mapped.any():
                    uu, vv, _ = TR.hit_uv(trec, tg[mapped], point[mapped])
                    M = NR.lookup_maps(tex.images, fr.nmap[tg[mapped]], uu, vv)
                    res = NR.normal(fr, M, nm.strength, tg[mapped], back[mapped], shade[mapped], nrm[mapped], rdg[mapped])
                    usem[mapped] = res.usem
                    shade = np.array(shade, F32)
                    shade[mapped] = res.norm
            featured = rec is not None or fr is not None
            matte = kg == SR.MATTE
            st.kinds[-1] = dict(matte=int(matte.sum()), reflective=int((kg == SR.REFLECTIVE).sum()), glass=int((kg == DIELECTRIC).sum()))
            # ---- the candidates: one per light and bouncing Matte hit; direct = the sum over l ascending
            mi = np.nonzero(matte)[0]
            for l, li in enumerate(lights):
                st.candidates[-1][l] = len(mi)
                if not len(mi):
                    continue
                ng_m = np.ascontiguousarray(nrm[mi])
                N_m = np.ascontiguousarray(shade[mi]) if featured else ng_m
                so_, dirs, d2, r, c, cg = candidates(seed, point[mi], N_m, ng_m, pixel[path[mi]], sample[path[mi]], j, l, li)
                by_n = ~(c > F32(0.0))
                live = ~by_n & (cg > F32(0.0))
                g = (c / d2).astype(F32) if inverse_square else c
                st.culled_n[-1][l] = int(by_n.sum())
                st.culled_ng[-1][l] = int((~by_n & ~live).sum())
                st.live[-1][l] = int(live.sum())
                st.differs[-1][l] = int((N_m.view(np.uint32) != ng_m.view(np.uint32)).any(axis=1).sum())
                st.mapped[-1][l] = int(usem[mi].sum())
                st.back[-1][l] = int(back[mi].sum())
                occ = np.zeros(int(live.sum()), np.uint8)
                if live.any():
                    l_o, l_d = np.ascontiguousarray(so_[live]), np.ascontiguousarray(dirs[live])
                    tmax = None if li.get("unbounded") else np.ascontiguousarray(r[live])
                    l_tri, l_t = (so.trace(l_o, l_d) if trace is None else trace(l_o, l_d))[:2]
                    occ = np.asarray(OR.from_hits(l_tri, l_t, tmax), np.uint8)
                    st.occluded[-1][l] = int((occ != 0).sum())
                    st.visible[-1][l] = int((occ == 0).sum())
                    vis = np.nonzero(live)[0][occ == 0]
                    wgt = np.zeros((len(vis), 4), F32)
                    wgt[:, :3] = (np.asarray(li.get("color", (1.0, 1.0, 1.0)), F32)[None, :] * g[vis, None]).astype(F32)
                    direct[mi[vis]] = (direct[mi[vis]] + wgt).astype(F32)
                if keep:
                    st.cand[-1][l] = dict(idx=path[mi], point=point[mi], o=so_, dir=dirs, d2=d2, r=r, c=c, cg=cg, live=live, occ=occ, N=N_m,
                                          ng=ng_m)
            st.lit_textured[-1] = int((textured[go] & matte & (direct != 0).any(axis=1)).sum())
            # ---- the bounce: shade_hit's, with the wrong-side re-evaluation
            bo = SR.bounce(kg, point, shade, nrm, use | usem, rdg, scat, back, rv, u)
            cur_o, cur_d = np.ascontiguousarray(bo.o), np.ascontiguousarray(bo.d)
        for paths_j, col_j, alpha_j, direct_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, (color[paths_j] + direct_j).astype(F32), alpha_j)
    st.rays = sum(st.passes)
    st.nlive = sum(sum(x) for x in st.live)
    return st


def total(st, name, level=None):
    """The sum of a count over the lights, of level `level` or of all levels"""
    rows = getattr(st, name)
    return sum(sum(x) for x in rows) if level is None else sum(rows[level]) if level < len(rows) else 0


def render(orc, so, vp12, w, h, spp, seed, maxdepth, lights=(), inverse_square=False, env=None, normals=None, tex=None, nm=None, sample0=0,
           nsamples=None, tile=None, accum0=None, trace=None, keep=False):
    """The expected buffers of one rtmi_render_lit* call with the flag (frame, progressive pass or tile): image, accum (rows, w, 4),
    color, rays (the plain rays), nlive (the live candidates traced); pt is path_trace's namespace"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, lights, inverse_square, env, normals, tex, nm, trace, keep)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, nlive=pt.nlive,
                           passes=pt.passes, pt=pt, o4=o4, d4=d4, pixel=pixel, sample=sample, npix=npix, n=n)


def bake(orc, so, seed, pos4, nrm4, K, maxdepth, lights=(), inverse_square=False, pixel0=0, bias=0.001, mode="points", env=None,
         normals=None, tex=None, nm=None, want_light=True, want_direct=True, want_open=True):
    """bake_lit_ref.bake_lit_ref on a featured scene: the gather paths through path_trace above; the element's own candidates are
    bake_lit_ref.direct's, with the caller's normal in both roles"""
    lights = list(lights)
    r = BR.rays(orc, seed, pos4, nrm4, K, pixel0, bias, mode)
    nrays, pt, el, light, dir_, open_ = 0, None, None, None, None, None
    if want_light and maxdepth:
        pt = path_trace(orc, so, r.orig, r.dir, r.pixel, r.sample, maxdepth, seed, lights, inverse_square, env, normals, tex, nm)
        light = fold_rays(pt.color, K)
        nrays += pt.rays + pt.nlive
        tri0 = pt.hits0[0]
    elif want_light:
        light = np.zeros((len(r.orig) // K, 4), F32)
    if want_open:
        if not (want_light and maxdepth):
            tri0 = np.asarray(so.trace(r.orig, r.dir)[0])
            nrays += len(r.orig)
        open_ = BR.open_from_hits(tri0, K)
    if want_direct:
        n = np.repeat(np.asarray(nrm4, F32).reshape(-1, 4), K, axis=0)
        el = BL.direct(so, seed, r.point, n, r.pixel, r.sample, K, lights, inverse_square)
        dir_ = el.direct
        nrays += el.live
    return SimpleNamespace(orig=r.orig, dir=r.dir, open=open_, light=light, direct=dir_, rays=nrays, pt=pt, el=el)
