"""The definition of a scene's vertex normals (rtmi_scene_set_normals / rtmi_smooth_normals, include/rtmi.h "VERTEX NORMALS OF A
SCENE") in float32 NumPy: `records`, `shading_normal`, `bounce` and `generate` are the header's listings, one NumPy operation
rounded to float32 per operation of the listing, and `path_trace` / `render` are env_ref's loop restated with the normal line
changed: a bouncing triangle hit is shaded with shading_normal's result where it is usable, and its bounce is evaluated again
with the geometric normal when the ray leaves on the wrong side.  `features` is features_ref's normal plane with the same normal.
Scene.trace supplies the closest hits, orc.rng_block the draws; the dielectric arm, random_vec, lambertian_ray, reflect_ray,
mix_color and the environment lookup are glass_ref's, shadowed_ref's and env_ref's.  COUNTERS names what the restatement counts:
how often `use` failed by each of its two conditions and how often the second evaluation ran, per kind.
tests/test_smooth_cpu.py pins the restatement to env_ref (no normals: bit for bit) and to a float64 textbook evaluation before
anything trusts it.  A plain helper module of tests/test_smooth_cpu.py and tests/test_smooth.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
from camera_ref import fold
from env_ref import lookup, vdot
from glass_ref import DIELECTRIC, EVENTS, dielectric_ray, keys_of, random_vec_u
from rays_ref import vunit
from shadowed_ref import MATTE, SOLID, lambertian_ray, mix_color, reflect_ray

F32 = np.float32
REFLECTIVE = 2
COUNTERS = ("smooth", "flat", "away_from_ng", "away_from_ray", "fallback_matte", "fallback_reflective", "fallback_glass_reflect",
            "fallback_glass_refract")


def v4(a3):
    """(..., 3) -> (..., 4) float32 with lane 3 = +0"""
    a3 = np.asarray(a3, F32)
    out = np.zeros(a3.shape[:-1] + (4,), F32)
    out[..., :3] = a3
    return out


def records(corners, normals):
    """The per-triangle part of the definition: corners, normals (n, 3, 3) -> a namespace of c0, e1, e2, n0, n1, n2 (n, 4) and
    d00, d01, d11, den (n,), all float32"""
    c, nn = v4(np.asarray(corners, F32).reshape(-1, 3, 3)), v4(np.asarray(normals, F32).reshape(-1, 3, 3))
    with np.errstate(all="ignore"):
        e1, e2 = (c[:, 1] - c[:, 0]).astype(F32), (c[:, 2] - c[:, 0]).astype(F32)
        d00, d01, d11 = vdot(e1, e1), vdot(e1, e2), vdot(e2, e2)
        den = ((d00 * d11).astype(F32) - (d01 * d01).astype(F32)).astype(F32)
    return SimpleNamespace(c0=c[:, 0], e1=e1, e2=e2, n0=nn[:, 0], n1=nn[:, 1], n2=nn[:, 2], d00=d00, d01=d01, d11=d11, den=den)


def shading_normal(rec, tri, back, point, rd, ng):
    """The header's listing at hits of triangles `tri` (indices into rec): point, rd, ng (m, 4) (ng already * -1.f on a back face),
    back (m,) bool = face & 1.  Returns a namespace: ns (m, 4), use (m,) bool, norm (m, 4) = use ? ns : ng, b (m, 3), and the two
    conditions of `use` on their own: toward_ng = vdot(ns, ng) > 0, toward_ray = vdot(rd, ns) < 0."""
    tri = np.asarray(tri, np.int64)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        w = (point - rec.c0[tri]).astype(F32)
        d20, d21 = vdot(w, rec.e1[tri]), vdot(w, rec.e2[tri])
        d00, d01, d11, den = rec.d00[tri], rec.d01[tri], rec.d11[tri], rec.den[tri]
        b1 = (((d11 * d20).astype(F32) - (d01 * d21).astype(F32)).astype(F32) / den).astype(F32)
        b2 = (((d00 * d21).astype(F32) - (d01 * d20).astype(F32)).astype(F32) / den).astype(F32)
        b0 = ((one - b1).astype(F32) - b2).astype(F32)
        s = ((rec.n0[tri] * b0[:, None]).astype(F32) + (rec.n1[tri] * b1[:, None]).astype(F32)).astype(F32)
        s = (s + (rec.n2[tri] * b2[:, None]).astype(F32)).astype(F32)
        ns = vunit(s)
        ns = np.where(np.asarray(back, bool)[:, None], (ns * F32(-1.0)).astype(F32), ns).astype(F32)
        toward_ng, toward_ray = vdot(ns, ng) > F32(0.0), vdot(rd, ns) < F32(0.0)
        use = toward_ng & toward_ray
    return SimpleNamespace(ns=ns, use=use, norm=np.where(use[:, None], ns, ng).astype(F32), b=np.stack([b0, b1, b2], axis=1),
                           toward_ng=toward_ng, toward_ray=toward_ray)


def _bounce_once(kind, point, norm, rd, scat, back, rv, u):
    """The bounce of every hit with normal `norm`: (o, d) as make_ray stores them, dir as passed to make_ray, side, and the
    dielectric's namespace"""
    with np.errstate(all="ignore"):
        mo, md = lambertian_ray(point, norm, rv)
        mdir = (norm + rv).astype(F32)
        ro, rdd = reflect_ray(point, norm, rd, scat, rv)
        g = dielectric_ray(point, norm, rd, scat, back, rv, u)
        matte, glass = (kind == MATTE)[:, None], kind == DIELECTRIC
        refract = glass & ~g.reflect
        o = np.where(glass[:, None], g.o, np.where(matte, mo, ro)).astype(F32)
        d = np.where(glass[:, None], g.d, np.where(matte, md, rdd)).astype(F32)
        # the direction handed to make_ray: Matte norm + rv; a reflection (the dielectric's too) the already normalised
        # reflect_dir, whose second normalisation make_ray's result is; a refraction td
        glass_dir = np.where(refract[:, None], g.td, _reflect_dir(norm, rd, np.zeros_like(scat), rv))
        dirv = np.where(glass[:, None], glass_dir, np.where(matte, mdir, _reflect_dir(norm, rd, scat, rv))).astype(F32)
        side = np.where(refract, F32(-1.0), F32(1.0)).astype(F32)
    return o, d, dirv, side, g


def _reflect_dir(norm, rd, fuzz, rv):
    """reflect_ray's `vunit(reflect + rv * scattering)`, the direction it passes to make_ray"""
    import light_ref as LR
    with np.errstate(all="ignore"):
        ddot = np.abs(LR.odot(rd, norm)).astype(F32)
        dir_p = (norm * ddot[:, None]).astype(F32)
        reflect = (dir_p + (rd + dir_p).astype(F32)).astype(F32)
        return vunit((reflect + (rv * np.asarray(fuzz, F32)[:, None]).astype(F32)).astype(F32))


def bounce(kind, point, norm, ng, use, rd, scat, back, rv, u):
    """The bounce with the fallback rule: evaluate with `norm`; where use && !(side * vdot(dir, ng) > 0.f) evaluate the whole
    bounce again with ng, same rv, same u.  Returns a namespace o, d (m, 4), again (m,) bool, g (the dielectric's namespace of
    the evaluation that counts), refract (m,) bool."""
    kind, scat, back = np.asarray(kind), np.asarray(scat, F32), np.asarray(back, bool)
    o, d, dirv, side, g = _bounce_once(kind, point, norm, rd, scat, back, rv, u)
    with np.errstate(all="ignore"):
        again = np.asarray(use, bool) & ~((side * vdot(dirv, ng)).astype(F32) > F32(0.0))
    o2, d2, _, _, g2 = _bounce_once(kind, point, ng, rd, scat, back, rv, u)
    m = again[:, None]
    reflect, tir = np.where(again, g2.reflect, g.reflect), np.where(again, g2.tir, g.tir)
    return SimpleNamespace(o=np.where(m, o2, o).astype(F32), d=np.where(m, d2, d).astype(F32), again=again,
                           g=SimpleNamespace(reflect=reflect, tir=tir), first=SimpleNamespace(reflect=g.reflect, tir=g.tir))


def generate(corners, facenorm, crease_cos):
    """rtmi_smooth_normals' definition, taken literally: corners (n, 3, 3), facenorm (n, 3) -> normals (n, 3, 3) float32.  The
    candidates of a corner are found by comparing positions with ==; the sum runs over them in increasing triangle index."""
    c = np.asarray(corners, F32).reshape(-1, 3, 3)
    fn = v4(np.asarray(facenorm, F32).reshape(-1, 3))
    n = len(c)
    cc = F32(crease_cos)
    with np.errstate(all="ignore"):
        a, b = (c[:, 1] - c[:, 0]).astype(F32), (c[:, 2] - c[:, 0]).astype(F32)
        x = np.zeros((n, 4), F32)
        x[:, 0] = ((a[:, 1] * b[:, 2]).astype(F32) - (a[:, 2] * b[:, 1]).astype(F32)).astype(F32)
        x[:, 1] = ((a[:, 2] * b[:, 0]).astype(F32) - (a[:, 0] * b[:, 2]).astype(F32)).astype(F32)
        x[:, 2] = ((a[:, 0] * b[:, 1]).astype(F32) - (a[:, 1] * b[:, 0]).astype(F32)).astype(F32)
        area = np.sqrt(vdot(x, x)).astype(F32)
        wg = (fn * area[:, None]).astype(F32)
        # candidates by position: == on floats (-0 == +0: folded onto +0 first; a NaN equals nothing: left out), found through
        # np.unique over the positions' bits; every candidate pair is checked with == below
        flat = (c.reshape(-1, 3) + F32(0.0)).astype(F32)
        valid = ~np.isnan(flat).any(axis=1)
        _, pid = np.unique(flat.view(np.uint32), axis=0, return_inverse=True)
        pid = np.asarray(pid).reshape(-1)
        corner = np.arange(3 * n)
        pairs = np.unique(np.stack([pid[valid], corner[valid] // 3], axis=1), axis=0)  # (position, triangle), sorted by both
        first = np.searchsorted(pairs[:, 0], np.arange(pid.max() + 1 if len(pid) else 0))
        count = np.bincount(pairs[:, 0], minlength=len(first))
        cidx = corner[valid]
        reps = count[pid[cidx]]
        cc_corner = np.repeat(cidx, reps)                                   # the corner of every (corner, candidate) pair
        rank = np.arange(len(cc_corner)) - np.repeat(np.cumsum(reps) - reps, reps)  # 0, 1, ... in increasing triangle index
        cand = pairs[first[pid[cc_corner]] + rank, 1]
        assert (flat[cc_corner][:, None, :] == (c[cand] + F32(0.0))).all(axis=2).any(axis=1).all()
        f_of = cc_corner // 3
        take = (cand == f_of) | (vdot(fn[f_of], fn[cand]) >= cc)
        s = np.zeros((3 * n, 4), F32)
        for r in range(int(rank.max()) + 1 if len(rank) else 0):  # every corner adds its r-th candidate: its own order is kept
            m = (rank == r) & take
            s[cc_corner[m]] = (s[cc_corner[m]] + wg[cand[m]]).astype(F32)
        out = vunit(s)[:, :3].reshape(n, 3, 3)
    return np.ascontiguousarray(out)


def hit_normals(so, normals, o4, d4):
    """`norm` of the definition at the closest hits of rays (o4, d4) on oracle scene `so` with vertex normals (ntris, 3, 3): a
    namespace tri, t, face, ng, norm (m, 4; ng where the hit is a miss or an edge face), and (m,) bool each: ok (a triangle hit
    that is no edge face), use, flat (all nine floats zero), away_from_ng, away_from_ray (the first and the second condition of
    `use` failing on a triangle that is not flat)"""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    tri, t, face, _ = so.trace(o4, d4)
    recs = so.triangles()[0]
    rec = records(recs[:, 20:29], normals)
    tri, face, t = np.asarray(tri, np.int64), np.asarray(face, np.uint32), np.asarray(t, F32)
    ng = v4(recs[tri, 3:6])
    back = (face & 1) != 0
    ng[back] = (ng[back] * F32(-1.0)).astype(F32)
    ok = (tri != 0) & ((face & 2) == 0)
    norm = np.array(ng, F32)
    z = np.zeros(len(tri), bool)
    out = SimpleNamespace(tri=tri, t=t, face=face, ng=ng, norm=norm, ok=ok, use=z.copy(), flat=z.copy(), away_from_ng=z.copy(),
                          away_from_ray=z.copy())
    if ok.any():
        with np.errstate(all="ignore"):
            point = ((d4[ok] * t[ok, None]).astype(F32) + o4[ok]).astype(F32)
        sn = shading_normal(rec, tri[ok], back[ok], point, d4[ok], ng[ok])
        norm[ok] = sn.norm
        flat = ~(np.asarray(normals, F32).reshape(-1, 9)[tri[ok]] != 0).any(axis=1)
        out.use[ok], out.flat[ok] = sn.use, flat
        out.away_from_ng[ok], out.away_from_ray[ok] = ~flat & ~sn.toward_ng, ~flat & sn.toward_ng & ~sn.toward_ray
    return out


def features(orc, so, normals, w, h, vp12, spp, seed, sample0=0, nsamples=None, tile=None, rays=None):
    """features_ref with the normal plane of a scene with vertex normals (n, 3, 3): albedo, normal (rows, w, 4), ids (rows, w).
    rays = (o4, d4, npix, n) replaces the pinhole camera's primary rays (the result is then (npix, 4), (npix, 4), (npix,))."""
    rows = None if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows) if rays is None else rays
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    hn = hit_normals(so, normals, o4, d4)
    tri, t, face, norm = hn.tri, hn.t, hn.face, hn.norm
    recs, _, surf = so.triangles()
    alb, _, ids = FR.features_from_hits(tri, t, face, recs, surf, npix, n)
    miss = np.asarray(tri) == 0
    nd = np.zeros((npix * n, 4), F32)
    nd[:, :3] = np.where(miss[:, None], F32(0.0), norm[:, :3])
    nd[:, 3] = np.where(miss, F32(0.0), np.asarray(t, F32))
    nd = nd.reshape(npix, n, 4)
    with np.errstate(all="ignore"):
        acc = np.zeros((npix, 4), F32)
        for s in range(n):
            acc = (acc + nd[:, s]).astype(F32)
        nrm = (acc * (F32(1.0) / F32(n))).astype(F32)
    if rays is not None:
        return alb, nrm, ids
    nr = npix // w
    return alb.reshape(nr, w, 4), nrm.reshape(nr, w, 4), ids.reshape(nr, w)


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None, spheres=None, env=None, normals=None):
    """env_ref.path_trace with vertex normals: normals = None (flat: env_ref's bits) or (ntris, 3, 3), entry 0 the sentinel's.
    The returned namespace is env_ref's, and `smooth`: a dict of COUNTERS over all passes."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    exhausted, tir_run = np.zeros(npaths, bool), np.zeros(npaths, np.int64)
    passes, events, hits0 = [], [], None
    cnt = dict.fromkeys(COUNTERS, 0)
    if maxdepth == 0:
        return SimpleNamespace(color=color, rays=0, passes=passes, hits0=None, events=events, total=dict.fromkeys(EVENTS, 0),
                               exhausted=exhausted, last_tir=tir_run, smooth=cnt)
    recs, kinds, surf = so.triangles()
    norms = recs[:, 3:6].astype(F32)
    ntris = len(kinds)
    rec = None if normals is None else records(recs[:, 20:29], normals)
    centers = np.zeros((0, 3), F32)
    if spheres is not None:
        centers = np.asarray(spheres.center, F32).reshape(-1, 3)
        kinds = np.concatenate([kinds, np.asarray(spheres.kind, kinds.dtype)])
        surf = np.concatenate([surf, np.asarray(spheres.surf, F32).reshape(-1, 5)])
        norms = np.concatenate([norms, np.zeros((len(centers), 3), F32)])
    sky = np.array([FR.SKY[0], FR.SKY[1], FR.SKY[2], 0.0], F32)
    path = np.arange(npaths)
    cur_o, cur_d = o4, d4
    levels = []  # per pass: (paths that pushed a surface, its colour (k, 4), its alpha (k,))
    with np.errstate(all="ignore"):
        for j in range(maxdepth):
            passes.append(len(path))
            events.append(dict.fromkeys(EVENTS, 0))
            if len(path) == 0:
                continue
            if trace is None:
                tri, t, face, _ = so.trace(cur_o, cur_d)
            else:
                tri, t, face = trace(cur_o, cur_d)[:3]
            tri, face, t = np.asarray(tri, np.uint32), np.asarray(face, np.uint32), np.asarray(t, F32)
            if j == 0:
                hits0 = (tri, t, face)
            miss = tri == 0
            edge = ~miss & ((face & 2) != 0)
            surface = ~miss & ~edge
            if env is None:
                color[path[miss]] = sky
            elif miss.any():
                color[path[miss]] = lookup(env.table, env.frame, cur_d[miss])
            color[path[edge]] = 0.0
            kind = np.where(surface, kinds[tri], -1)
            col = np.zeros((len(path), 4), F32)
            col[:, :3] = surf[tri, 0:3].astype(F32)
            solid = kind == SOLID
            color[path[solid]] = col[solid]
            go = surface & ~solid
            levels.append((path[go], col[go], surf[tri[go], 3].astype(F32)))
            if maxdepth - j - 1 == 0:  # project_ray at depth 0: black
                color[path[go]] = 0.0
                exhausted[path[go]] = True
                path = path[:0]
                continue
            point = ((cur_d[go] * t[go, None]).astype(F32) + cur_o[go]).astype(F32)  # Ray::at
            nrm = np.zeros((int(go.sum()), 4), F32)
            nrm[:, :3] = norms[tri[go]]
            sph = tri[go] >= ntris
            if sph.any():  # (point - center).unit()
                c4 = np.zeros((int(sph.sum()), 4), F32)
                c4[:, :3] = centers[tri[go][sph] - ntris]
                nrm[sph] = vunit((point[sph] - c4).astype(F32))
            back = (face[go] & 1) != 0
            nrm[back] = nrm[back] * F32(-1.0)
            path = path[go]
            rv, u = random_vec_u(orc, seed, pixel[path], sample[path], j + 1)
            kg, scat = kind[go], surf[tri[go], 4].astype(F32)
            # the normal line: norm = use ? ns : ng for a triangle hit of a scene with vertex normals
            use = np.zeros(len(path), bool)
            shade = nrm
            if rec is not None and (~sph).any():
                tt = ~sph
                sn = shading_normal(rec, tri[go][tt], back[tt], point[tt], cur_d[go][tt], nrm[tt])
                use[tt] = sn.use
                shade = np.array(nrm, F32)
                shade[tt] = sn.norm
                isflat = ~(np.asarray(normals, F32).reshape(-1, 9)[tri[go][tt]] != 0).any(axis=1)
                cnt["smooth"] += int(sn.use.sum())
                cnt["flat"] += int(isflat.sum())
                cnt["away_from_ng"] += int((~isflat & ~sn.toward_ng).sum())
                cnt["away_from_ray"] += int((~isflat & sn.toward_ng & ~sn.toward_ray).sum())
            bo = bounce(kg, point, shade, nrm, use, cur_d[go], scat, back, rv, u)
            glass = kg == DIELECTRIC
            cnt["fallback_matte"] += int((bo.again & (kg == MATTE)).sum())
            cnt["fallback_reflective"] += int((bo.again & (kg == REFLECTIVE)).sum())
            cnt["fallback_glass_reflect"] += int((bo.again & glass & bo.first.reflect).sum())
            cnt["fallback_glass_refract"] += int((bo.again & glass & ~bo.first.reflect).sum())
            g = bo.g
            ev = events[-1]
            ev["refract_in"] = int((glass & ~g.reflect & ~back).sum())
            ev["refract_out"] = int((glass & ~g.reflect & back).sum())
            ev["schlick"] = int((glass & g.reflect & ~g.tir).sum())
            ev["tir"] = int((glass & g.tir).sum())
            tir_run[path] = np.where(glass & g.tir, tir_run[path] + 1, 0)
            cur_o, cur_d = np.ascontiguousarray(bo.o), np.ascontiguousarray(bo.d)
        for paths_j, col_j, alpha_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
    total = {k: sum(e[k] for e in events) for k in EVENTS}
    return SimpleNamespace(color=color, rays=sum(passes), passes=passes, hits0=hits0, events=events, total=total, exhausted=exhausted,
                           last_tir=tir_run, smooth=cnt)


def render(orc, so, vp12, w, h, spp, seed, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, spheres=None, env=None,
           normals=None):
    """env_ref.render with vertex normals: the expected buffers of one render call (frame, progressive pass or tile)"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace, spheres, env, normals)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, passes=pt.passes, pt=pt,
                           o4=o4, d4=d4, pixel=pixel, sample=sample)
