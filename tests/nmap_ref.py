"""The definition of a scene's normal maps (rtmi_scene_set_normal_maps / rtmi_normal_map_from_height, include/rtmi.h "NORMAL MAPS OF
A SCENE") in float32 NumPy: `frames`, `normal` and `from_height` are the header's listings, one NumPy operation rounded to float32
per operation of the listing, and `path_trace` / `render` are tex_ref's loop restated with the normal line changed: a bouncing hit
of a mapped triangle is shaded with `normal`'s result where it is usable, and the wrong-side rule runs with (use || usem).
`features` is tex_ref's with the normal plane of the same normal.  The uvs, the barycentrics and the bilinear lookup are tex_ref's
(`records`, `hit_uv`, `lookup`), the vertex normal smooth_ref's.  COUNTERS names what the restatement counts per hit.
tests/test_nmap_cpu.py pins the restatement to tex_ref (no maps: bit for bit) and to a float64 textbook evaluation before anything
trusts it.  A plain helper module of tests/test_nmap_cpu.py and tests/test_nmap.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import smooth_ref as SR
import tex_ref as TR
from camera_ref import fold
from env_ref import lookup as env_lookup, vdot
from glass_ref import DIELECTRIC, EVENTS, keys_of, random_vec_u
from rays_ref import vunit
from shadowed_ref import SOLID, mix_color

F32 = np.float32
v4 = SR.v4
COUNTERS = ("usem", "away_from_ray", "away_from_ng", "nan", "retry_usem", "back_usem", "flat_usem", "mapped_matte",
            "mapped_reflective", "mapped_glass", "unmapped")


def maps(nmap_of_tri, strength=1.0):
    """What the restatement takes as a scene's normal maps beside tex_ref.textures(): nmap_of_tri (ntris,), entry 0 the sentinel's"""
    return SimpleNamespace(nmap_of_tri=np.asarray(nmap_of_tri, np.int64), strength=F32(strength))


def cross(a, b):
    """(m, 4) x (m, 4) -> (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x, +0), every step rounded"""
    out = np.zeros(a.shape, F32)
    with np.errstate(all="ignore"):
        for c, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            out[..., c] = ((a[..., i] * b[..., j]).astype(F32) - (a[..., j] * b[..., i]).astype(F32)).astype(F32)
    return out


def frames(corners, uvs, facenorm, nmap_of_tri):
    """The per-triangle part of the definition: corners (n, 3, 3), uvs (n, 3, 2), facenorm (n, 3) (the records' front normals),
    nmap_of_tri (n,) -> a namespace of T (n, 4) float32, hand (n,) float32 of +-1, nmap (n,): nmap_of_tri, and 0 where det == 0.f or
    den == 0.f, and det, den (n,).  T and hand are zeros / +1 where nmap is 0, as the device's table has them."""
    rec = TR.records(corners, uvs, np.zeros(len(np.asarray(uvs).reshape(-1, 6)), np.int64))
    uv = rec.uv
    ng = v4(np.asarray(facenorm, F32).reshape(-1, 3))
    with np.errstate(all="ignore"):
        du1, du2 = (uv[:, 1, 0] - uv[:, 0, 0]).astype(F32), (uv[:, 2, 0] - uv[:, 0, 0]).astype(F32)
        dv1, dv2 = (uv[:, 1, 1] - uv[:, 0, 1]).astype(F32), (uv[:, 2, 1] - uv[:, 0, 1]).astype(F32)
        det = ((du1 * dv2).astype(F32) - (du2 * dv1).astype(F32)).astype(F32)
        T = ((rec.e1 * dv2[:, None]).astype(F32) - (rec.e2 * dv1[:, None]).astype(F32)).astype(F32)
        B = ((rec.e2 * du1[:, None]).astype(F32) - (rec.e1 * du2[:, None]).astype(F32)).astype(F32)
        neg = det < F32(0.0)
        T = np.where(neg[:, None], (T * F32(-1.0)).astype(F32), T).astype(F32)
        B = np.where(neg[:, None], (B * F32(-1.0)).astype(F32), B).astype(F32)
        hand = np.where(vdot(cross(ng, T), B) >= F32(0.0), F32(1.0), F32(-1.0)).astype(F32)
    nmap = np.where((det == F32(0.0)) | (rec.den == F32(0.0)), 0, np.asarray(nmap_of_tri, np.int64))
    none = nmap == 0
    T = np.where(none[:, None], F32(0.0), T).astype(F32)
    hand = np.where(none, F32(1.0), hand).astype(F32)
    return SimpleNamespace(T=T, hand=hand, nmap=nmap, det=det, den=rec.den)


def decode(M, strength):
    """x, y, z of the listing from the looked-up texel M (m, 4)"""
    s, one, two = F32(strength), F32(1.0), F32(2.0)
    with np.errstate(all="ignore"):
        x = (((M[:, 0] * two).astype(F32) - one).astype(F32) * s).astype(F32)
        y = (((M[:, 1] * two).astype(F32) - one).astype(F32) * s).astype(F32)
        z = ((M[:, 2] * two).astype(F32) - one).astype(F32)
    return x, y, z


def normal(fr, M, strength, tri, back, N, ng, rd):
    """The per-hit listing at hits of mapped triangles `tri` (indices into fr): M (m, 4) the map's lookup, back (m,) bool = face &
    1, N (m, 4) the vertex-normal section's norm, ng, rd (m, 4).  Returns a namespace: nm (m, 4), usem (m,) bool, norm (m, 4) =
    usem ? nm : N, t, b (m, 4), and toward_ng = vdot(nm, ng) > 0, toward_ray = vdot(rd, nm) < 0, nan = a NaN in nm."""
    tri = np.asarray(tri, np.int64)
    with np.errstate(all="ignore"):
        x, y, z = decode(M, strength)
        T = fr.T[tri]
        t = vunit((T - (N * vdot(N, T)[:, None]).astype(F32)).astype(F32))
        hs = np.where(np.asarray(back, bool), (fr.hand[tri] * F32(-1.0)).astype(F32), fr.hand[tri]).astype(F32)
        b = (cross(N, t) * hs[:, None]).astype(F32)
        s = ((t * x[:, None]).astype(F32) + (b * y[:, None]).astype(F32)).astype(F32)
        nm = vunit((s + (N * z[:, None]).astype(F32)).astype(F32))
        toward_ng, toward_ray = vdot(nm, ng) > F32(0.0), vdot(rd, nm) < F32(0.0)
        usem = toward_ng & toward_ray
    return SimpleNamespace(nm=nm, usem=usem, norm=np.where(usem[:, None], nm, N).astype(F32), t=t, b=b, toward_ng=toward_ng,
                           toward_ray=toward_ray, nan=np.isnan(nm).any(axis=1))


def lookup_maps(images, k, u, v):
    """M (m, 4): tex_ref.lookup of image k[i] (1-based, never 0) at (u[i], v[i])"""
    M = np.zeros((len(k), 4), F32)
    for kk in np.unique(k):
        sel = k == kk
        M[sel] = TR.lookup(images[kk - 1], u[sel], v[sel])
    return M


def from_height(height, scale):
    """rtmi_normal_map_from_height's definition: height (h, w) -> (h, w, 3) float32"""
    hh = np.asarray(height, F32)
    s, half = F32(scale), F32(0.5)
    with np.errstate(all="ignore"):
        dx = (((np.roll(hh, -1, axis=1) - np.roll(hh, 1, axis=1)).astype(F32) * half).astype(F32) * s).astype(F32)
        dy = (((np.roll(hh, -1, axis=0) - np.roll(hh, 1, axis=0)).astype(F32) * half).astype(F32) * s).astype(F32)
        n = np.zeros((hh.size, 4), F32)
        n[:, 0], n[:, 1], n[:, 2] = (dx * F32(-1.0)).ravel(), (dy * F32(-1.0)).ravel(), F32(1.0)
        n = vunit(n)
        out = ((n[:, :3] * half).astype(F32) + half).astype(F32)
    return np.ascontiguousarray(out.reshape(hh.shape + (3,)))


def _frames_of(so, tex, nm):
    recs = so.triangles()[0]
    return frames(recs[:, 20:29], tex.uvs, recs[:, 3:6], nm.nmap_of_tri), TR.records(recs[:, 20:29], tex.uvs, tex.tex_of_tri)


def hit_normals(so, normals, tex, nm, o4, d4):
    """`norm` of the definition at the closest hits of rays (o4, d4): smooth_ref.hit_normals' namespace with norm replaced at the
    hits of mapped triangles, and mapped, usem (m,) bool, nm (m, 4; NaN where not mapped)"""
    recs = so.triangles()[0]
    nn = np.zeros((len(recs), 3, 3), F32) if normals is None else normals
    hn = SR.hit_normals(so, nn, o4, d4)
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    hn.mapped, hn.usem, hn.nm = np.zeros(len(hn.tri), bool), np.zeros(len(hn.tri), bool), np.full((len(hn.tri), 4), np.nan, F32)
    hn.N = np.array(hn.norm, F32)
    if nm is None:
        return hn
    fr, trec = _frames_of(so, tex, nm)
    m = hn.ok & (fr.nmap[hn.tri] != 0)
    if m.any():
        with np.errstate(all="ignore"):
            point = ((d4[m] * hn.t[m, None]).astype(F32) + o4[m]).astype(F32)
        u, v, _ = TR.hit_uv(trec, hn.tri[m], point)
        M = lookup_maps(tex.images, fr.nmap[hn.tri[m]], u, v)
        res = normal(fr, M, nm.strength, hn.tri[m], (hn.face[m] & 1) != 0, hn.norm[m], hn.ng[m], d4[m])
        hn.norm[m] = res.norm
        hn.mapped, hn.usem[m], hn.nm[m] = m, res.usem, res.nm
    return hn


def features(orc, so, normals, tex, nm, w, h, vp12, spp, seed, sample0=0, nsamples=None, tile=None, rays=None):
    """tex_ref.features with the normal plane of a scene with normal maps `nm` (maps()' namespace, or None): albedo, normal, ids"""
    rows = None if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows) if rays is None else rays
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    alb, _, ids = TR.features(orc, so, normals, tex, w, h, vp12, spp, seed, rays=(o4, d4, npix, n))
    hn = hit_normals(so, normals, tex, nm, o4, d4)
    miss = np.asarray(hn.tri) == 0
    nd = np.zeros((npix * n, 4), F32)
    nd[:, :3] = np.where(miss[:, None], F32(0.0), hn.norm[:, :3])
    nd[:, 3] = np.where(miss, F32(0.0), np.asarray(hn.t, F32))
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


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None, spheres=None, env=None, normals=None, tex=None, nm=None):
    """tex_ref.path_trace with normal maps: nm = None (tex_ref's bits) or maps()' namespace (tex must then be given).  The returned
    namespace has color, rays, passes, hits0, tex, total as tex_ref's, and `nmap`: a dict of COUNTERS over all passes."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    passes, hits0 = [], None
    cnt = dict.fromkeys(("solid", "matte", "reflective", "glass", "untextured"), 0)
    ncnt = dict.fromkeys(COUNTERS, 0)
    total = dict.fromkeys(EVENTS, 0)
    if maxdepth == 0:
        return SimpleNamespace(color=color, rays=0, passes=passes, hits0=None, tex=cnt, total=total, nmap=ncnt)
    recs, kinds, surf = so.triangles()
    norms = recs[:, 3:6].astype(F32)
    ntris = len(kinds)
    rec = None if normals is None else SR.records(recs[:, 20:29], normals)
    trec = None if tex is None else TR.records(recs[:, 20:29], tex.uvs, tex.tex_of_tri)
    fr = None if nm is None else frames(recs[:, 20:29], tex.uvs, recs[:, 3:6], nm.nmap_of_tri)
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
                color[path[miss]] = env_lookup(env.table, env.frame, cur_d[miss])
            color[path[edge]] = 0.0
            kind = np.where(surface, kinds[tri], -1)
            col = np.zeros((len(path), 4), F32)
            col[:, :3] = surf[tri, 0:3].astype(F32)
            tt = surface & (tri < ntris)
            if trec is not None and tt.any():
                pt_all = ((cur_d[tt] * t[tt, None]).astype(F32) + cur_o[tt]).astype(F32)  # Ray::at
                c, det = TR.colour(trec, tex.images, tri[tt], pt_all, surf[tri[tt], 0:3], detail=True)
                col[tt] = c
                kt = kind[tt]
                cnt["solid"] += int((det.textured & (kt == SOLID)).sum())
                cnt["matte"] += int((det.textured & (kt == SR.MATTE)).sum())
                cnt["reflective"] += int((det.textured & (kt == SR.REFLECTIVE)).sum())
                cnt["glass"] += int((det.textured & (kt == DIELECTRIC)).sum())
                cnt["untextured"] += int((~det.textured).sum())
            solid = kind == SOLID
            color[path[solid]] = col[solid]
            go = surface & ~solid
            levels.append((path[go], col[go], surf[tri[go], 3].astype(F32)))
            if maxdepth - j - 1 == 0:  # project_ray at depth 0: black
                color[path[go]] = 0.0
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
            use = np.zeros(len(path), bool)
            shade = nrm
            if rec is not None and (~sph).any():
                ts = ~sph
                sn = SR.shading_normal(rec, tri[go][ts], back[ts], point[ts], cur_d[go][ts], nrm[ts])
                use[ts] = sn.use
                shade = np.array(nrm, F32)
                shade[ts] = sn.norm
            # the normal line: norm = usem ? nm : N for a hit of a mapped triangle
            usem = np.zeros(len(path), bool)
            if fr is not None:
                tg = tri[go]
                mapped = ~sph
                mapped[mapped] = fr.nmap[tg[mapped]] != 0
                ncnt["unmapped"] += int((~mapped).sum())
                if mapped.any():
                    uu, vv, _ = TR.hit_uv(trec, tg[mapped], point[mapped])
                    M = lookup_maps(tex.images, fr.nmap[tg[mapped]], uu, vv)
                    res = normal(fr, M, nm.strength, tg[mapped], back[mapped], shade[mapped], nrm[mapped], cur_d[go][mapped])
                    usem[mapped] = res.usem
                    shade = np.array(shade, F32)
                    shade[mapped] = res.norm
                    km = kg[mapped]
                    ncnt["usem"] += int(res.usem.sum())
                    ncnt["nan"] += int(res.nan.sum())
                    ncnt["away_from_ng"] += int((~res.nan & ~res.toward_ng).sum())
                    ncnt["away_from_ray"] += int((~res.nan & res.toward_ng & ~res.toward_ray).sum())
                    ncnt["back_usem"] += int((res.usem & back[mapped]).sum())
                    ncnt["flat_usem"] += int((res.usem & ~use[mapped]).sum()) if rec is not None else 0
                    ncnt["mapped_matte"] += int((km == SR.MATTE).sum())
                    ncnt["mapped_reflective"] += int((km == SR.REFLECTIVE).sum())
                    ncnt["mapped_glass"] += int((km == DIELECTRIC).sum())
            bo = SR.bounce(kg, point, shade, nrm, use | usem, cur_d[go], scat, back, rv, u)
            ncnt["retry_usem"] += int((bo.again & usem).sum())
            glass = kg == DIELECTRIC
            total["refract_in"] += int((glass & ~bo.g.reflect & ~back).sum())
            total["refract_out"] += int((glass & ~bo.g.reflect & back).sum())
            total["schlick"] += int((glass & bo.g.reflect & ~bo.g.tir).sum())
            total["tir"] += int((glass & bo.g.tir).sum())
            cur_o, cur_d = np.ascontiguousarray(bo.o), np.ascontiguousarray(bo.d)
        for paths_j, col_j, alpha_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
    return SimpleNamespace(color=color, rays=sum(passes), passes=passes, hits0=hits0, tex=cnt, total=total, nmap=ncnt)


def render(orc, so, vp12, w, h, spp, seed, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, spheres=None, env=None,
           normals=None, tex=None, nm=None):
    """tex_ref.render with normal maps: the expected buffers of one render call (frame, progressive pass or tile)"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace, spheres, env, normals, tex, nm)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, passes=pt.passes, pt=pt,
                           o4=o4, d4=d4, pixel=pixel, sample=sample)
