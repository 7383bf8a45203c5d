"""The definition of a scene's textures (rtmi_scene_set_textures / rtmi_project_uvs, include/rtmi.h "TEXTURES OF A SCENE") in
float32 NumPy: `records`, `hit_uv`, `lookup`, `colour` and `project` are the header's listings, one NumPy operation rounded to
float32 per operation of the listing, and `path_trace` / `render` are smooth_ref's loop restated with the colour line changed: a
triangle hit that is no edge face and has a texture is coloured by `colour`, a Solid hit ends with it and every other hit's level
folds with it.  `features` is smooth_ref's with the albedo plane of the same colour.  Scene.trace supplies the closest hits,
orc.rng_block the draws; the normals, the bounce, the dielectric arm, mix_color and the environment lookup are smooth_ref's,
glass_ref's, shadowed_ref's and env_ref's.  tests/test_tex_cpu.py pins the restatement to smooth_ref (no textures, and all-ones
textures: bit for bit) and to a float64 textbook evaluation before anything trusts it.  A plain helper module of
tests/test_tex_cpu.py and tests/test_tex.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import smooth_ref as SR
from camera_ref import fold
from env_ref import lookup as env_lookup, vdot
from glass_ref import DIELECTRIC, EVENTS, keys_of, random_vec_u
from rays_ref import vunit
from shadowed_ref import SOLID, mix_color

F32 = np.float32
v4 = SR.v4


def textures(images, uvs, tex_of_tri):
    """What the restatement takes as a scene's textures: images a list of (h, w, 3), uvs (ntris, 3, 2), tex_of_tri (ntris,), entry 0
    the sentinel's"""
    return SimpleNamespace(images=[np.asarray(im, F32) for im in images], uvs=np.asarray(uvs, F32).reshape(-1, 3, 2),
                           tex_of_tri=np.asarray(tex_of_tri, np.int64))


def records(corners, uvs, tex_of_tri):
    """The per-triangle part of the definition: corners (n, 3, 3), uvs (n, 3, 2), tex_of_tri (n,) -> smooth_ref.records' namespace
    (c0, e1, e2, d00, d01, d11, den by the vertex-normal section's statements) with uv (n, 3, 2) float32 and tex (n,): tex_of_tri,
    and 0 where den == 0.f"""
    rec = SR.records(corners, np.zeros((len(np.asarray(corners).reshape(-1, 9)), 3, 3), F32))
    rec.uv = np.asarray(uvs, F32).reshape(-1, 3, 2)
    rec.tex = np.where(rec.den == F32(0.0), 0, np.asarray(tex_of_tri, np.int64))
    return rec


def hit_uv(rec, tri, point):
    """(u, v) (m,) float32 each at `point` (m, 4) of triangles `tri`, and the barycentric coordinates b (m, 3)"""
    tri = np.asarray(tri, np.int64)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        w = (point - rec.c0[tri]).astype(F32)
        d20, d21 = vdot(w, rec.e1[tri]), vdot(w, rec.e2[tri])
        d00, d01, d11, den = rec.d00[tri], rec.d01[tri], rec.d11[tri], rec.den[tri]
        b1 = (((d11 * d20).astype(F32) - (d01 * d21).astype(F32)).astype(F32) / den).astype(F32)
        b2 = (((d00 * d21).astype(F32) - (d01 * d20).astype(F32)).astype(F32) / den).astype(F32)
        b0 = ((one - b1).astype(F32) - b2).astype(F32)
        uv = rec.uv[tri]
        out = []
        for c in (0, 1):
            s = ((uv[:, 0, c] * b0).astype(F32) + (uv[:, 1, c] * b1).astype(F32)).astype(F32)
            out.append((s + (uv[:, 2, c] * b2).astype(F32)).astype(F32))
    return out[0], out[1], np.stack([b0, b1, b2], axis=1)


def texel_coords(u, n):
    """One axis of the lookup: coordinate u (m,) on an axis of n texels -> (fx unclamped, index i0 = floor of the clamped value,
    weight t), float32 / int64 / float32"""
    u = np.asarray(u, F32)
    fn = F32(n)
    with np.errstate(all="ignore"):
        fu = (u - np.floor(u).astype(F32)).astype(F32)
        fx = ((fu * fn).astype(F32) - F32(0.5)).astype(F32)
        top = (fn - F32(1.0)).astype(F32)
        cx = np.where(~(fx >= F32(-1.0)), F32(-1.0), np.where(fx > top, top, fx)).astype(F32)
        i0 = np.floor(cx).astype(np.int64)
        t = (fx - np.floor(fx).astype(F32)).astype(F32)
    return fx, i0, t


def wrap(i, n):
    """one wrap step of the repeat"""
    return np.where(i < 0, i + n, np.where(i >= n, i - n, i))


def lookup(image, u, v, detail=False):
    """The bilinear, repeating lookup of `image` (h, w, 3; row 0 is v = 0) at (u, v) (m,): (m, 4) float32, lane 3 the texels' +0.
    detail: also (ix, iy, tx, ty)."""
    img = np.asarray(image, F32)
    h, w = img.shape[:2]
    t4 = np.zeros((h, w, 4), F32)
    t4[..., :3] = img
    _, ix, tx = texel_coords(u, w)
    _, iy, ty = texel_coords(v, h)
    x0, x1, y0, y1 = wrap(ix, w), wrap(ix + 1, w), wrap(iy, h), wrap(iy + 1, h)
    assert ((x0 >= 0) & (x0 < w) & (x1 >= 0) & (x1 < w) & (y0 >= 0) & (y0 < h) & (y1 >= 0) & (y1 < h)).all()
    with np.errstate(all="ignore"):
        out = mix_color(mix_color(t4[y0, x0], t4[y0, x1], tx), mix_color(t4[y1, x0], t4[y1, x1], tx), ty)
    return (out, ix, iy, tx, ty) if detail else out


def colour(rec, images, tri, point, mat_rgb, detail=False):
    """The colour of hits of triangles `tri` at `point` (m, 4) whose material colours are mat_rgb (m, 3): (m, 4) float32 with lane
    3 +0.  An untextured triangle's is its material's, unmodified.  detail: also a namespace of textured (m,) bool and, NaN / -9
    where untextured, u, v, ix, iy, and the images' w, h per hit."""
    tri = np.asarray(tri, np.int64)
    out = v4(np.asarray(mat_rgb, F32))
    k = rec.tex[tri]
    u, v, _ = hit_uv(rec, tri, point)
    m = len(tri)
    d = SimpleNamespace(textured=k != 0, u=u, v=v, ix=np.full(m, -9), iy=np.full(m, -9), w=np.zeros(m, np.int64), h=np.zeros(m, np.int64), tex=k)
    for kk in np.unique(k[k != 0]):
        sel = k == kk
        img = images[kk - 1]
        tc, ix, iy, _, _ = lookup(img, u[sel], v[sel], detail=True)
        with np.errstate(all="ignore"):
            c = np.zeros((int(sel.sum()), 4), F32)
            c[:, :3] = (np.asarray(mat_rgb, F32)[sel] * tc[:, :3]).astype(F32)
        out[sel] = c
        d.ix[sel], d.iy[sel], d.w[sel], d.h[sel] = ix, iy, img.shape[1], img.shape[0]
    return (out, d) if detail else out


def project(corners, facenorm, lo, scale):
    """rtmi_project_uvs' definition: corners (n, 3, 3), facenorm (n, 3) -> uvs (n, 3, 2) float32"""
    c = np.asarray(corners, F32).reshape(-1, 3, 3)
    a = np.abs(np.asarray(facenorm, F32).reshape(-1, 3))
    lo, scale = np.asarray(lo, F32), F32(scale)
    ax = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    j, k = (ax + 1) % 3, (ax + 2) % 3
    r = np.arange(len(c))
    out = np.zeros((len(c), 3, 2), F32)
    with np.errstate(all="ignore"):
        for p in range(3):
            out[:, p, 0] = ((c[r, p, j] - lo[j]).astype(F32) * scale).astype(F32)
            out[:, p, 1] = ((c[r, p, k] - lo[k]).astype(F32) * scale).astype(F32)
    return out


def features(orc, so, normals, tex, w, h, vp12, spp, seed, sample0=0, nsamples=None, tile=None, rays=None):
    """smooth_ref.features with the albedo plane of a scene with textures `tex` (textures()' namespace): albedo, normal, ids.
    normals may be None (flat)."""
    rows = None if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows) if rays is None else rays
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    recs, _, surf = so.triangles()
    nn = np.zeros((len(recs), 3, 3), F32) if normals is None else normals
    _, nrm, ids = SR.features(orc, so, nn, w, h, vp12, spp, seed, rays=(o4, d4, npix, n))
    tri, t, face, _ = so.trace(o4, d4)
    tri, face, t = np.asarray(tri, np.int64), np.asarray(face, np.uint32), np.asarray(t, F32)
    miss, edge = tri == 0, (face & 2) != 0
    ok = ~miss & ~edge
    a = np.zeros((npix * n, 4), F32)
    a[:, :3] = np.where(miss[:, None], FR.SKY, F32(0.0))
    a[:, 3] = np.where(miss, F32(0.0), F32(1.0))
    if ok.any():
        rec = records(recs[:, 20:29], tex.uvs, tex.tex_of_tri)
        with np.errstate(all="ignore"):
            point = ((d4[ok] * t[ok, None]).astype(F32) + o4[ok]).astype(F32)
        a[ok, :3] = colour(rec, tex.images, tri[ok], point, surf[tri[ok], 0:3])[:, :3]
    a = a.reshape(npix, n, 4)
    with np.errstate(all="ignore"):
        acc = np.zeros((npix, 4), F32)
        for s in range(n):
            acc = (acc + a[:, s]).astype(F32)
        alb = (acc * (F32(1.0) / F32(n))).astype(F32)
    if rays is not None:
        return alb, nrm, ids
    nr = npix // w
    return alb.reshape(nr, w, 4), nrm.reshape(nr, w, 4), ids.reshape(nr, w)


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None, spheres=None, env=None, normals=None, tex=None):
    """smooth_ref.path_trace with textures: tex = None (smooth_ref's bits) or textures()' namespace.  The returned namespace has
    color, rays, passes, hits0, and `tex`: a dict of counters over all passes -- textured hits per kind (solid, matte, reflective,
    glass) and untextured surface hits."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    passes, hits0 = [], None
    cnt = dict.fromkeys(("solid", "matte", "reflective", "glass", "untextured"), 0)
    total = dict.fromkeys(EVENTS, 0)
    if maxdepth == 0:
        return SimpleNamespace(color=color, rays=0, passes=passes, hits0=None, tex=cnt, total=total)
    recs, kinds, surf = so.triangles()
    norms = recs[:, 3:6].astype(F32)
    ntris = len(kinds)
    rec = None if normals is None else SR.records(recs[:, 20:29], normals)
    trec = None if tex is None else records(recs[:, 20:29], tex.uvs, tex.tex_of_tri)
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
            # the colour line: a triangle hit (no sphere, no edge face) of a scene with textures
            tt = surface & (tri < ntris)
            if trec is not None and tt.any():
                pt_all = ((cur_d[tt] * t[tt, None]).astype(F32) + cur_o[tt]).astype(F32)  # Ray::at
                c, det = colour(trec, tex.images, tri[tt], pt_all, surf[tri[tt], 0:3], detail=True)
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
            bo = SR.bounce(kg, point, shade, nrm, use, cur_d[go], scat, back, rv, u)
            glass = kg == DIELECTRIC
            total["refract_in"] += int((glass & ~bo.g.reflect & ~back).sum())
            total["refract_out"] += int((glass & ~bo.g.reflect & back).sum())
            total["schlick"] += int((glass & bo.g.reflect & ~bo.g.tir).sum())
            total["tir"] += int((glass & bo.g.tir).sum())
            cur_o, cur_d = np.ascontiguousarray(bo.o), np.ascontiguousarray(bo.d)
        for paths_j, col_j, alpha_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
    return SimpleNamespace(color=color, rays=sum(passes), passes=passes, hits0=hits0, tex=cnt, total=total)


def render(orc, so, vp12, w, h, spp, seed, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, spheres=None, env=None,
           normals=None, tex=None):
    """smooth_ref.render with textures: the expected buffers of one render call (frame, progressive pass or tile)"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace, spheres, env, normals, tex)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, passes=pt.passes, pt=pt,
                           o4=o4, d4=d4, pixel=pixel, sample=sample)
