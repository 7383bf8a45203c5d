"""The definition of the dielectric surface kind (RTMI_DIELECTRIC, include/rtmi.h) in float32 NumPy, from the oracle as it is:
camera_ref.path_trace restated with the dielectric arm.  Scene.trace supplies the closest hits of every pass (the oracle's Surface
stores any integer kind, so a scene with kind 3 builds and traces; only its own render is meaningless and nothing here uses it),
Scene.triangles the normals and surfaces, orc.rng_block the draws.  Every operation of the header's listing is one NumPy
operation rounded to float32 on all four lanes; random_vec, lambertian_ray, reflect_ray and mix_color are shadowed_ref's.
tests/test_glass_cpu.py pins the restatement to the oracle (no glass: Scene.render's bits) and to an independent float64 evaluation
of Snell and Schlick before anything trusts it.  A plain helper module of tests/test_glass_cpu.py and tests/test_glass.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import light_ref as LR
from camera_ref import fold, unit_f32
from rays_ref import vunit
from shadowed_ref import MATTE, SOLID, lambertian_ray, mix_color, reflect_ray

F32 = np.float32
DIELECTRIC = 3
EVENTS = ("refract_in", "refract_out", "schlick", "tir")


def random_vec_u(orc, seed, pixel, sample, blk):
    """random_vec (raytrace.rs:188-192) of RNG block `blk` of every (pixel[i], sample[i]), and the unit float of the block's word 3"""
    v = np.zeros((len(pixel), 4), F32)
    w3 = np.zeros(len(pixel), np.uint32)
    for i in range(len(pixel)):
        w = orc.rng_block(int(seed), int(pixel[i]), int(sample[i]), int(blk))
        v[i, :3] = [F32(F32(orc.u32_to_unit_f32(int(w[c]))) - F32(0.5)) for c in range(3)]
        w3[i] = w[3]
    return vunit(v), unit_f32(w3)


def dielectric_ray(point, norm, rd, ior, back, rv, u):
    """The bounce ray of a dielectric hit, the header's listing line by line.  point, norm (already * -1.f on a back face), rd, rv:
    (n, 4); ior, u: (n,); back: (n,) bool = face & 1.  Returns a namespace: o, d (the ray as make_ray stores it), reflect, tir
    (n,) bool, and the intermediate values R, k, ci, ct, eta, td (the refracted direction before make_ray)."""
    ior, u, back = np.asarray(ior, F32), np.asarray(u, F32), np.asarray(back, bool)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        ci = np.abs(LR.odot(rd, norm)).astype(F32)
        eta = np.where(back, ior, (one / ior).astype(F32)).astype(F32)
        s2 = (one - (ci * ci).astype(F32)).astype(F32)
        k = (one - ((eta * eta).astype(F32) * s2).astype(F32)).astype(F32)
        tir = ~(k >= F32(0.0))
        ct = np.sqrt(k).astype(F32)
        cs = np.where(back, ct, ci).astype(F32)
        r0 = ((one - ior).astype(F32) / (one + ior).astype(F32)).astype(F32)
        r0 = (r0 * r0).astype(F32)
        x = (one - cs).astype(F32)
        x2 = (x * x).astype(F32)
        x5 = ((x2 * x2).astype(F32) * x).astype(F32)
        R = (r0 + ((one - r0).astype(F32) * x5).astype(F32)).astype(F32)
        reflect = tir | (u < R)
        perp = ((rd + (norm * ci[:, None]).astype(F32)).astype(F32) * eta[:, None]).astype(F32)
        par = (norm * (-ct)[:, None]).astype(F32)
        td = vunit((perp + par).astype(F32))
        to, tdd = (point + (td * F32(0.001)).astype(F32)).astype(F32), vunit(td)
        ro, rdd = reflect_ray(point, norm, rd, np.zeros(len(ior), F32), rv)
        m = reflect[:, None]
        return SimpleNamespace(o=np.where(m, ro, to).astype(F32), d=np.where(m, rdd, tdd).astype(F32), reflect=reflect, tir=tir,
                               R=R, k=k, ci=ci, ct=ct, eta=eta, td=td)


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None, spheres=None):
    """camera_ref.path_trace with the dielectric arm.  spheres (optional): a namespace center (m, 3), kind (m,), surf (m, 5) =
    (colour, alpha, scattering) of the scene's analytic spheres; hit index ntris + i is sphere i and its normal is
    vunit(point - center).  Returns a namespace: color (n, 4), rays, passes (rays per pass), hits0, events (per pass: a dict of the
    counts of EVENTS), exhausted (n,) bool: the path ended because its depth ran out, last_tir (n,) int: how many total internal
    reflections in a row the path had behind it when it ended."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    exhausted, tir_run = np.zeros(npaths, bool), np.zeros(npaths, np.int64)
    passes, events, hits0 = [], [], None
    if maxdepth == 0:
        return SimpleNamespace(color=color, rays=0, passes=passes, hits0=None, events=events, total=dict.fromkeys(EVENTS, 0),
                               exhausted=exhausted, last_tir=tir_run)
    rec, kinds, surf = so.triangles()
    norms = rec[:, 3:6].astype(F32)
    ntris = len(kinds)
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
            color[path[miss]] = sky
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
            mo, md = lambertian_ray(point, nrm, rv)
            ro, rd = reflect_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), rv)
            g = dielectric_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), back, rv, u)
            matte = (kind[go] == MATTE)[:, None]
            glass = kind[go] == DIELECTRIC
            ev = events[-1]
            ev["refract_in"] = int((glass & ~g.reflect & ~back).sum())
            ev["refract_out"] = int((glass & ~g.reflect & back).sum())
            ev["schlick"] = int((glass & g.reflect & ~g.tir).sum())
            ev["tir"] = int((glass & g.tir).sum())
            tir_run[path] = np.where(glass & g.tir, tir_run[path] + 1, 0)
            cur_o = np.ascontiguousarray(np.where(glass[:, None], g.o, np.where(matte, mo, ro)).astype(F32))
            cur_d = np.ascontiguousarray(np.where(glass[:, None], g.d, np.where(matte, md, rd)).astype(F32))
        for paths_j, col_j, alpha_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
    total = {k: sum(e[k] for e in events) for k in EVENTS}
    return SimpleNamespace(color=color, rays=sum(passes), passes=passes, hits0=hits0, events=events, total=total, exhausted=exhausted,
                           last_tir=tir_run)


def keys_of(w, rows, n, sample0=0):
    """(pixel, sample) of the rays of FR.tile_rays over image rows `rows`, in [pixel][sample] order"""
    pix = (np.repeat(np.asarray(rows, np.int64), w) * w + np.tile(np.arange(w, dtype=np.int64), len(rows)))
    return np.repeat(pix, n), np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), len(pix))


def render(orc, so, vp12, w, h, spp, seed, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, spheres=None):
    """Expected buffers of one render call (frame, progressive pass or tile) on oracle scene `so`: FR.tile_rays' primary rays,
    path_trace, walk_ray_set's fold.  Returns a namespace: image, accum (rows, w, 4), color (the sample colours), rays, passes, pt
    (path_trace's namespace), o4, d4, pixel, sample (the primary rays and their keys)."""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace, spheres)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, passes=pt.passes, pt=pt,
                           o4=o4, d4=d4, pixel=pixel, sample=sample)
