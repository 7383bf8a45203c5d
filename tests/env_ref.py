"""The definition of a scene's environment (rtmi_scene_set_environment / rtmi_scene_set_sky, include/rtmi.h) in float32 NumPy:
`lookup` and `sky_table` are the header's listings, one NumPy operation rounded to float32 per operation of the listing, and
`path_trace` / `render` are glass_ref's loop restated with one line changed: a path that misses starts its fold at
lookup(table, frame, its ray's direction) instead of the sky constant.  Scene.trace supplies the closest hits, orc.rng_block the
draws; the dielectric arm, random_vec, lambertian_ray, reflect_ray and mix_color are glass_ref's and shadowed_ref's.
tests/test_env_cpu.py pins the restatement to glass_ref (no table: bit for bit) and to a float64 textbook evaluation of the
octahedral map before anything trusts it.  A plain helper module of tests/test_env_cpu.py and tests/test_env.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
from camera_ref import fold
from glass_ref import DIELECTRIC, EVENTS, dielectric_ray, keys_of, random_vec_u
from rays_ref import vunit
from shadowed_ref import MATTE, SOLID, lambertian_ray, mix_color, reflect_ray

F32 = np.float32
IDENTITY = np.eye(3, dtype=F32)
SKY_DEFAULTS = dict(up=(0.0, 1.0, 0.0), sun_dir=(-0.5, 0.7, -0.5), sun_cos=0.995, zenith=(0.15, 0.35, 0.9), horizon=(0.85, 0.9, 1.0),
                    ground=(0.25, 0.22, 0.2), sun_color=(40.0, 36.0, 28.0))  # rtmi_sky_defaults


def vdot(a, b):
    """(..., 4) x (..., 4) -> (((0 + x x) + y y) + z z) + w w in float32, as Vec3::dot (raytrace.rs:65-77)"""
    acc = (F32(0.0) + (a[..., 0] * b[..., 0]).astype(F32)).astype(F32)
    for c in (1, 2, 3):
        acc = (acc + (a[..., c] * b[..., c]).astype(F32)).astype(F32)
    return acc


def _sg(v):
    return np.where(v >= F32(0.0), F32(1.0), F32(-1.0)).astype(F32)


def oct_fold(px, py):
    """The swap-and-sign rule of the lower hemisphere, both results from the old values"""
    one = F32(1.0)
    return (((one - np.abs(py)).astype(F32)) * _sg(px)).astype(F32), (((one - np.abs(px)).astype(F32)) * _sg(py)).astype(F32)


def texel_coords(frame, d4, n):
    """Steps 1-3 of the listing: (fx, fy) before the clamp, (cx, cy) after it; (m,) float32 each"""
    d = np.asarray(d4, F32).reshape(-1, 4)
    fr = np.zeros((3, 4), F32)
    fr[:, :3] = np.asarray(IDENTITY if frame is None else frame, F32).reshape(3, 3)
    fn, half = F32(n), F32(0.5)
    with np.errstate(all="ignore"):
        mx, my, mz = (vdot(np.broadcast_to(fr[k], d.shape), d) for k in range(3))
        a = ((np.abs(mx) + np.abs(my)).astype(F32) + np.abs(mz)).astype(F32)
        px, py = (mx / a).astype(F32), (my / a).astype(F32)
        qx, qy = oct_fold(px, py)
        low = mz < F32(0.0)
        px, py = np.where(low, qx, px).astype(F32), np.where(low, qy, py).astype(F32)
        fx = ((((px * half).astype(F32) + half).astype(F32) * fn).astype(F32) - half).astype(F32)
        fy = ((((py * half).astype(F32) + half).astype(F32) * fn).astype(F32) - half).astype(F32)
        clamp = lambda f: np.where(~(f >= F32(-1.0)), F32(-1.0), np.where(f > fn, fn, f)).astype(F32)
        return fx, fy, clamp(fx), clamp(fy)


def texel_index(i, j, n):
    """The octahedral border rule: (ic, jc) of texel (i, j), i and j in [-1, n]"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    ox, oy = (i < 0) | (i >= n), (j < 0) | (j >= n)
    ic, jc = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
    jc = np.where(ox, n - 1 - jc, jc)
    ic = np.where(oy, n - 1 - ic, ic)
    return ic, jc


def lookup(table, frame, d4, detail=False):
    """The colour of the environment in the unit directions d4 (m, 4): (m, 4) float32, lane 3 from the texels' +0.  table:
    (n, n, 3), row j, column i.  The indices come from the clamped coordinates, the weights from the unclamped ones (the same
    numbers unless they are NaN).  detail: also (ix, iy, tx, ty)."""
    t = np.asarray(table, F32)
    n = t.shape[0]
    assert t.shape == (n, n, 3) and n >= 1
    t4 = np.zeros((n, n, 4), F32)
    t4[..., :3] = t
    fx, fy, cx, cy = texel_coords(frame, d4, n)
    with np.errstate(all="ignore"):
        ix, iy = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
        tx, ty = (fx - np.floor(fx)).astype(F32), (fy - np.floor(fy)).astype(F32)

        def tex(i, j):
            ic, jc = texel_index(i, j, n)
            assert ((ic >= 0) & (ic < n) & (jc >= 0) & (jc < n)).all()
            return t4[jc, ic]
        c = mix_color(mix_color(tex(ix, iy), tex(ix + 1, iy), tx), mix_color(tex(ix, iy + 1), tex(ix + 1, iy + 1), tx), ty)
    return (c, ix, iy, tx, ty) if detail else c


def texel_dirs(n):
    """The direction of every texel centre, the inverse of the map as k_env_sky runs it: (n, n, 4), [j, i]"""
    fn, one = F32(n), F32(1.0)
    i = np.arange(n, dtype=F32)
    with np.errstate(all="ignore"):
        p = ((((i + F32(0.5)).astype(F32) / fn).astype(F32) * F32(2.0)).astype(F32) - one).astype(F32)
        px, py = np.broadcast_to(p[None, :], (n, n)).astype(F32), np.broadcast_to(p[:, None], (n, n)).astype(F32)
        z = ((one - np.abs(px)).astype(F32) - np.abs(py)).astype(F32)
        qx, qy = oct_fold(px, py)
        low = z < F32(0.0)
        px, py = np.where(low, qx, px).astype(F32), np.where(low, qy, py).astype(F32)
        d = np.zeros((n * n, 4), F32)
        d[:, 0], d[:, 1], d[:, 2] = px.reshape(-1), py.reshape(-1), z.reshape(-1)
        return vunit(d).reshape(n, n, 4)


def sky_table(n, sky=None):
    """rtmi_scene_set_sky's table: (n, n, 3) float32.  sky: a dict of rtmi_sky_t's fields over SKY_DEFAULTS"""
    k = dict(SKY_DEFAULTS)
    k.update(sky or {})
    v4 = lambda v: np.array([[v[0], v[1], v[2], 0.0]], F32)
    dirs = texel_dirs(n).reshape(-1, 4)
    m = len(dirs)
    with np.errstate(all="ignore"):
        up, sun = vunit(v4(k["up"])), vunit(v4(k["sun_dir"]))
        h = vdot(dirs, np.broadcast_to(up, dirs.shape))
        grad = mix_color(np.broadcast_to(v4(k["horizon"]), (m, 4)), np.broadcast_to(v4(k["zenith"]), (m, 4)), h)
        c = np.where((h < F32(0.0))[:, None], v4(k["ground"]), grad).astype(F32)
        lit = vdot(dirs, np.broadcast_to(sun, dirs.shape)) >= F32(k["sun_cos"])
        c = np.where(lit[:, None], (c + v4(k["sun_color"])).astype(F32), c).astype(F32)
    return np.ascontiguousarray(c[:, :3].reshape(n, n, 3))


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None, spheres=None, env=None):
    """glass_ref.path_trace with the environment: env = None (the sky constant) or a namespace table (n, n, 3), frame (3, 3) or
    None.  Everything else, the returned namespace included, is glass_ref's."""
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


def render(orc, so, vp12, w, h, spp, seed, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, spheres=None, env=None):
    """glass_ref.render with the environment: the expected buffers of one render call (frame, progressive pass or tile)"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace, spheres, env)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, passes=pt.passes, pt=pt,
                           o4=o4, d4=d4, pixel=pixel, sample=sample)
