"""The definition of the built-in camera models (rtmi_render_camera*, include/rtmi.h) in float32 NumPy, from the oracle as it is.
Two parts.  camera_rays restates the ray of (row, col, sample) operation by operation, every step rounded to float32 on all four
lanes: pixel_ray's image-plane point, the orthographic axis, the lens sample and the thin lens; orc.rng_block supplies the draws.
path_trace is the bounce loop from explicit rays, built from shadowed_ref's random_vec, lambertian_ray, reflect_ray and mix_color
and from Scene.trace.  render puts them together with walk_ray_set's fold and features_ref.features_from_hits for the guides.
tests/test_camera_cpu.py pins both parts to the oracle (the pinhole's rays are orc.primary_rays, path_trace over them is
Scene.render) before anything trusts them.  A plain helper module of tests/test_camera_cpu.py and tests/test_camera.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
from rays_ref import vunit
from shadowed_ref import MATTE, SOLID, lambertian_ray, mix_color, random_vec, reflect_ray

F32 = np.float32
PINHOLE, THIN_LENS, ORTHO = 0, 1, 2
LENS_BLOCK = 0x40000000
# (1 - pi/4)^4: the probability that all four candidates of a lens sample miss the unit disc
P_FALLBACK = (1.0 - np.pi / 4.0) ** 4


def cam(model, lens_radius=0.0, focus=1.0):
    """What camera_rays reads of an rtmi_camera_t"""
    return SimpleNamespace(model=int(model), lens_radius=float(F32(lens_radius)), focus=float(F32(focus)))


def unit_f32(w):
    """rand's Standard f32 of uint32 words: the top 24 bits * 2^-24 (exact in float32)"""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def _v4(a3):
    out = np.zeros(4, F32)
    out[:3] = np.asarray(a3, F32)
    return out


def _blocks(orc, seed, pixel, sample, blk):
    """(n, 4) uint32: RNG block `blk` of every (pixel[i], sample[i])"""
    return np.array([orc.rng_block(int(seed), int(p), int(s), int(blk)) for p, s in zip(pixel, sample)], np.uint32).reshape(-1, 4)


def lens_samples(orc, seed, pixel, sample):
    """The lens sample of every key: (x, y, candidate) with candidate = 2 k + j of the one taken, 4 = none (the sample is (0, 0)).
    Candidate 2 k + j is (2 u(w[2 j]) - 1, 2 u(w[2 j + 1]) - 1) of block LENS_BLOCK | k."""
    n = len(pixel)
    x, y, taken = np.zeros(n, F32), np.zeros(n, F32), np.full(n, 4, np.int64)
    for k in (0, 1):
        u = unit_f32(_blocks(orc, seed, pixel, sample, LENS_BLOCK | k))
        for j in (0, 1):
            cx = ((F32(2.0) * u[:, 2 * j]).astype(F32) - F32(1.0)).astype(F32)
            cy = ((F32(2.0) * u[:, 2 * j + 1]).astype(F32) - F32(1.0)).astype(F32)
            inside = ((cx * cx).astype(F32) + (cy * cy).astype(F32)).astype(F32) <= F32(1.0)
            take = inside & (taken == 4)
            x[take], y[take], taken[take] = cx[take], cy[take], 2 * k + j
    return x, y, taken


def camera_rays(orc, vp12, w, h, spp, seed, camera, sample0=0, nsamples=None, rows=None):
    """The rays of samples [sample0, sample0 + nsamples) of a frame of `spp` samples for every pixel of image rows `rows` (default:
    all), in [pixel][sample] order, with their RNG keys.  Returns a namespace: o4, d4 (n, 4), keys (n, 2) uint32 = (pixel,
    sample), npix, n (samples per pixel of the call), and what they were made from: p (the image-plane point), and for the thin
    lens lens_xy (n, 2), taken (n,), o (the lens point relative to cam), F (the point in focus)."""
    vp = np.asarray(vp12, F32)
    orig, eye, vu, vv = (_v4(vp[3 * i:3 * i + 3]) for i in range(4))
    n = spp - sample0 if nsamples is None else nsamples
    rows = list(range(h)) if rows is None else list(rows)
    npix = len(rows) * w
    row = np.repeat(np.repeat(np.array(rows, np.int64), w), n)
    col = np.repeat(np.tile(np.arange(w, dtype=np.int64), len(rows)), n)
    sample = np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), npix)
    pixel = row * w + col
    with np.errstate(all="ignore"):
        vu_delta = (vu * (F32(1.0) / F32(w))).astype(F32)
        vv_delta = (vv * (F32(1.0) / F32(h))).astype(F32)
        if spp != 1:
            u = unit_f32(_blocks(orc, seed, pixel, sample, 0))
            u_off, v_off = u[:, 0], u[:, 1]
        else:
            u_off = v_off = np.full(len(pixel), 0.5, F32)
        vu_frac = (vu_delta[None, :] * (col.astype(F32) + u_off).astype(F32)[:, None]).astype(F32)
        vv_frac = (vv_delta[None, :] * (row.astype(F32) + v_off).astype(F32)[:, None]).astype(F32)
        p = ((orig[None, :] + vu_frac).astype(F32) + vv_frac).astype(F32)
        out = SimpleNamespace(p=p, keys=np.ascontiguousarray(np.stack([pixel, sample], axis=1).astype(np.uint32)), npix=npix, n=n)
        if camera.model == PINHOLE:
            out.o4, out.d4 = p, vunit(vunit((p - eye[None, :]).astype(F32)))
        elif camera.model == ORTHO:
            c = ((orig + (vu * F32(0.5)).astype(F32)).astype(F32) + (vv * F32(0.5)).astype(F32)).astype(F32)
            axis = vunit(vunit((c - eye).astype(F32)[None, :]))
            out.o4, out.d4 = p, np.ascontiguousarray(np.repeat(axis, len(pixel), axis=0))
        elif camera.model == THIN_LENS:
            r, f = F32(camera.lens_radius), F32(camera.focus)
            eu, ev = vunit(vu[None, :])[0], vunit(vv[None, :])[0]
            x, y, taken = lens_samples(orc, seed, pixel, sample)
            o = ((eu[None, :] * (x * r).astype(F32)[:, None]).astype(F32) + (ev[None, :] * (y * r).astype(F32)[:, None]).astype(F32)).astype(F32)
            e = (p - eye[None, :]).astype(F32)
            F = (eye[None, :] + (e * f).astype(F32)).astype(F32)
            k = F32(F32(1.0) - F32(F32(1.0) / f))
            O = (p + (o * k).astype(F32)).astype(F32)
            out.o4, out.d4 = O, vunit(vunit((F - (eye[None, :] + o).astype(F32)).astype(F32)))
            out.lens_xy, out.taken, out.o, out.F = np.stack([x, y], axis=1), taken, o, F
        else:
            raise ValueError("unknown camera model")
    out.o4, out.d4 = np.ascontiguousarray(out.o4, F32), np.ascontiguousarray(out.d4, F32)
    return out


def path_trace(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None):
    """project_ray from explicit rays: the colour of a path of depth `maxdepth` that starts with ray i and has RNG key (pixel[i],
    sample[i]); bounce k draws block k.  trace(o4, d4) -> (tri, t, face) replaces the oracle's closest hits (the modes that are not
    bit-exact are held against the product's own rtmi_trace).  Returns a namespace: color (n, 4), rays (the "Rays" statistic),
    passes (rays per pass), hits0 (tri, t, face of the given rays; None when maxdepth == 0)."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    passes, hits0 = [], None
    if maxdepth == 0:
        return SimpleNamespace(color=color, rays=0, passes=passes, hits0=None)
    rec, kinds, surf = so.triangles()
    norms = rec[:, 3:6].astype(F32)
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
                path = path[:0]
                continue
            point = ((cur_d[go] * t[go, None]).astype(F32) + cur_o[go]).astype(F32)  # Ray::at
            nrm = np.zeros((int(go.sum()), 4), F32)
            nrm[:, :3] = norms[tri[go]]
            back = (face[go] & 1) != 0
            nrm[back] = nrm[back] * F32(-1.0)
            path = path[go]
            rv = random_vec(orc, seed, pixel[path], sample[path], j + 1)
            mo, md = lambertian_ray(point, nrm, rv)
            ro, rd = reflect_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), rv)
            matte = (kind[go] == MATTE)[:, None]
            cur_o = np.ascontiguousarray(np.where(matte, mo, ro).astype(F32))
            cur_d = np.ascontiguousarray(np.where(matte, md, rd).astype(F32))
        for paths_j, col_j, alpha_j in reversed(levels):  # the nested mix_color calls, inside-out
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
    return SimpleNamespace(color=color, rays=sum(passes), passes=passes, hits0=hits0)


def fold(color, npix, n, sample0=0, accum0=None):
    """walk_ray_set's fold continued from accum0 (sample0 > 0) or from 0.f: (accum, image = accum * (1 / (sample0 + n)))"""
    acc = np.zeros((npix, 4), F32) if sample0 == 0 else np.array(accum0, F32).reshape(npix, 4)
    cs = np.asarray(color, F32).reshape(npix, n, 4)
    with np.errstate(all="ignore"):
        for s in range(n):
            acc = (acc + cs[:, s]).astype(F32)
        return acc, (acc * (F32(1.0) / F32(sample0 + n))).astype(F32)


def render(orc, so, vp12, w, h, spp, seed, camera, maxdepth, sample0=0, nsamples=None, tile=None, trace=None, accum0=None, guides=True):
    """Expected buffers of one rtmi_render_camera* call on oracle scene `so`.  Returns a namespace: image, accum (rows, w, 4),
    albedo, normal (rows, w, 4), ids (rows, w) (None without guides), rays, passes, and cr (camera_rays' namespace)."""
    rows = None if tile is None else FR.tile_rows(tile)
    cr = camera_rays(orc, vp12, w, h, spp, seed, camera, sample0, nsamples, rows)
    pt = path_trace(orc, so, cr.o4, cr.d4, cr.keys[:, 0], cr.keys[:, 1], maxdepth, seed, trace)
    acc, img = fold(pt.color, cr.npix, cr.n, sample0, accum0)
    nr = cr.npix // w
    out = SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), rays=pt.rays, passes=pt.passes, cr=cr,
                          albedo=None, normal=None, ids=None)
    if guides:
        hits = pt.hits0
        if hits is None:
            hits = so.trace(cr.o4, cr.d4)[:3] if trace is None else trace(cr.o4, cr.d4)[:3]
        rec, _, surf = so.triangles()
        alb, nrm, ids = FR.features_from_hits(hits[0], hits[1], hits[2], rec, surf, cr.npix, cr.n)
        out.albedo, out.normal, out.ids = alb.reshape(nr, w, 4), nrm.reshape(nr, w, 4), ids.reshape(nr, w)
    return out
