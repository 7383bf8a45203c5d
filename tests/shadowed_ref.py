"""The definition of the shadowed path-trace (rtmi_render_shadowed*, include/rtmi.h) in float32 NumPy, from the oracle as it is:
the whole bounce loop restated pass by pass.  FR.tile_rays makes the renderer's primary rays, Scene.trace the closest hits of
every pass and of the shadow rays, Scene.triangles the normals and surfaces, orc.rng_block the draws, LR.candidates the shadow
ray of a hit (its RNG block moved from 0xC0000000 | 0 to 0xC0000000 | j), OR.from_hits the occlusion rule.  Restated here, every
operation rounded to float32 on all four lanes in the reference's order: random_vec, lambertian_ray, reflect_ray, make_ray,
mix_color and walk_ray_set's fold.  With no light the result must be Scene.render's, bit for bit: tests/test_shadowed_cpu.py pins
the restatement to the oracle that way before anything trusts it.  A plain helper module of tests/test_shadowed_cpu.py and
tests/test_shadowed.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import light_ref as LR
import occluded_ref as OR
from rays_ref import vunit

F32 = np.float32
SOLID, MATTE, REFLECTIVE = 0, 1, 2


def _v4(a3):
    out = np.zeros((a3.shape[0], 4), F32)
    out[:, :3] = a3
    return out


def random_vec(orc, seed, pixel, sample, blk):
    """random_vec (raytrace.rs:188-192) of RNG block `blk` of every (pixel[i], sample[i]): unit((u0 - .5, u1 - .5, u2 - .5, 0))"""
    v = np.zeros((len(pixel), 4), F32)
    for i in range(len(pixel)):
        w = orc.rng_block(int(seed), int(pixel[i]), int(sample[i]), int(blk))
        v[i, :3] = [F32(F32(orc.u32_to_unit_f32(int(w[c]))) - F32(0.5)) for c in range(3)]
    return vunit(v)


def mix_color(c1, c2, a):
    """mix_color (raytrace.rs:299-301): c1 * (1.f - a) + c2 * a"""
    a = np.asarray(a, F32)[:, None]
    return ((c1 * (F32(1.0) - a)).astype(F32) + (c2 * a).astype(F32)).astype(F32)


def lambertian_ray(point, norm, rv):
    """(raytrace.rs:292-297) -> (orig, dir) as make_ray stores them"""
    return (point + (rv * F32(0.001)).astype(F32)).astype(F32), vunit((norm + rv).astype(F32))


def reflect_ray(point, norm, rd, fuzz, rv):
    """(raytrace.rs:278-290) -> (orig, dir) as make_ray stores them: the direction is normalised twice, as the reference does"""
    ddot = np.abs(LR.odot(rd, norm)).astype(F32)
    dir_p = (norm * ddot[:, None]).astype(F32)
    dir_o = (rd + dir_p).astype(F32)
    reflect = (dir_p + dir_o).astype(F32)
    rvf = (rv * np.asarray(fuzz, F32)[:, None]).astype(F32)
    reflect_dir = vunit((reflect + rvf).astype(F32))
    return (point + (reflect_dir * F32(0.001)).astype(F32)).astype(F32), vunit(reflect_dir)


def shadowed_ref(orc, so, w, h, vp12, maxdepth, spp, seed, light=None, len2=0.0, bias=0.005, flags=0, sample0=0, nsamples=None,
                 tile=None, trace=None, occluded=None):
    """Expected image of oracle scene `so` and what it was made from.  light: the corner of the box light, or None: no shadow
    test is made and no bit is ever set (the plain path trace).  trace(o4, d4) -> (tri, t, face) and occluded(o4, d4, tmax) ->
    bytes replace the oracle's closest hits and the rule on them (the not-bit-exact modes are held against the product's own
    rtmi_trace / rtmi_occluded).  Returns a namespace: image (rows, w, 4) = accum * (1 / (sample0 + n)) for sums that start at
    0; accum (rows, w, 4); color (npaths, 4), the sample colours in [pixel][sample] order; passes, one dict per pass with
    rays (the pass's path rays), tested, culled, live, occluded, shadowed (= culled + occluded), refl_shadowed (shadowed hits
    on a Reflective surface); rays (the plain call's "Rays") and nlive (the live shadow rays) over all passes."""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    npaths = npix * n
    color = np.zeros((npaths, 4), F32)
    passes = []
    if maxdepth == 0:
        img = np.zeros((len(rows), w, 4), F32)
        return SimpleNamespace(image=img, accum=img.copy(), color=color, passes=passes, rays=0, nlive=0, npaths=npaths)
    rec, kinds, surf = so.triangles()
    norms = rec[:, 3:6].astype(F32)
    pixel = np.repeat(np.array([r * w + c for r in rows for c in range(w)], np.int64), n)
    sample = np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), npix)
    sky = np.array([FR.SKY[0], FR.SKY[1], FR.SKY[2], 0.0], F32)
    path = np.arange(npaths)
    cur_o, cur_d = o4, d4
    levels = []  # per pass: (paths that pushed a surface, its colour or black (k, 4), its alpha (k,))
    with np.errstate(all="ignore"):
        for j in range(maxdepth):
            st = dict(rays=len(path), tested=0, culled=0, live=0, occluded=0, shadowed=0, refl_shadowed=0)
            passes.append(st)
            if len(path) == 0:
                continue
            if trace is None:
                tri, t, face, _ = so.trace(cur_o, cur_d)
            else:
                tri, t, face = trace(cur_o, cur_d)
            tri, face, t = np.asarray(tri, np.uint32), np.asarray(face, np.uint32), np.asarray(t, F32)
            miss = tri == 0
            edge = ~miss & ((face & 2) != 0)
            surface = ~miss & ~edge
            color[path[miss]] = sky
            color[path[edge]] = 0.0
            # ---- the shadow test of every surface hit: one candidate, RNG block 0xC0000000 | j
            shadowed = np.zeros(len(path), bool)
            if light is not None and surface.any():
                blk = SimpleNamespace(rng_block=lambda s, p, k, b: orc.rng_block(s, p, k, b | j), u32_to_unit_f32=orc.u32_to_unit_f32)
                hit, so_, sd_, r, c = LR.candidates(blk, seed, cur_o, cur_d, np.where(surface, tri, 0), t, face, norms, pixel[path],
                                                    sample[path], 1, light, len2, bias)
                assert np.array_equal(hit, np.nonzero(surface)[0])
                live = c[:, 0] > F32(0.0)
                l_o, l_d, l_r = (np.ascontiguousarray(a[live, 0]) for a in (so_, sd_, r))
                tmax = None if flags & LR.UNBOUNDED else l_r
                if not live.any():
                    occ = np.zeros(0, np.uint8)
                elif occluded is None:
                    l_tri, l_t, _, _ = so.trace(l_o, l_d)
                    occ = OR.from_hits(l_tri, l_t, tmax)
                else:
                    occ = np.asarray(occluded(l_o, l_d, tmax), np.uint8)
                sh = ~live
                sh[live] = occ != 0
                shadowed[hit] = sh
                refl = kinds[tri[hit]] == REFLECTIVE
                st.update(tested=len(hit), culled=int((~live).sum()), live=int(live.sum()), occluded=int((occ != 0).sum()),
                          shadowed=int(sh.sum()), refl_shadowed=int((sh & refl).sum()))
            # ---- color_ray
            kind = np.where(surface, kinds[tri], -1)
            col = _v4(surf[tri, 0:3].astype(F32))
            col[shadowed] = 0.0
            solid = kind == SOLID
            color[path[solid]] = col[solid]
            go = surface & ~solid
            levels.append((path[go], col[go], surf[tri[go], 3].astype(F32)))
            if maxdepth - j - 1 == 0:  # project_ray at depth 0: black
                color[path[go]] = 0.0
                path = path[:0]
                continue
            point = ((cur_d[go] * t[go, None]).astype(F32) + cur_o[go]).astype(F32)  # Ray::at
            nrm = _v4(norms[tri[go]])
            back = (face[go] & 1) != 0
            nrm[back] = nrm[back] * F32(-1.0)
            path = path[go]
            rv = random_vec(orc, seed, pixel[path], sample[path], j + 1)
            mo, md = lambertian_ray(point, nrm, rv)
            ro, rd = reflect_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), rv)
            matte = (kind[go] == MATTE)[:, None]
            cur_o = np.ascontiguousarray(np.where(matte, mo, ro).astype(F32))
            cur_d = np.ascontiguousarray(np.where(matte, md, rd).astype(F32))
        # ---- the nested mix_color calls, inside-out
        for paths_j, col_j, alpha_j in reversed(levels):
            color[paths_j] = mix_color(col_j, color[paths_j], alpha_j)
        # ---- walk_ray_set's fold
        acc = np.zeros((npix, 4), F32)
        cs = color.reshape(npix, n, 4)
        for s in range(n):
            acc = (acc + cs[:, s]).astype(F32)
        img = (acc * (F32(1.0) / F32(sample0 + n))).astype(F32)
    return SimpleNamespace(image=img.reshape(len(rows), w, 4), accum=acc.reshape(len(rows), w, 4), color=color, passes=passes,
                           rays=sum(p["rays"] for p in passes), nlive=sum(p["live"] for p in passes), npaths=npaths)


# ---------------------------------------------------------------- scenes and lights the two test files share
CAMERA = (2.0, 0.0, 0.0)            # the canonical camera, looking down +z
BEHIND_CAMERA = (2.0, 0.0, -3.0)    # a point light behind it on its axis
BEHIND_WALL = (2.0, 0.0, 30.0)      # ... and one behind the wall


def recipe_wall(color=(200, 200, 200), alpha=0.5):
    """One Matte wall of two triangles in front of the canonical camera, edge 0, slightly tilted (z = 6 + 0.05 x + 0.03 y: no
    ray of the view is parallel to it and no hit time is a round number), in a small octree.  It covers the whole view."""
    def r(api):
        s = api.scene()
        m = api.matte(color, alpha)
        z = lambda x, y: 6.0 + 0.05 * x + 0.03 * y
        a, b, c, d = ([-10.0, -12.0], [14.0, -12.0], [14.0, 12.0], [-10.0, 12.0])
        p = lambda q: [q[0], q[1], z(*q)]
        api.add_triangle(s, np.array([p(a), p(b), p(c)], F32), m, 0.0)
        api.add_triangle(s, np.array([p(a), p(c), p(d)], F32), m, 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 6.0], 16.0, 3, 1)
        return s
    return r


def recipe_corridor():
    """Two huge Reflective walls without scattering facing each other (z = +-6, tilted by a few 1e-4), the canonical camera
    between them: every path bounces between them until its depth is exhausted, so a depth of 32 fills every bit of a path's
    shadow mask.  CORRIDOR_LIGHT is a box that straddles the far wall: about half of its samples lie behind it."""
    def r(api):
        s = api.scene()
        m = api.reflective(0.0, (220, 200, 180), 0.3)
        for zc, flip in ((6.0, 1.0), (-6.0, -1.0)):
            z = lambda x, y: zc + flip * (0.0001 * x + 0.0002 * y)
            a, b, c, d = ([-1000.0, -1001.0], [1004.0, -1001.0], [1004.0, 1001.0], [-1000.0, 1001.0])
            p = lambda q: [q[0], q[1], z(*q)]
            api.add_triangle(s, np.array([p(a), p(b), p(c)], F32), m, 0.0)
            api.add_triangle(s, np.array([p(a), p(c), p(d)], F32), m, 0.0)
        s.populate_triangle_numbers()
        s.build_bounding_box([2.0, 0.0, 0.0], 1024.0, 2, 1)
        return s
    return r


CORRIDOR_LIGHT, CORRIDOR_LEN2 = (1.0, 2.0, 4.0), 4.0


# ---------------------------------------------------------------- the refused calls (no GPU is touched: every call fails first)
def check_refusals():
    """Every RTMI_ERR_INVALID case of rtmi_render_shadowed* in include/rtmi.h, for both variants, through a dangling scene handle
    that a failing check never dereferences; stats must come back cleared.  Raises AssertionError."""
    import ctypes as C
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    INVALID, OK = 1, 0
    bogus, acc, out = C.c_void_p(0x10), 0x100000, 0x200000
    nan, inf = float("nan"), float("inf")

    class Vp(C.Structure):
        _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                    ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]

    def vp(w=8, h=8, spp=4, maxdepth=5):
        v = Vp()
        v.width, v.height, v.maxdepth, v.samples_per_pixel = w, h, maxdepth, spp
        return v

    def both(scene=bogus, view="dflt", tile=(0, 8, 8, 0), sample0=0, nsamples=4, light="dflt", accum=acc, outp=out, orig=None, variants=(True, False), **fields):
        v = vp() if view == "dflt" else view
        a = None
        if light == "dflt":
            a = _ffi.Light()
            L.rtmi_light_defaults(C.byref(a))
            a.rays = 1
            for k, x in fields.items():
                setattr(a, k, x)
            if orig is not None:
                a.orig[0], a.orig[1], a.orig[2] = orig
        res = []
        for dev in variants:
            st = _ffi.Stats()
            st.rays = 123
            vp_p, li_p = (C.byref(v) if v is not None else None), (C.byref(a) if a is not None else None)
            ap, op = (C.c_void_p(accum) if accum else None), (C.c_void_p(outp) if outp else None)
            if dev:
                t = _ffi.Tile(*tile) if tile is not None else None
                rc = L.rtmi_render_shadowed_device(scene, vp_p, 7, C.byref(t) if t is not None else None, sample0, nsamples, li_p, ap, op,
                                                   None, C.byref(st))
            else:
                row0, nrows = (tile[0], tile[1]) if tile is not None else (0, 8)
                rc = L.rtmi_render_shadowed(scene, vp_p, 7, row0, nrows, sample0, nsamples, li_p, ap, op, C.byref(st))
            res.append((rc, L.rtmi_last_error(), st.rays))
        return res

    def refused(word, **kw):
        for rc, msg, rays in both(**kw):
            assert rc == INVALID and word in msg and rays == 0, (kw, rc, msg, rays)

    # rtmi_render_samples[_device]'s checks
    for kw in (dict(scene=None), dict(view=None), dict(accum=0)):
        refused(b"NULL", **kw)
    refused(b"different buffers", accum=acc, outp=acc)
    refused(b"nsamples", nsamples=0)
    refused(b"sample0 + nsamples", sample0=3, nsamples=2)
    refused(b"sample0 + nsamples", sample0=0xFFFFFFFF, nsamples=2)
    refused(b"samples_per_pixel", view=vp(spp=0))
    rc, msg, rays = both(view=vp(w=0), variants=(True,))[0]  # (the host variant, like rtmi_render_samples, has nothing to do for zero pixels)
    assert rc == INVALID and b"empty viewport" in msg and rays == 0
    refused(b"outside", tile=(4, 8, 8, 0))
    refused(b"outside", tile=(0, 9, 9, 0))
    rc, msg, rays = both(tile=None, variants=(True,))[0]
    assert rc == INVALID and b"tile" in msg and rays == 0
    for tile, word in (((0, 4, 0, 0), b"stripe_rows"), ((0, 8, 2, 1), b"overlap"), ((0, 8, 2, 4), b"outside")):
        rc, msg, rays = both(tile=tile, variants=(True,))[0]  # (what the host variant cannot express)
        assert rc == INVALID and word in msg and rays == 0, (tile, msg)
    for rc, msg, rays in both(view=vp(maxdepth=33)):
        assert rc == 3 and b"maxdepth" in msg and rays == 0  # RTMI_ERR_UNSUPPORTED, as a plain render
    # rtmi_render_light*'s parameter checks
    refused(b"NULL", light=None)
    for fields in (dict(rays=0), dict(rays=257), dict(rays=1 << 31), dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(len2=nan),
                   dict(len2=-1.0), dict(len2=inf), dict(len2=-inf), dict(bias=nan), dict(bias=inf), dict(bias=-inf),
                   dict(orig=(nan, 0.0, 0.0)), dict(orig=(0.0, inf, 0.0)), dict(orig=(0.0, 0.0, -inf))):
        refused(list(fields)[0].encode(), **fields)
    # ... and the one this call adds
    for k in (2, 4, 256):
        refused(b"rays must be 1", rays=k)
    # valid edge parameters reach the next check; an empty tile is fine and touches nothing
    for fields in (dict(len2=0.0), dict(len2=-0.0), dict(len2=1e30), dict(flags=1), dict(bias=0.0), dict(bias=-0.5), dict(outp=0),
                   dict(orig=(-3e30, 6.0, 1.0))):
        refused(b"sample0 + nsamples", nsamples=5, **fields)
    for tile in ((0, 0, 1, 0), (100, 0, 0, 0)):
        for rc, _, rays in both(tile=tile):
            assert rc == OK and rays == 0
