"""The definition of emissive triangles sampled at matte hits (rtmi_scene_set_emitters, rtmi_render_emissive*,
rtmi_scene_get_emitter_sampler; include/rtmi.h "EMISSIVE TRIANGLES") in NumPy: the lamps' tables in integers (`lamp_tables`), the
density `pe`, the sampled point (`sample_lamp`) with one NumPy operation rounded to float32 per operation of the header's listing,
and the whole pass (`path_trace`, `render`) over envlight_ref's path loop: the oracle's closest hits (Scene.trace) for the paths and
for the first hit of every live shadow ray.  With nee=False the loop is the plain render's (lit_ref.path_trace without lights pins
that in tests/test_emissive_cpu.py).  A plain helper module of tests/test_emissive_cpu.py and tests/test_emissive.py."""
from types import SimpleNamespace

import numpy as np

import env_ref as ER
import envlight_ref as EL
import features_ref as FR
from camera_ref import fold
from glass_ref import keys_of
from rays_ref import vunit
from shadowed_ref import MATTE, SOLID, lambertian_ray, mix_color, reflect_ray

F32 = np.float32
U32, U64 = np.uint32, np.uint64
EMISSIVE_BLOCK = 0xC0040000
QSCALE = EL.QSCALE
NO_SAMPLE = F32(-1.0)


def _v4(a3):
    a3 = np.asarray(a3, F32).reshape(-1, 3)
    out = np.zeros((a3.shape[0], 4), F32)
    out[:, :3] = a3
    return out


# ---------------------------------------------------------------- the tables
def lamp_tables(corners, norms, radiance):
    """The tables of L lamps from their corners (L, 3, 3), their records' normals (L, 3) and their radiance (L, 3): a namespace n,
    c0, e1, e2, nrm, rad (L, 4 each), A, w (L,), q (L,) uint32, cum (L,) uint64, total (int)"""
    c = np.asarray(corners, F32).reshape(-1, 3, 3)
    L = c.shape[0]
    with np.errstate(all="ignore"):
        c0, e1, e2 = _v4(c[:, 0]), _v4((c[:, 1] - c[:, 0]).astype(F32)), _v4((c[:, 2] - c[:, 0]).astype(F32))
        m = lambda a, b: (a * b).astype(F32)
        x = np.zeros((L, 4), F32)
        x[:, 0] = (m(e1[:, 1], e2[:, 2]) - m(e1[:, 2], e2[:, 1])).astype(F32)
        x[:, 1] = (m(e1[:, 2], e2[:, 0]) - m(e1[:, 0], e2[:, 2])).astype(F32)
        x[:, 2] = (m(e1[:, 0], e2[:, 1]) - m(e1[:, 1], e2[:, 0])).astype(F32)
        A = (F32(0.5) * np.sqrt(ER.vdot(x, x)).astype(F32)).astype(F32)
        rad = _v4(radiance)
        lum = ((rad[:, 0] + rad[:, 1]).astype(F32) + rad[:, 2]).astype(F32)
        w = (A * lum).astype(F32)
        w = np.where((w > F32(0.0)) & np.isfinite(w), w, F32(0.0)).astype(F32)
        wmax = F32(w.max()) if L else F32(0.0)
        if wmax == F32(0.0):
            q = np.ones(L, U32)
        else:
            s = (w * (F32(QSCALE) / wmax).astype(F32)).astype(F32)
            s = np.where(~(s >= F32(0.0)), F32(0.0), np.where(s > F32(QSCALE), F32(QSCALE), s)).astype(F32)
            q = (s.astype(U32) + U32(1)).astype(U32)
    cum = np.cumsum(q.astype(U64), dtype=U64)
    return SimpleNamespace(n=L, c0=c0, e1=e1, e2=e2, nrm=_v4(norms), rad=rad, A=A, w=w, q=q, cum=cum, total=int(cum[-1]) if L else 0)


def tables_of(so, lamps):
    """The tables of an oracle scene whose lamps are the triangles `lamps` (numbers, any order: the table is in triangle order), with
    tri (L,) the lamps' triangles and idx (ntris,) the lamp number of every triangle (1-based, 0 = not a lamp)"""
    rec, kinds, surf = so.triangles()
    tri = np.array(sorted(int(k) for k in lamps), np.int64)
    assert len(tri) and tri.min() >= 1 and (kinds[tri] == SOLID).all()
    tb = lamp_tables(rec[tri, 20:29].reshape(-1, 3, 3), rec[tri, 3:6], surf[tri, 0:3])
    tb.tri = tri
    tb.idx = np.zeros(len(kinds), U32)
    tb.idx[tri] = np.arange(1, len(tri) + 1, dtype=U32)
    return tb


def records(tb):
    """The (L, 5, 4) records rtmi_scene_get_emitter_sampler copies back: (c0, A), (e1, w), (e2, 0), (n, 0), (radiance, 0)"""
    r = np.zeros((tb.n, 5, 4), F32)
    r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = tb.c0, tb.e1, tb.e2, tb.nrm, tb.rad
    r[:, 0, 3], r[:, 1, 3] = tb.A, tb.w
    return r


def first_above(cum, T):
    """The kernel's search: the first k with cum[k] > T, for T < cum[-1]"""
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if int(cum[mid]) > T:
            hi = mid
        else:
            lo = mid + 1
    return lo


def table_cases():
    """name -> (corners (L, 3, 3), norms (L, 3), radiance (L, 3)): the lamp counts 1, 63, 64, 65, 257 and 1000 with random triangles
    and HDR radiances; every case of more than one lamp holds a zero-area, an infinite-radiance and an all-black lamp"""
    cases = {}
    for L in (1, 63, 64, 65, 257, 1000):
        rng = np.random.default_rng(7 + L)
        c = (rng.random((L, 3, 3)) * 4.0 - 2.0).astype(F32)
        n = rng.standard_normal((L, 3)).astype(F32)
        rad = (rng.random((L, 3)) ** 4 * 100.0).astype(F32)
        if L > 1:
            c[L // 2, 2] = c[L // 2, 1]          # zero area
            rad[L // 3] = (np.inf, 1.0, 1.0)     # infinite radiance
            rad[L - 1] = 0.0                     # all black
            rad[0] = (np.nan, 1.0, 1.0)
        cases[f"lamps{L}"] = (c, n, rad)
    cases["all black"] = ((np.random.default_rng(3).random((5, 3, 3))).astype(F32), np.ones((5, 3), F32), np.zeros((5, 3), F32))
    return cases


# ---------------------------------------------------------------- the density and the drawn point
def pe(tb, e, x2, d4):
    """pe(e, x2, dir) for lamp numbers e (1-based, (m,)), squared distances x2 (m,) and unit directions d4 (m, 4): (m,) float32"""
    k = np.asarray(e, np.int64) - 1
    with np.errstate(all="ignore"):
        ndot = np.abs(ER.vdot(tb.nrm[k], np.asarray(d4, F32).reshape(-1, 4))).astype(F32)
        sel = (tb.q[k].astype(F32) / F32(U64(tb.total))).astype(F32)
        return ((((sel / tb.A[k]).astype(F32)) * np.asarray(x2, F32)).astype(F32) / ndot).astype(F32)


def sample_lamp(tb, w):
    """The lamp (1-based) and the point y (m, 4) of the words w (m, 4) of a block"""
    x = (np.asarray(w[:, 0], U64) << U64(32)) | np.asarray(w[:, 1], U64)
    T = np.array([(int(v) * tb.total) >> 64 for v in x], U64)
    k = np.searchsorted(tb.cum, T, side="right")
    with np.errstate(all="ignore"):
        a, b = EL.unit_f32(w[:, 2]), EL.unit_f32(w[:, 3])
        over = (a + b).astype(F32) > F32(1.0)
        a, b = np.where(over, (F32(1.0) - a).astype(F32), a).astype(F32), np.where(over, (F32(1.0) - b).astype(F32), b).astype(F32)
        y = ((tb.c0[k] + (tb.e1[k] * a[:, None]).astype(F32)).astype(F32) + (tb.e2[k] * b[:, None]).astype(F32)).astype(F32)
    return (k + 1).astype(np.int64), y


# ---------------------------------------------------------------- the pass
def path_trace(so, o4, d4, pixel, sample, maxdepth, seed, lamps, env=None, nee=True, trace=None):
    """The sample colours of rtmi_render_emissive* (nee) or of the plain render of the same scene (not nee) for the primary rays
    (o4, d4) with keys (pixel, sample).  Returns a namespace: color (m, 4), rays (the plain "Rays"), passes, and per pass candidates,
    culled, nlive (the live shadow rays), lost, visible, visible_paths (the paths whose candidate counted); wsum (wA + wB of every shadow ray that counted, evaluated on its own hit
    record both ways); hits0."""
    o4, d4 = np.asarray(o4, F32).reshape(-1, 4), np.asarray(d4, F32).reshape(-1, 4)
    pixel, sample = np.asarray(pixel, np.int64), np.asarray(sample, np.int64)
    npaths = o4.shape[0]
    color = np.zeros((npaths, 4), F32)
    st = SimpleNamespace(color=color, rays=0, passes=[], nlive=[], candidates=[], culled=[], lost=[], visible=[], visible_paths=[], wsum=[], hits0=None)
    if maxdepth == 0:
        return st
    tb = tables_of(so, lamps) if nee else None
    trace = so.trace if trace is None else trace
    rec, kinds, surf = so.triangles()
    norms = rec[:, 3:6].astype(F32)
    sky = np.array([FR.SKY[0], FR.SKY[1], FR.SKY[2], 0.0], F32)
    path = np.arange(npaths)
    cur_o, cur_d = o4, d4
    wp = np.full(npaths, NO_SAMPLE, F32)
    levels = []  # per pass: (paths that pushed a surface, its colour (k, 4), its alpha (k,), its direct light (k, 4))
    with np.errstate(all="ignore"):
        for j in range(maxdepth):
            st.passes.append(len(path))
            for a in (st.nlive, st.candidates, st.culled, st.lost, st.visible):
                a.append(0)
            st.visible_paths.append(np.zeros(0, np.int64))
            if len(path) == 0:
                continue
            tri, t, face = trace(cur_o, cur_d)[:3]
            tri, face, t = np.asarray(tri, U32), np.asarray(face, U32), np.asarray(t, F32)
            if j == 0:
                st.hits0 = (tri, t, face)
            miss = tri == 0
            edge = ~miss & ((face & 2) != 0)
            surface = ~miss & ~edge
            if miss.any():
                color[path[miss]] = sky if env is None else ER.lookup(env.table, env.frame, cur_d[miss])
            color[path[edge]] = 0.0
            kind = np.where(surface, kinds[tri], -1)
            col = np.zeros((len(path), 4), F32)
            col[:, :3] = surf[tri, 0:3].astype(F32)
            solid = kind == SOLID
            color[path[solid]] = col[solid]
            if nee and j > 0:  # strategy A: a bounce that ends on a lamp, weighted against the sample that stood beside it
                onl = np.nonzero(solid & (tb.idx[tri] != 0) & (wp[path] >= F32(0.0)))[0]
                if len(onl):
                    pbp = wp[path[onl]]
                    pev = pe(tb, tb.idx[tri[onl]], (t[onl] * t[onl]).astype(F32), cur_d[onl])
                    wA = (pbp / (pbp + pev).astype(F32)).astype(F32)
                    color[path[onl]] = (col[onl] * wA[:, None]).astype(F32)
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
            matte = kind[go] == MATTE
            rv = EL.random_vec(EL.rng_blocks(seed, pixel[path], sample[path], j + 1))
            mo, md = lambertian_ray(point, nrm, rv)
            ro, rd = reflect_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), rv)
            if nee:
                # ---- k_emissive_rays: one candidate per bouncing Matte hit, RNG block 0xC0040000 | j
                mi = np.nonzero(matte)[0]
                st.candidates[-1] = len(mi)
                if len(mi):
                    w = EL.rng_blocks(seed, pixel[path[mi]], sample[path[mi]], EMISSIVE_BLOCK | j)
                    e, y = sample_lamp(tb, w)
                    n_m = nrm[mi]
                    dv = (y - point[mi]).astype(F32)
                    d2 = ER.vdot(dv, dv)
                    omega = vunit(dv)
                    s_m = EL.bounce_s(n_m, omega)  # the random_vec whose bounce is omega: the shadow ray starts where that bounce would
                    so_ = (point[mi] + (s_m * F32(0.001)).astype(F32)).astype(F32)
                    cos = ER.vdot(n_m, omega)
                    ndot = np.abs(ER.vdot(tb.nrm[e - 1], omega)).astype(F32)
                    rad = tb.rad[e - 1]
                    live = (cos > F32(0.0)) & (ndot > F32(0.0)) & ((rad[:, 0] != 0) | (rad[:, 1] != 0) | (rad[:, 2] != 0))
                    st.culled[-1] = int((~((cos > F32(0.0)) & (ndot > F32(0.0)))).sum())
                    st.nlive[-1] = int(live.sum())
                    if live.any():
                        lv = np.nonzero(live)[0]
                        l_tri, l_t, l_face = trace(np.ascontiguousarray(so_[lv]), np.ascontiguousarray(omega[lv]))[:3]
                        l_tri, l_face, l_t = np.asarray(l_tri, np.int64), np.asarray(l_face, U32), np.asarray(l_t, F32)
                        hit = (l_tri == tb.tri[e[lv] - 1]) & ((l_face & 2) == 0)
                        st.lost[-1], st.visible[-1] = int((~hit).sum()), int(hit.sum())
                        k = lv[hit]
                        st.visible_paths[-1] = path[mi[k]]
                        pbv = EL.pb(n_m[k], omega[k], s_m[k])
                        pev = pe(tb, e[k], (l_t[hit] * l_t[hit]).astype(F32), omega[k])
                        pet = pe(tb, e[k], d2[k], omega[k])
                        wB = (pev / (pbv + pev).astype(F32)).astype(F32)
                        direct[mi[k]] = (rad[k] * ((pbv / pet).astype(F32) * wB).astype(F32)[:, None]).astype(F32)
                        st.wsum.append((wB + (pbv / (pbv + pev).astype(F32)).astype(F32)).astype(F32))
                # ---- the bounce's own pdf, for the lamp its ray may end on
                wpn = np.full(len(path), NO_SAMPLE, F32)
                if len(mi):
                    wpn[mi] = EL.pb(nrm[mi], md[mi], rv[mi])
                wp[path] = wpn
            cur_o = np.ascontiguousarray(np.where(matte[:, None], mo, ro).astype(F32))
            cur_d = np.ascontiguousarray(np.where(matte[:, None], md, rd).astype(F32))
        for paths_j, col_j, alpha_j, direct_j in reversed(levels):  # the nested mix_color calls, inside-out
            inner = (color[paths_j] + direct_j).astype(F32) if nee else color[paths_j]
            color[paths_j] = mix_color(col_j, inner, alpha_j)
    st.rays = sum(st.passes)
    return st


def render(orc, so, vp12, w, h, spp, seed, maxdepth, lamps, env=None, sample0=0, nsamples=None, tile=None, accum0=None, nee=True, trace=None):
    """The expected buffers of one rtmi_render_emissive* call (frame, progressive pass or tile): image, accum (rows, w, 4), color,
    rays (the plain rays), nlive (the live shadow rays), pt (path_trace's namespace)"""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    pixel, sample = keys_of(w, rows, n, sample0)
    pt = path_trace(so, o4, d4, pixel, sample, maxdepth, seed, lamps, env, nee, trace)
    acc, img = fold(pt.color, npix, n, sample0, accum0)
    nr = npix // w
    return SimpleNamespace(image=img.reshape(nr, w, 4), accum=acc.reshape(nr, w, 4), color=pt.color, rays=pt.rays, nlive=sum(pt.nlive),
                           passes=pt.passes, pt=pt, o4=o4, d4=d4, pixel=pixel, sample=sample, n=n, npix=npix)


def block_ids(maxdepth=32, nlights=4):
    """Every RNG block a path may draw under one key in rtmi_render_lit*, rtmi_render_rays_lit*, rtmi_bake_lit* (DESIGN.md 4.29's list)
    and here: name -> block id"""
    ids = {}
    for j in range(maxdepth + 1):
        ids[f"path {j}"] = j
    for j in range(maxdepth):
        for l in range(nlights):
            ids[f"lit {l} {j}"] = 0xC0000000 | (l << 16) | j
        ids[f"emissive {j}"] = EMISSIVE_BLOCK | j
    for l in range(nlights):
        ids[f"bake lit {l}"] = 0xC000FFFF | (l << 16)
    return ids


# ---------------------------------------------------------------- the invalid calls (no GPU is touched: every call fails first)
def check_invalid_arguments():
    """Every argument refusal of rtmi_render_emissive* in include/rtmi.h, for both variants, through a dangling scene handle that a
    failing check never dereferences; stats must come back cleared.  Raises AssertionError."""
    import ctypes as C
    from rust_raytrace_amd import _ffi
    L = _ffi.lib()
    INVALID, OK = 1, 0
    bogus, acc, out = C.c_void_p(0x10), 0x100000, 0x200000

    class Vp(C.Structure):
        _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("orig", C.c_float * 3), ("cam", C.c_float * 3), ("vu", C.c_float * 3),
                    ("vv", C.c_float * 3), ("maxdepth", C.c_uint32), ("samples_per_pixel", C.c_uint32)]

    def vp(w=8, h=8, spp=4, maxdepth=4):
        v = Vp()
        v.width, v.height, v.maxdepth, v.samples_per_pixel = w, h, maxdepth, spp
        return v

    def both(scene=bogus, view="dflt", tile=(0, 8, 8, 0), sample0=0, nsamples=4, accum=acc, outp=out, variants=(True, False)):
        v = vp() if view == "dflt" else view
        res = []
        for dev in variants:
            st = _ffi.Stats()
            st.rays = 123
            vp_p = C.byref(v) if v is not None else None
            ap, op = (C.c_void_p(accum) if accum else None), (C.c_void_p(outp) if outp else None)
            if dev:
                t = _ffi.Tile(*tile) if tile is not None else None
                rc = L.rtmi_render_emissive_device(scene, vp_p, 7, C.byref(t) if t is not None else None, sample0, nsamples, ap, op, None,
                                                   C.byref(st))
            else:
                row0, nrows = (tile[0], tile[1]) if tile is not None else (0, 8)
                rc = L.rtmi_render_emissive(scene, vp_p, 7, row0, nrows, sample0, nsamples, ap, op, C.byref(st))
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
    rc, msg, rays = both(view=vp(w=0), variants=(True,))[0]  # (the host variant has nothing to do for zero pixels)
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
    # a valid edge argument reaches the next check; an empty tile is fine and touches nothing
    refused(b"sample0 + nsamples", nsamples=5, outp=0)
    for tile in ((0, 0, 1, 0), (100, 0, 0, 0)):
        for rc, _, rays in both(tile=tile):
            assert rc == OK and rays == 0
    # the setter's own argument errors, likewise before the scene is used
    assert L.rtmi_scene_set_emitters(None, None, None, 0) == INVALID and b"NULL" in L.rtmi_last_error()
    n = C.c_uint32(5)
    assert L.rtmi_scene_get_emitter_sampler(None, None, None, None, None, None, C.byref(n)) == INVALID
