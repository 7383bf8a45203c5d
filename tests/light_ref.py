"""The definition of the direct-light buffer (rtmi_render_light*, include/rtmi.h) in float32 NumPy, from the oracle as it is:
FR.tile_rays makes the renderer's primary rays, Scene.trace their closest hits and the shadow rays' closest hits,
Scene.triangles the normals, orc.rng_block / orc.u32_to_unit_f32 the four draws of every light sample, OR.from_hits the
occlusion rule.  Every operation is rounded to float32 in the order the header states, on all four lanes.  A plain helper
module of tests/test_light_cpu.py and tests/test_light.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import occluded_ref as OR

F32 = np.float32
LIGHT_BLOCK = 0xC0000000  # RNG block of light sample k: LIGHT_BLOCK | k
UNBOUNDED = 1             # RTMI_LIGHT_UNBOUNDED


def odot(a, b):
    """(..., 4) x (..., 4) -> (((0 + x x) + y y) + z z) + w w, as Vec3::dot (raytrace.rs:65-77)"""
    acc = F32(0.0) + a[..., 0] * b[..., 0]
    for c in (1, 2, 3):
        acc = acc + a[..., c] * b[..., c]
    return acc.astype(F32)


def uniforms(orc, seed, pixel, sample, K):
    """The four uniforms of RNG blocks LIGHT_BLOCK | k, k < K, of every (pixel[i], sample[i]): (n, K, 4) float32"""
    n = len(pixel)
    u = np.zeros((n, K, 4), F32)
    for i in range(n):
        for k in range(K):
            w = orc.rng_block(int(seed), int(pixel[i]), int(sample[i]), LIGHT_BLOCK | k)
            u[i, k] = [F32(orc.u32_to_unit_f32(int(w[c]))) for c in range(4)]
    return u


def candidates(orc, seed, o4, d4, tri, t, face, norm, pixel, sample, K, orig, len2, bias):
    """The K candidate shadow rays of every path that hit: (index of the paths that hit (nh,), o (nh, K, 4), dir (nh, K, 4),
    r (nh, K), c (nh, K)).  A candidate is live iff c > 0."""
    hit = np.nonzero(np.asarray(tri) != 0)[0]
    nh = len(hit)
    with np.errstate(all="ignore"):
        point = ((d4[hit] * np.asarray(t, F32)[hit, None]).astype(F32) + o4[hit]).astype(F32)
        n4 = np.zeros((nh, 4), F32)
        n4[:, :3] = norm[np.asarray(tri)[hit]]
        back = (np.asarray(face)[hit] & 1) != 0
        n4[back] = n4[back] * F32(-1.0)
        u = uniforms(orc, seed, pixel[hit], sample[hit], K)
        adj = np.zeros((nh, K, 4), F32)
        adj[..., :3] = np.asarray(orig, F32)[None, None, :] + (u[..., :3] * F32(len2)).astype(F32)
        v = (adj - point[:, None, :]).astype(F32)
        r = np.sqrt(odot(v, v)).astype(F32)
        dirs = (v * (F32(1.0) / r)[..., None]).astype(F32)
        smudge = (F32(bias) * (u[..., 3] + F32(1.0))).astype(F32)
        o = (point[:, None, :] + (n4[:, None, :] * smudge[..., None]).astype(F32)).astype(F32)
        c = odot(np.broadcast_to(n4[:, None, :], dirs.shape), dirs)
    return hit, o, dirs, r, c


def resolve(tri, live, occ, c, npix, n, K):
    """(shadow, irradiance) per pixel.  tri: the primaries' hit indices ([pixel][sample]); live, c: (nh, K) of the paths that
    hit, in path order; occ: the answers of the live rays in (path, k) order."""
    hit = np.nonzero(np.asarray(tri).reshape(-1) != 0)[0]
    vis = np.ones((npix * n, K), bool)       # a miss: K visible rays
    lit = np.zeros((npix * n, K), bool)      # live and not occluded: contributes c
    cc = np.zeros((npix * n, K), F32)
    clear = np.zeros(live.shape, bool)
    clear[live] = np.asarray(occ) == 0
    vis[hit] = clear
    lit[hit] = clear
    cc[hit] = c
    vis, lit, cc = (a.reshape(npix, n * K) for a in (vis, lit, cc))
    inv = F32(1.0) / F32(n * K)
    shadow = (vis.sum(axis=1).astype(F32) * inv).astype(F32)
    acc = np.zeros(npix, F32)
    with np.errstate(all="ignore"):
        for e in range(n * K):  # sample order, then k order
            acc = np.where(lit[:, e], (acc + cc[:, e]).astype(F32), acc)
        irradiance = (acc * inv).astype(F32)
    return shadow, irradiance


def light_ref(orc, so, w, h, vp12, spp, seed, K, orig, len2=0.0, bias=0.005, flags=0, sample0=0, nsamples=None, tile=None,
              trace=None, occluded=None):
    """Expected planes of oracle scene `so` and everything they were made from.  trace(o4, d4) -> (tri, t, face) and
    occluded(o4, d4, tmax) -> bytes replace the oracle's closest hits and the rule on them (the not-bit-exact modes are held
    against the product's own rtmi_trace / rtmi_occluded).  Returns a namespace: shadow, irradiance (rows, w); o4 / d4 / tmax /
    c (the live rays, path-major, k fastest; tmax None when unbounded) and r (their distances); occ; ncand, nlive, nculled;
    nhit (samples that hit), npaths; dirs (nh, K, 4) of all candidates; cn_primary / cn_light (the oracle's counters for both
    sets; None with a custom trace); l_tri / l_t (the live rays' closest hits, likewise)."""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    cn_primary = cn_light = l_tri = l_t = None
    if trace is None:
        tri, t, face, cn_primary = so.trace(o4, d4)
    else:
        tri, t, face = trace(o4, d4)
    rec, _, _ = so.triangles()
    pixel = np.repeat(np.array([r * w + c for r in rows for c in range(w)], np.int64), n)
    sample = np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), npix)
    hit, o, dirs, r, c = candidates(orc, seed, o4, d4, tri, t, face, rec[:, 3:6].astype(F32), pixel, sample, K, orig, len2, bias)
    with np.errstate(invalid="ignore"):
        live = c > F32(0.0)
    l_o, l_d = np.ascontiguousarray(o[live]), np.ascontiguousarray(dirs[live])
    l_r, l_c = np.ascontiguousarray(r[live]), np.ascontiguousarray(c[live])
    tmax = None if flags & UNBOUNDED else l_r
    nlive = int(live.sum())
    if occluded is None:
        if nlive:
            l_tri, l_t, _, cn_light = so.trace(l_o, l_d)
        else:
            l_tri, l_t, cn_light = np.zeros(0, np.uint32), np.zeros(0, F32), dict.fromkeys(orc.COUNTER_NAMES, 0)
        occ = OR.from_hits(l_tri, l_t, tmax)
    else:
        occ = np.asarray(occluded(l_o, l_d, tmax), np.uint8) if nlive else np.zeros(0, np.uint8)
    shadow, irradiance = resolve(tri, live, occ, c, npix, n, K)
    return SimpleNamespace(shadow=shadow.reshape(len(rows), w), irradiance=irradiance.reshape(len(rows), w), o4=l_o, d4=l_d, tmax=tmax,
                           r=l_r, c=l_c, occ=occ, ncand=len(hit) * K, nlive=nlive, nculled=len(hit) * K - nlive,
                           nhit=int((np.asarray(tri) != 0).sum()), npaths=npix * n, dirs=dirs, tri=np.asarray(tri),
                           cn_primary=cn_primary, cn_light=cn_light, l_tri=l_tri, l_t=l_t)
