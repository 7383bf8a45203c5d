"""The definition of the ambient-occlusion buffer (rtmi_render_ao*, include/rtmi.h) in float32 NumPy, from the oracle as it is:
orc.primary_rays makes the renderer's primary rays, Scene.trace their closest hits and the AO rays' closest hits,
Scene.triangles the normals, orc.rng_block / orc.u32_to_unit_f32 the random vectors.  Every operation is rounded to float32 in
the order the header states, on all four lanes; unit(v) = v * (1 / sqrt(ordered dot)).  A plain helper module of
tests/test_ao_cpu.py and tests/test_ao.py."""
from types import SimpleNamespace

import numpy as np

import features_ref as FR
import occluded_ref as OR

F32 = np.float32
AO_BLOCK = 0x80000000  # RNG block of AO ray k: AO_BLOCK | k


def vunit(v):
    """(n, 4) float32 -> v * (1 / sqrt((((0 + x x) + y y) + z z) + w w)), as Vec3::unit (raytrace.rs:93-96)"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        l2 = F32(0.0) + v[:, 0] * v[:, 0]
        for c in (1, 2, 3):
            l2 = l2 + v[:, c] * v[:, c]
        inv = F32(1.0) / np.sqrt(l2)
        return (v * inv[:, None]).astype(F32)


def random_vecs(orc, seed, pixel, sample, K):
    """random_vec (raytrace.rs:188-192) of RNG blocks AO_BLOCK | k, k < K, of every (pixel[i], sample[i]): (n, K, 4)"""
    n = len(pixel)
    raw = np.zeros((n, K, 4), F32)
    for i in range(n):
        for k in range(K):
            w = orc.rng_block(int(seed), int(pixel[i]), int(sample[i]), AO_BLOCK | k)
            raw[i, k, :3] = [F32(orc.u32_to_unit_f32(int(w[c]))) - F32(0.5) for c in range(3)]
    return vunit(raw.reshape(-1, 4)).reshape(n, K, 4)


def ao_rays(orc, seed, o4, d4, tri, t, face, norm, pixel, sample, K, bias):
    """The AO rays of the paths that hit, path-major, k fastest: (orig4, dir4, index of each ray's path)"""
    hit = np.nonzero(np.asarray(tri) != 0)[0]
    with np.errstate(all="ignore"):
        point = (d4[hit] * np.asarray(t, F32)[hit, None]).astype(F32) + o4[hit]
        n4 = np.zeros((len(hit), 4), F32)
        n4[:, :3] = norm[np.asarray(tri)[hit]]
        back = (np.asarray(face)[hit] & 1) != 0
        n4[back] = n4[back] * F32(-1.0)
        rv = random_vecs(orc, seed, pixel[hit], sample[hit], K)
        orig = (point + n4 * F32(bias)).astype(F32)
        dirs = vunit((n4[:, None, :] + rv).reshape(-1, 4)).reshape(len(hit), K, 4)
    ao_o = np.ascontiguousarray(np.repeat(orig[:, None, :], K, axis=1).reshape(-1, 4))
    return ao_o, np.ascontiguousarray(dirs.reshape(-1, 4)), np.repeat(hit, K)


def resolve(tri, occ, npix, n, K):
    """ao per pixel from the primaries' hit indices ([pixel][sample]) and the answers of the AO rays (path-major, k fastest)"""
    tri = np.asarray(tri).reshape(npix, n)
    vis_path = np.full(npix * n, K, np.int64)
    hit = np.nonzero(tri.reshape(-1) != 0)[0]
    vis_path[hit] = K - np.asarray(occ, np.int64).reshape(len(hit), K).sum(axis=1)
    visible = vis_path.reshape(npix, n).sum(axis=1)
    return (visible.astype(F32) * (F32(1.0) / F32(n * K))).astype(F32)


def ao_ref(orc, so, w, h, vp12, spp, seed, K, radius=np.inf, bias=0.001, sample0=0, nsamples=None, tile=None, trace=None,
           occluded=None):
    """Expected AO image of oracle scene `so` and everything it was made from.  trace(o4, d4) -> (tri, t, face) and
    occluded(o4, d4, tmax) -> bytes replace the oracle's closest hits and the rule on them (the not-bit-exact modes are held
    against the product's own rtmi_trace / rtmi_occluded).  Returns a namespace: ao (rows, w), o4 / d4 (the AO rays), src (the
    triangle each ray left), occ, nhit (samples that hit), npaths, cn_primary / cn_ao (the oracle's counters for both sets;
    None with a custom trace), ao_tri / ao_t (the AO rays' closest hits, likewise)."""
    rows = list(range(h)) if tile is None else FR.tile_rows(tile)
    o4, d4, npix, n = FR.tile_rays(orc, w, h, vp12, spp, seed, sample0, nsamples, rows)
    cn_primary = cn_ao = ao_tri = ao_t = None
    if trace is None:
        tri, t, face, cn_primary = so.trace(o4, d4)
    else:
        tri, t, face = trace(o4, d4)
    rec, _, _ = so.triangles()
    pixel = np.repeat(np.array([r * w + c for r in rows for c in range(w)], np.int64), n)
    sample = np.tile(np.arange(sample0, sample0 + n, dtype=np.int64), npix)
    ao_o, ao_d, path = ao_rays(orc, seed, o4, d4, tri, t, face, rec[:, 3:6].astype(F32), pixel, sample, K, bias)
    tmax = np.full(ao_o.shape[0], radius, F32)
    if occluded is None:
        if ao_o.shape[0]:
            ao_tri, ao_t, _, cn_ao = so.trace(ao_o, ao_d)
        else:
            ao_tri, ao_t, cn_ao = np.zeros(0, np.uint32), np.zeros(0, F32), dict.fromkeys(orc.COUNTER_NAMES, 0)
        occ = OR.from_hits(ao_tri, ao_t, tmax)
    else:
        occ = occluded(ao_o, ao_d, tmax) if ao_o.shape[0] else np.zeros(0, np.uint8)
    img = resolve(tri, occ, npix, n, K).reshape(len(rows), w)
    return SimpleNamespace(ao=img, o4=ao_o, d4=ao_d, src=np.asarray(tri)[path], occ=occ, nhit=int((np.asarray(tri) != 0).sum()),
                           npaths=npix * n, cn_primary=cn_primary, cn_ao=cn_ao, ao_tri=ao_tri, ao_t=ao_t)
