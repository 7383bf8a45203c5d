"""The definition of the light bake (rtmi_bake*, include/rtmi.h) in float32 NumPy, from the oracle as it is: orc.rng_block /
orc.u32_to_unit_f32 make the draws, ao_ref.random_vecs / ao_ref.vunit the gather directions (rtmi_render_ao*'s two lines with
RNG block 0 and key (pixel0 + m, k)), Scene.trace the closest hits behind `open`.  Every operation is rounded to float32 in the
order the header states, on all four lanes.  The colour of a gather ray is not restated by the call: it is rtmi_render_rays*'s.
To hold it against the oracle, which renders camera rays only, path_colors() follows project_ray pass by pass over
Scene.trace with shadowed_ref's restated lambertian_ray / reflect_ray / mix_color; tests/test_bake_cpu.py pins that loop to
Scene.render before anything trusts it.  A plain helper module of tests/test_bake_cpu.py and tests/test_bake.py."""
from types import SimpleNamespace

import numpy as np

import ao_ref as AR
import shadowed_ref as SR
from features_ref import SKY
from rays_ref import fold

F32 = np.float32
BLOCK_POINT = 0x20000000  # RNG block of the point on a triangle; the direction's random_vec is block 0


def _block0(orc):
    """the oracle's RNG with ao_ref's block AO_BLOCK | k moved to block k: random_vecs(..., K=1) then draws block 0"""
    return SimpleNamespace(rng_block=lambda s, p, k, b: orc.rng_block(s, p, k, b & ~AR.AO_BLOCK), u32_to_unit_f32=orc.u32_to_unit_f32)


def keys(M, K, pixel0=0):
    """(pixel, sample) of ray m K + k: (pixel0 + m, k)"""
    return np.repeat(np.arange(M, dtype=np.int64) + int(pixel0), K), np.tile(np.arange(K, dtype=np.int64), M)


def fold_uv(orc, seed, pixel, sample):
    """(u, v) of every key: the unit floats of words 0 and 1 of block BLOCK_POINT, folded onto the triangle: (n, 2) float32"""
    uv = np.zeros((len(pixel), 2), F32)
    for i in range(len(pixel)):
        w = orc.rng_block(int(seed), int(pixel[i]), int(sample[i]), BLOCK_POINT)
        u, v = F32(orc.u32_to_unit_f32(int(w[0]))), F32(orc.u32_to_unit_f32(int(w[1])))
        if F32(u + v) > F32(1.0):
            u, v = F32(F32(1.0) - u), F32(F32(1.0) - v)
        uv[i] = (u, v)
    return uv


def triangle_points(corners4, uv, K):
    """point = vadd(vadd(c0, vmul(vsub(c1, c0), u)), vmul(vsub(c2, c0), v)) for the K (u, v) of every triangle: (M K, 4)"""
    c = np.asarray(corners4, F32).reshape(-1, 3, 4)
    c0 = np.repeat(c[:, 0], K, axis=0)
    e1 = np.repeat((c[:, 1] - c[:, 0]).astype(F32), K, axis=0)
    e2 = np.repeat((c[:, 2] - c[:, 0]).astype(F32), K, axis=0)
    a = (c0 + (e1 * uv[:, 0:1]).astype(F32)).astype(F32)
    return (a + (e2 * uv[:, 1:2]).astype(F32)).astype(F32)


def rays(orc, seed, pos4, nrm4, K, pixel0=0, bias=0.001, mode="points"):
    """The gather rays of a bake, element-major, k fastest -> namespace(orig (M K, 4), dir (M K, 4), point (M K, 4), uv (M K, 2)
    or None, pixel, sample)"""
    n4 = np.asarray(nrm4, F32).reshape(-1, 4)
    M = n4.shape[0]
    pixel, sample = keys(M, K, pixel0)
    with np.errstate(all="ignore"):
        if mode == "triangles":
            uv = fold_uv(orc, seed, pixel, sample)
            point = triangle_points(pos4, uv, K)
        else:
            uv = None
            point = np.repeat(np.asarray(pos4, F32).reshape(-1, 4), K, axis=0)
        n = np.repeat(n4, K, axis=0)
        rv = AR.random_vecs(_block0(orc), seed, pixel, sample, 1)[:, 0]
        orig = (point + (n * F32(bias)).astype(F32)).astype(F32)
        dirs = AR.vunit((n + rv).astype(F32))
    return SimpleNamespace(orig=np.ascontiguousarray(orig), dir=np.ascontiguousarray(dirs), point=point, uv=uv, pixel=pixel, sample=sample)


def open_from_hits(tri, K):
    """open[m] = (float)misses * (1.f / (float)K) from the closest hits of the rays (element-major, k fastest)"""
    misses = (np.asarray(tri).reshape(-1, K) == 0).sum(axis=1)
    return (misses.astype(F32) * (F32(1.0) / F32(K))).astype(F32)


def path_colors(orc, so, o4, d4, pixel, sample, maxdepth, seed, trace=None):
    """project_ray (raytrace.rs:1199-1295) of explicit rays with RNG keys (pixel, sample): bounce j draws block j.
    -> (colour (n, 4), tri of pass 0, rays traced in all passes).  trace(o4, d4) -> (tri, t, face) replaces the oracle's hits."""
    n = o4.shape[0]
    color = np.zeros((n, 4), F32)
    if maxdepth == 0:
        return color, None, 0
    rec, kinds, surf = so.triangles()
    norms = rec[:, 3:6].astype(F32)
    sky = np.array([SKY[0], SKY[1], SKY[2], 0.0], F32)
    path = np.arange(n)
    cur_o, cur_d = np.ascontiguousarray(o4, F32), np.ascontiguousarray(d4, F32)
    levels, tri0, nrays = [], None, 0
    with np.errstate(all="ignore"):
        for j in range(maxdepth):
            if len(path) == 0:
                break
            nrays += len(path)
            tri, t, face = (so.trace(cur_o, cur_d) if trace is None else trace(cur_o, cur_d))[:3]
            tri, face, t = np.asarray(tri, np.uint32), np.asarray(face, np.uint32), np.asarray(t, F32)
            if j == 0:
                tri0 = tri
            miss = tri == 0
            edge = ~miss & ((face & 2) != 0)
            surface = ~miss & ~edge
            color[path[miss]] = sky
            color[path[edge]] = 0.0
            kind = np.where(surface, kinds[tri], -1)
            col = SR._v4(surf[tri, 0:3].astype(F32))
            solid = kind == SR.SOLID
            color[path[solid]] = col[solid]
            go = surface & ~solid
            levels.append((path[go], col[go], surf[tri[go], 3].astype(F32)))
            if maxdepth - j - 1 == 0:  # project_ray at depth 0: black
                color[path[go]] = 0.0
                break
            point = ((cur_d[go] * t[go, None]).astype(F32) + cur_o[go]).astype(F32)
            nrm = SR._v4(norms[tri[go]])
            back = (face[go] & 1) != 0
            nrm[back] = nrm[back] * F32(-1.0)
            path = path[go]
            rv = SR.random_vec(orc, seed, pixel[path], sample[path], j + 1)
            mo, md = SR.lambertian_ray(point, nrm, rv)
            ro, rd = SR.reflect_ray(point, nrm, cur_d[go], surf[tri[go], 4].astype(F32), rv)
            matte = (kind[go] == SR.MATTE)[:, None]
            cur_o = np.ascontiguousarray(np.where(matte, mo, ro).astype(F32))
            cur_d = np.ascontiguousarray(np.where(matte, md, rd).astype(F32))
        for paths_j, col_j, alpha_j in reversed(levels):
            color[paths_j] = SR.mix_color(col_j, color[paths_j], alpha_j)
    return color, tri0, nrays


def bake_ref(orc, so, seed, pos4, nrm4, K, maxdepth, pixel0=0, bias=0.001, mode="points", want_light=True):
    """Expected outputs of a bake on oracle scene `so` -> namespace(orig, dir, light (M, 4) or None, open (M,), color, rays)"""
    r = rays(orc, seed, pos4, nrm4, K, pixel0, bias, mode)
    if want_light and maxdepth:
        color, tri0, nrays = path_colors(orc, so, r.orig, r.dir, r.pixel, r.sample, maxdepth, seed)
    else:
        color, nrays = np.zeros_like(r.orig), r.orig.shape[0]
        tri0 = np.asarray(so.trace(r.orig, r.dir)[0])
    return SimpleNamespace(orig=r.orig, dir=r.dir, uv=r.uv, light=fold(color, K), open=open_from_hits(tri0, K), color=color, rays=nrays)


# ---------------------------------------------------------------- the elements the two test files share
ANCHOR = dict(w=16, h=16, seed=7, K=4, maxdepth=4, pixel0=1000, npoints=20)
SKY_POINT = ((0.0, 45.0, 20.0, 0.0), (0.0, 1.0, 0.0, 0.0))  # above the canonical root box (centre (0, 0, 20.1), half edge 20), facing away


def first_hit_points(orc, so, w, h, limit=None):
    """(pos4, nrm4) of the first hits of the canonical w x h view at one sample per pixel, in pixel order: point = rd * t + ro,
    the triangle's norm negated on a back face (the features call's normal); edge faces included"""
    o4, d4 = orc.primary_rays(w, h, orc.canonical_viewport(w, h), 1)
    tri, t, face, _ = so.trace(o4, d4)
    hit = np.nonzero(np.asarray(tri) != 0)[0][:limit]
    rec, _, _ = so.triangles()
    pos = ((d4[hit] * np.asarray(t, F32)[hit, None]).astype(F32) + o4[hit]).astype(F32)
    nrm = np.zeros((len(hit), 4), F32)
    nrm[:, :3] = rec[np.asarray(tri)[hit], 3:6]
    back = (np.asarray(face)[hit] & 1) != 0
    nrm[back] = nrm[back] * F32(-1.0)
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm)


def anchor_elements(orc, so):
    """ANCHOR's points: about 20 first hits of the canonical 16 x 16 view, then SKY_POINT (all of whose rays miss)"""
    a = ANCHOR
    pos, nrm = first_hit_points(orc, so, a["w"], a["h"], a["npoints"])
    return (np.ascontiguousarray(np.concatenate([pos, np.array([SKY_POINT[0]], F32)])),
            np.ascontiguousarray(np.concatenate([nrm, np.array([SKY_POINT[1]], F32)])))


def scene_triangles(so, first=1, count=40):
    """(corners4 (3 count, 4), nrm4 (2 count, 4) ...) of triangles [first, first + count) of the scene from their make_triangle
    corners, each baked on both sides: 2 count elements, the front sides first"""
    rec, _, _ = so.triangles()
    c = np.zeros((count, 3, 4), F32)
    c[:, :, :3] = rec[first:first + count, 20:29].reshape(count, 3, 3)
    n = np.zeros((count, 4), F32)
    n[:, :3] = rec[first:first + count, 3:6]
    neg = (n * F32(-1.0)).astype(F32)
    neg[:, 3] = 0.0  # lane 3 = +0 on both sides
    return np.ascontiguousarray(np.concatenate([c, c]).reshape(-1, 4)), np.ascontiguousarray(np.concatenate([n, neg]))
